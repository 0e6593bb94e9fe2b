"""Scenes of tests/test_byte_family_cases.py (CPU: the oracles say which assignment regimes and life-cycle events the scenes reach) and
of tests/test_gpu_byte_family_pinned.py (GPU: the ByteTrack and BoT-SORT epoch kernels replay them and must give, bit for bit, what
tests/golden/byte_family_state.npz holds; tests/golden/make_byte_family_state.py recorded it through the same functions).

Both trackers run every scene with track_buffer = 5, so that the lost timeout falls inside the long small scene; BoT-SORT gets
64-float features (synthetic.identity_features) and, on the small scene, a camera-motion warp on most frames.  Every scene is run
under lsap_fast 0 / 1 and epoch_frames 1 / 0, and the 12- and 40-target scenes once more as a ragged two-stream bank."""
import os
import sys
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KINDS = ("bytetrack", "botsort")
DIM = 64
PARAMS = {"bytetrack": dict(track_buffer=5), "botsort": dict(track_buffer=5, feature_dim=DIM)}
ARENA_SIDE = {"bytetrack": 111, "botsort": 107}                  # largest extended side whose matrix fits the kernel's LDS arena
CONFIGS = ((1, 1), (0, 1), (1, 0), (0, 0))                       # (lsap_fast, epoch_frames)
CLOCKS = ("cost_cycles", "kernel_cycles")                        # shader-clock totals: not recorded
REGIMES = ("side<=64", "64<side<=arena", "arena<side<=128", "128<side<=512")
EVENTS = ("lost", "refound", "timed_out", "unconfirmed_removed")


@dataclass
class FamilyScene:
    id: str
    n: int
    frames: int
    seed: int
    chunk: int                                                   # frames per update call
    long: bool = False                                           # gaps, births and warps: the life-cycle scene
    kw: dict = field(default_factory=dict)

    def scene(self):
        from conftest import pkg
        kw = dict(conf_range=(0.05, 0.95), jitter=1.5, shuffle=True)
        if self.long:                                            # the occlusions and late births of test_gpu_bytetrack.scene
            rng = np.random.default_rng(self.seed)
            n, frames = self.n, self.frames
            kw["gaps"] = [(int(t), int(a), int(a + rng.integers(3, 20))) for t, a in zip(rng.integers(0, n, n), rng.integers(5, frames - 20, n))]
            kw["births"] = {int(t): int(f) for t, f in zip(rng.choice(n, n // 4, replace=False), rng.integers(1, frames // 2, n // 4))}
        else:                                                    # the crowd of test_crowd_exercises_the_large_lsap
            kw.update(jitter=2.0, w_range=(30.0, 50.0), h_range=(80.0, 120.0))
        kw.update(self.kw)
        return pkg("synthetic").Scene(seed=self.seed, n_targets=self.n, **kw)

    def warps(self):
        if not self.long:
            return [None] * self.frames
        th = 0.004 * np.sin(np.arange(self.frames) * 0.7)
        w = [np.array([[np.cos(t), -np.sin(t), 1.5 * np.cos(i)], [np.sin(t), np.cos(t), -0.75 * np.sin(i)]], np.float32) for i, t in enumerate(th)]
        for i in range(5, self.frames, 6):                       # frames without an estimate: the identity
            w[i] = None
        return w


SCENES = (FamilyScene("small12", 12, 60, 9, 7, long=True),
          FamilyScene("crowd40", 40, 8, 21, 8),
          FamilyScene("crowd100", 100, 8, 22, 5),
          FamilyScene("crowd150", 150, 8, 21, 3, kw=dict(conf_range=(0.15, 0.95))))
BANK = ("small12", "crowd40")                                    # the streams of the bank run
BANK_PLAN = ((7, 3), (0, 5), (16, 0), (37, 0))                   # frames per call and stream: ragged, with a stream absent from a call
# What the oracles meet on each scene: (non-empty assignment problems, largest extended side).  tests/test_byte_family_cases.py holds
# the oracles to these figures and to the regimes behind them; the device's counters must show the same figures.
PROMISED = {"bytetrack": {"small12": (136, 19), "crowd40": (20, 51), "crowd100": (20, 114), "crowd150": (20, 192)},
            "botsort": {"small12": (135, 16), "crowd40": (20, 38), "crowd100": (20, 97), "crowd150": (20, 144)}}
_FRAMES = {}


def scene_of(sid):
    return next(s for s in SCENES if s.id == sid)


def frames_of(sid, kind):
    """Per frame (boxes, scores, cls) for ByteTrack, (boxes, scores, cls, raw features, warp or None) for BoT-SORT; computed once."""
    if (sid, kind) not in _FRAMES:
        from conftest import pkg
        syn = pkg("synthetic")
        fs = scene_of(sid)
        sc, warps, out = fs.scene(), fs.warps(), []
        for f in range(fs.frames):
            b, c, k, ident = sc.detections(f)
            k = (k + (np.arange(len(k)) % 3)).astype(np.int32)   # a few classes: cls follows the last matched detection
            if kind == "bytetrack":
                out.append((b, c, k))
            else:                                                # not unit length: the device normalises
                ft = (syn.identity_features(ident, f, dim=DIM, seed=7) * np.float32(1.5 + 0.01 * f)).astype(np.float32)
                out.append((b, c, k, ft, warps[f]))
        _FRAMES[sid, kind] = out
    return _FRAMES[sid, kind]


def regime(kind, side):
    return REGIMES[0 if side <= 64 else 1 if side <= ARENA_SIDE[kind] else 2 if side <= 128 else 3]


# ------------------------------------------------------------------------------------------------------------------ the oracles
def oracle_run(kind, sid):
    """The oracle over the scene -> (extended sides of its non-empty assignment problems, life-cycle events seen, appearance pairs)."""
    import botsort_oracle
    import bytetrack_oracle
    mod = bytetrack_oracle if kind == "bytetrack" else botsort_oracle
    sides, events = [], set()
    inner = mod.linear_assignment

    def recording(cost, thresh):
        if np.asarray(cost).size:
            sides.append(int(sum(np.asarray(cost).shape)))
        return inner(cost, thresh)

    mod.linear_assignment = recording
    try:
        kw = {k: v for k, v in PARAMS[kind].items() if k != "feature_dim"}
        ora = mod.BYTETracker(**kw) if kind == "bytetrack" else mod.BoTSORT(**kw)
        for fr in frames_of(sid, kind):
            tracked, lost = list(ora.tracked_stracks), list(ora.lost_stracks)
            unconfirmed = [t for t in tracked if not t.is_activated]
            ora.update_xyxy(*fr)
            now_t, now_l = set(map(id, ora.tracked_stracks)), set(map(id, ora.lost_stracks))
            if any(id(t) in now_l for t in tracked):
                events.add("lost")
            if any(id(t) in now_t for t in lost):
                events.add("refound")
            if any(t.state == mod.REMOVED and ora.frame_id - t.end_frame > ora.max_time_lost for t in lost):
                events.add("timed_out")
            if any(t.state == mod.REMOVED for t in unconfirmed):
                events.add("unconfirmed_removed")
    finally:
        mod.linear_assignment = inner
    return sides, events, getattr(ora, "n_appearance", 0)


# ------------------------------------------------------------------------------------------------------------------ the device
def _flat(prefix, per_frame, rec):
    rec[prefix + "/n"] = np.array([len(r) for r, _ in per_frame], np.int32)
    rec[prefix + "/rows"] = np.concatenate([r for r, _ in per_frame] + [np.zeros((0, 6), np.int32)]).astype(np.int32)
    rec[prefix + "/conf"] = np.concatenate([c for _, c in per_frame] + [np.zeros(0, np.float32)]).astype(np.float32)


def _state(prefix, export, counters, rec):
    for k, v in export.items():
        rec[f"{prefix}/export/{k}"] = np.asarray(v)
    for k, v in counters.items():
        if k not in CLOCKS:
            rec[f"{prefix}/counters/{k}"] = np.array(v, np.int64)


def device_run(kind, sid, lsap_fast, epoch_frames):
    """The public single-tracker class over the scene -> {name: array}: every frame's rows and conf, the final export(), counters()."""
    from conftest import pkg
    fs = scene_of(sid)
    dev = pkg(kind).BYTETracker(**PARAMS[kind]) if kind == "bytetrack" else pkg(kind).BoTSORT(**PARAMS[kind])
    dev.option("lsap_fast", lsap_fast)
    dev.option("epoch_frames", epoch_frames)
    frames, got = frames_of(sid, kind), []
    for f in range(0, len(frames), fs.chunk):
        got += dev.update_batch_arrays(frames[f:f + fs.chunk])
    rec = {}
    _flat("frames", got, rec)
    _state("final", dev.export(), dev.counters(), rec)
    dev.close()
    return rec


def bank_run(kind, lsap_fast, epoch_frames):
    """The public bank class over the scenes of BANK under the ragged BANK_PLAN -> {name: array}, per stream as device_run."""
    from conftest import pkg
    S = len(BANK)
    bk = pkg(kind).BYTETrackerBank(S, **PARAMS[kind]) if kind == "bytetrack" else pkg(kind).BoTSORTBank(S, **PARAMS[kind])
    bk.option("lsap_fast", lsap_fast)
    bk.option("epoch_frames", epoch_frames)
    dets = [frames_of(sid, kind) for sid in BANK]
    pos, got = [0] * S, [[] for _ in range(S)]
    for call in BANK_PLAN:
        parts = [dets[s][pos[s]:pos[s] + call[s]] for s in range(S)]
        res = bk.update_arrays(parts)
        for s in range(S):
            got[s] += res[s]
            pos[s] += len(parts[s])
    rec = {}
    for s in range(S):
        _flat(f"stream{s}/frames", got[s], rec)
        _state(f"stream{s}/final", bk.export(s), bk.counters(s), rec)
    bk.close()
    return rec


def runs():
    """(name, function) of every recorded run: name = kind/scene or kind/bank, then /fast{lsap_fast}_epoch{epoch_frames}."""
    for kind in KINDS:
        for lf, ef in CONFIGS:
            cfg = f"fast{lf}_epoch{ef}"
            for fs in SCENES:
                yield f"{kind}/{fs.id}/{cfg}", (lambda kind=kind, sid=fs.id, lf=lf, ef=ef: device_run(kind, sid, lf, ef))
            yield f"{kind}/bank/{cfg}", (lambda kind=kind, lf=lf, ef=ef: bank_run(kind, lf, ef))


# A run whose arrays (the counters aside) equal, bit for bit, those of the same scene's first configuration is stored as that statement,
# "<run>/same_as_first" = 1; expected() undoes it.  Nothing is left out: the replayed run is still compared with every array.
def _first(name):
    return name.rsplit("/", 1)[0] + "/fast%d_epoch%d" % CONFIGS[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def pack(records):
    """{run: {name: array}} -> the flat dict np.savez takes."""
    out = {}
    for run, rec in records.items():
        first = records[_first(run)]
        plain = {k: v for k, v in rec.items() if "/counters/" not in k}
        dup = run != _first(run) and plain.keys() == {k for k in first if "/counters/" not in k} and all(same_bits(v, first[k]) for k, v in plain.items())
        if dup:
            out[run + "/same_as_first"] = np.array(1, np.int32)
        for k, v in rec.items():
            if not dup or "/counters/" in k:
                out[f"{run}/{k}"] = v
    return out


def expected(npz, run):
    """What the fixture holds for `run`: {name: array}."""
    keys = list(npz.keys())
    rec = {k[len(run) + 1:]: npz[k] for k in keys if k.startswith(run + "/") and not k.endswith("/same_as_first")}
    if run + "/same_as_first" in keys:
        f = _first(run)
        rec.update({k[len(f) + 1:]: npz[k] for k in keys if k.startswith(f + "/") and "/counters/" not in k})
    return rec
