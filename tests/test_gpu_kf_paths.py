"""Every device path of the xyah Kalman filter, element by element against float64 (tests/kf_ref.py) and bit for bit against its siblings.
The arithmetic has one home, csrc/trk_math.hpp: kf_predict_wave / kf_update_wave / kf_initiate_wave (a per-lane compute part, then the
fenced stores) and the update's pieces kf_gain_row / kf_s_gain / kf_mean_elem / kf_cov_elem.  The forms are the kernels that call it, each
with its own way of choosing the track, the measurement and where the state lives (tests/test_trk_math_host.py runs the same header on
the CPU):

  form 1   kf_*_kernel of kernels_trk.hip (one kf_*_wave call each) through the aic_kf_* entries    test_form1_*, test_gating_*
  form 2   trk_commit_kernel: TrackerCore.update_arrays on the host path                       test_planted_frame[host]
  form 4   the kf_*_wave functions inside an epoch kernel: ByteTrack's, and the DeepSORT epoch kernel
           once 72 T floats no longer fit its LDS arena (193 tracks, derived in kf_ref.epoch_arena_floats)
                                                                                               test_bytetrack_*, test_epoch_kernel_both_update_forms
  form 5   the DeepSORT epoch kernel's thread-per-row update, written on the update's pieces: device_assoc = 1 frame by frame (three full
           cost matrices in HBM), and update_batch (the lean cost matrix in the arena the update then overwrites)
                                                                                               test_planted_frame[device], [batch]
  form 6   the same kernel as block 1 of a two-stream bank launch                              test_bank_stream_*
  form 3   the commit in front of trk_assoc_all_kernel (launch_trk_step) runs only when a PIPELINE on the host chain hands the next
           frame's detections to Tracker::update; no entry of the tracker's own C ABI reaches it (aic_tracker_update_batch always runs
           the epoch kernels).  A three-frame launch group with the state planted in the pipeline's tracker           test_pipeline_stepped_commit

Allowances: max(4 x the figure of the fp32 NumPy restatement on the same inputs in the same metric, 8 x 2^-24), measured on the CPU in
tests/test_kf_ref.py, never against the device.  Tracker paths start from ONE planted state (kf_ref.plan: 28 case states as confirmed
tracks, one gallery row each, nine tentative decoys between them), see one frame whose shuffled detections sit on the predicted boxes,
and must report exactly the planned pairing.  aic_tracker_import_state gives track i slot i and the decoys are pruned after the
commit, so in that frame the slot still equals the list position; what the decoys separate from the slot is the position among the
MATCHED tracks (upd_slot[m] of trk_commit_kernel, the row of the output boxes).  List position != slot is met from the second frame on:
test_sixteen_frame_epoch, test_pipeline_stepped_commit, and the second frames of test_epoch_kernel_both_update_forms."""
import functools

import numpy as np
import pytest

import kf_ref as K
from conftest import assert_rows_equal_or_on_rounding_edge, pkg
from oracle import deepsort_oracle as O
from test_kf_ref import FALLBACK_T, OracleKF, base_plan, big_plan, check_plan, oracle_figures, oracle_step, pipeline_plan, step_figures

pytestmark = pytest.mark.gpu

BUDGET = 20                                      # >= 16: a sixteen-frame epoch is one launch (an epoch never outruns the gallery budget)
STATE_KEYS = ("track_id", "state", "hits", "age", "time_since_update", "cls", "gallery_len", "conf", "mean", "cov")


class GpuKF:
    """core.kalman_filter.KalmanFilter (one launch of a form-1 kernel per call) with the interface kf_ref.measure takes."""

    def __init__(self, lib):
        self.lib, self.KF = lib, pkg("core.kalman_filter").KalmanFilter

    def initiate(self, z):
        return self.KF().initiate(z)

    def predict(self, mean, cov, dt=1.0):
        return self.KF(dt=dt).predict(mean, cov)

    def project(self, mean, cov):
        return self.KF().project(mean, cov)

    def update(self, mean, cov, z):
        return self.KF().update(mean, cov, z)

    def gating(self, mean, cov, zs, shared_z, only_position):
        L = self.lib
        n, m = len(mean), zs.shape[-2]
        mean, cov, zs = L.as_f32(mean), L.as_f32(cov), L.as_f32(zs)
        d2 = np.full((n, m), np.nan, np.float32)
        L.call("aic_kf_gating", 0, L.ptr(mean), L.ptr(cov), n, L.ptr(zs), m, int(shared_z), int(only_position), L.ptr(d2))
        return d2


# ------------------------------------------------------------------------------------------------------------------ (a) form 1
N_WAVE, N_THREAD = (1, 3, 4, 5, 257), (1, 63, 64, 65)             # four waves per 256-thread block; project: 64 threads per block


def test_form1_bit_equal_to_restatement(gpu, lib):
    """initiate, predict at dt = 1 and project: the kernels' header claims the reference's bits."""
    kf, orc = GpuKF(lib), OracleKF()
    for bi, n in enumerate(N_WAVE):
        mean, cov, z = K.batch(K.cyclic(n, 13 * bi))
        for got, want in ((kf.initiate(z), orc.initiate(z)), (kf.predict(mean, cov), orc.predict(mean, cov))):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n
    for bi, n in enumerate(N_THREAD):
        mean, cov, _ = K.batch(K.cyclic(n, 17 * bi))
        got, want = kf.project(mean, cov), orc.project(mean, cov)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n


def test_form1_against_fp64(gpu, lib):
    fig, _ = oracle_figures()
    dev = K.measure(GpuKF(lib), n_list=N_WAVE, project_n=N_THREAD)
    for k in sorted(dev):
        print(f"form 1 {k}: covariance {dev[k][0]:.2e} of {K.allow(fig[k][0]):.2e}, mean {dev[k][1]:.2e} of {K.allow(fig[k][1]):.2e}")
    # measured on MI355X (covariance, mean; allowed): initiate 1.2e-7, 0 (4.8e-7: the floor)   project 9.4e-8, 0 (4.8e-7)
    #   predict dt 1 / 0.5 / 2 / 1/30: 9.1e-8 / 1.1e-7 / 1.0e-7 / 1.1e-7, 5.5e-8 .. 5.9e-8 (4.8e-7): the restatement's own figures to three digits
    #   update 2.8e-7 (1.3e-6), 2.1e-7 (7.8e-7); the restatement: 3.2e-7, 1.9e-7
    for k in dev:
        assert dev[k][0] <= K.allow(fig[k][0]) and dev[k][1] <= K.allow(fig[k][1]), (k, dev[k], fig[k])


def test_gating_against_fp64(gpu, lib):
    """aic_kf_gating itself: 1 and 5 tracks, 1 .. 200 measurements (the block strides by 64), shared and per-track measurements (a wrong
    row offset reads another track's), position only and all four components, the three states that are not positive definite."""
    fig, _ = oracle_figures()
    recs = K.gate_runs(GpuKF(lib).gating)
    dev = K.gate_figure(recs)                                       # (also asserts that exactly the +inf cells of float64 are +inf)
    print(f"form 1 gating: {dev:.2e} of {K.allow(fig['gating']):.2e} over {sum(r[5].size for r in recs)} cells")
    assert dev <= K.allow(fig["gating"])                             # measured on MI355X: 4.3e-7 of 1.8e-6 over 163 488 cells (the restatement: 4.4e-7)
    for r, s in zip(recs, K.gate_sure(recs, fig["gating"])):
        assert np.array_equal((r[6] > K.CHI2_4)[s], (r[5] > K.CHI2_4)[s]), r[:5]


# ------------------------------------------------------------------------------------------------------------------ (b) tracker paths
def import_plan(p, trk=None, galleries=True, **opts):
    """The plan's state in a TrackerCore (a new one on the host path unless given): ids 1 .. T in list order, one gallery row per confirmed
    track, or none at all."""
    if trk is None:
        trk = pkg("core.tracker_core").TrackerCore(nn_budget=BUDGET)
    t = len(p.mean)
    conf = p.state == 2
    st = dict(track_id=np.arange(1, t + 1), state=p.state, hits=np.where(conf, 5, 1), age=np.full(t, 5), time_since_update=np.zeros(t),
              cls=np.zeros(t), conf=np.full(t, 0.9, np.float32), gallery_len=conf.astype(np.int32) if galleries else np.zeros(t, np.int32),
              mean=p.mean, cov=p.cov, galleries=p.feat[conf] if galleries else np.zeros((0, 1), np.float32), dim=K.DIM if galleries else 0,
              next_track_id=t + 1)
    trk.import_state(st)
    for k, v in opts.items():
        trk.option(k, v)
    return trk


def frame_of(p, det=None):
    n = len(p.det)
    return (p.det if det is None else det, np.full(n, 0.9, np.float32), np.zeros(n, np.int32), p.det_feat, np.ones(n, np.uint8))


def run_frame(p, path):
    """The planted frame through one path: (export_arrays after it, matches, rows, the tracker)."""
    if path == "host":
        trk = import_plan(p)
    elif path == "device":
        trk = import_plan(p, device_assoc=1, epoch_frames=1)
    else:
        trk = import_plan(p)
    if path == "batch":
        rows, _, matches = trk.update_batch([frame_of(p)])[0]
    else:
        trk.predict()
        trk.update_arrays(*frame_of(p))
        rows, matches = trk.outputs()[0], trk.last_matches()
    return trk.export_arrays(), matches, rows, trk


def form1_step(lib, p):
    """Form 1 on the plan's inputs: aic_kf_predict, then aic_kf_update with the planned measurement.  {list position: (mean, cov)}."""
    kf, z = GpuKF(lib), K.xyah32(p.det)
    ts = sorted(p.pair)
    pm, pp = kf.predict(p.mean[ts], p.cov[ts])
    want = OracleKF().predict(p.mean[ts], p.cov[ts])
    assert np.array_equal(pm, want[0]) and np.array_equal(pp, want[1])
    um, uc = kf.update(pm, pp, z[[p.pair[t] for t in ts]])
    return {t: (um[i], uc[i]) for i, t in enumerate(ts)}


def expected_rows(p):
    """x1, y1, x2, y2 of the float64 updated states of the planned pairs, list order, before rounding."""
    want = K.expected_step(p)
    b = np.array([K.mean_to_tlwh(want[t][0]) for t in sorted(p.pair)])
    return np.stack([b[:, 0], b[:, 1], b[:, 0] + b[:, 2], b[:, 1] + b[:, 3]], 1)


def check_frame(p, lib, exported, matches, rows, where, ids=None, next_id=None, hits=6):
    """Matches, state, rows and new tracks of the planted frame (ids: the track id of every list position of the plan, 1 .. T as import_plan
    gives them unless told; next_id: the first new track's).  Returns the state by list position, {position: (mean, cov)}."""
    ts = sorted(p.pair)
    ids = list(range(1, len(p.mean) + 1)) if ids is None else [int(i) for i in ids]
    next_id = len(p.mean) + 1 if next_id is None else next_id
    assert sorted(matches) == sorted((ids[t], p.pair[t]) for t in ts), where
    row = {int(tid): k for k, tid in enumerate(exported["track_id"])}
    assert sorted(row) == [ids[t] for t in ts] + [next_id + q for q in range(len(p.new))], where    # decoys gone, three new tracks
    got = {t: (exported["mean"][row[ids[t]]], exported["cov"][row[ids[t]]]) for t in ts}
    assert all(exported["time_since_update"][row[ids[t]]] == 0 and exported["hits"][row[ids[t]]] == hits for t in ts), where
    # ---- float64
    c, m, c2, m2 = step_figures(p, got)
    oc, om, oc2, om2 = step_figures(p, oracle_step(p))
    print(f"{where}: covariance {c:.2e} of {K.allow(oc):.2e}, mean {m:.2e} of {K.allow(om):.2e} in one piece; covariance {c2:.2e} of "
          f"{K.allow(oc2):.2e}, mean {m2:.2e} of {K.allow(om2):.2e} from the fp32 predicted state")
    # measured on MI355X, the same on every path (host, device, batch): covariance 2.1e-7 of 1.3e-6 and mean 1.0e-2 of 4.0e-2 in one piece (the
    # restatement is at 1.0e-2 itself: step_figures says why); covariance 1.9e-7 of 1.3e-6 and mean 1.6e-7 of 6.5e-7 from the fp32 predicted
    # state.  192 / 193 tracks (second frame): 2.6e-7 of 1.3e-6, 1.1e-1 of 4.3e-1; 2.7e-7 of 1.3e-6, 1.3e-7 of 8.0e-7
    assert c <= K.allow(oc) and m <= K.allow(om) and c2 <= K.allow(oc2) and m2 <= K.allow(om2), where
    # ---- output rows: the confirmed tracks updated in this frame, list order
    exp = expected_rows(p)
    assert rows[:, 4].tolist() == [ids[t] for t in ts], where
    assert_rows_equal_or_on_rounding_edge(rows[:, :4], np.rint(exp), exp, where)
    # ---- new tracks: the restatement's bits, ascending detection row -> ascending id
    z = K.xyah32(p.det)
    for q, j in enumerate(p.new):
        k = row[next_id + q]
        im, ic = O.kf_initiate(z[j])
        assert np.array_equal(exported["mean"][k], im) and np.array_equal(exported["cov"][k], ic), (where, q)
        assert exported["state"][k] == 1 and exported["gallery_len"][k] == 1
    # ---- form 1 on the same inputs: the same fp32 operations in the same order, contraction off
    f1 = form1_step(lib, p)
    for t in ts:
        assert np.array_equal(got[t][0], f1[t][0]) and np.array_equal(got[t][1], f1[t][1]), (where, t)
    return got


@functools.lru_cache(maxsize=None)
def planted_frame(path):
    return run_frame(base_plan(), path)


@pytest.mark.parametrize("path", ["host", "device", "batch"])
def test_planted_frame(gpu, lib, path):
    exported, matches, rows, _ = planted_frame(path)
    check_frame(base_plan(), lib, exported, matches, rows, path)


def test_planted_frame_paths_agree(gpu):
    """The exports of the three paths are equal in every field, and stay so through an empty frame (predict alone; the three tentative
    tracks are deleted; for update_batch the empty frame is the second of a two-frame call: the epoch kernel's n = 0 frame)."""
    host = planted_frame("host")
    for path in ("device", "batch"):
        other = planted_frame(path)
        for key in STATE_KEYS:
            assert np.array_equal(host[0][key], other[0][key]), (path, key)
        assert np.array_equal(host[2], other[2]), path
    p = base_plan()
    empty = (np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), None, None)
    trk = host[3]
    trk.predict()
    trk.update_arrays(*empty)
    two = import_plan(p)
    res = two.update_batch([frame_of(p), empty])
    assert np.array_equal(res[0][0], host[2]) and len(res[1][0]) == 0
    a, b = trk.export_arrays(), two.export_arrays()
    assert len(a["track_id"]) == len(p.pair)
    for key in STATE_KEYS:
        assert np.array_equal(a[key], b[key]), key
    for k, t in enumerate(sorted(p.pair)):                           # the predict of the empty frame, the restatement's bits
        pm, pc = O.kf_predict(host[0]["mean"][k], host[0]["cov"][k])
        assert np.array_equal(a["mean"][k], pm) and np.array_equal(a["cov"][k], pc), t


def test_epoch_kernel_both_update_forms(gpu, lib):
    """`72 * T <= L.arena_floats` in trk_epoch_kernel: 192 tracks take the thread-per-row update (form 5), 193 the wave per track
    (kf_update_wave, form 4) -- kf_ref.first_fallback_tracks, the arithmetic asserted in tests/test_kf_ref.py.  Nothing at run time says
    which form a launch took: the two counts stand on that restatement of lds_carve (test_epoch_kernel_fallback_threshold).
    Two frames each.  The first (big_plan: the tracks with a tentative decoy after every third, 256 / 257 in all) only prunes the decoys,
    so that in the second the track at list position t holds Kalman slot t + t // 3 (import_state gives track i slot i) -- below 96 in
    LDS, from 96 on in HBM.  The second, built on the state exported in between, has exactly 192 / 193 tracks and 195 / 196 detections: it
    is held to float64 and to form 1, and the 192 tracks the two runs share are equal bit for bit."""
    assert FALLBACK_T is not None and FALLBACK_T <= 512
    got = {}
    for n in (FALLBACK_T - 1, FALLBACK_T):
        first = big_plan(n)
        trk = import_plan(first, device_assoc=1, epoch_frames=1)
        trk.predict()
        trk.update_arrays(*frame_of(first))
        assert sorted(trk.last_matches()) == sorted((t + 1, j) for t, j in first.pair.items()), n
        st = trk.export_arrays()
        slots = st["track_id"] - 1                                   # the list position at import = the slot, for good
        assert len(slots) == n and (st["hits"] == 6).all() and (slots != np.arange(n)).sum() == n - 3 and (slots >= 96).sum() > 100
        p = K.plan_states(st["mean"], st["cov"], decoy_every=0, seed=n)
        check_plan(p, gate_tells_apart=True)
        assert len(p.mean) == n and len(p.det) == n + 3
        trk.predict()
        trk.update_arrays(*frame_of(p))
        got[n] = check_frame(p, lib, trk.export_arrays(), trk.last_matches(), trk.outputs()[0], f"device, {n} tracks", ids=st["track_id"],
                             next_id=len(first.mean) + 1, hits=7)
    for t in got[FALLBACK_T - 1]:
        for a, b in zip(got[FALLBACK_T - 1][t], got[FALLBACK_T][t]):
            assert np.array_equal(a, b), t


def test_sixteen_frame_epoch(gpu):
    """Sixteen frames of the planted frame's boxes, each going on at its track's velocity and drifting by 0.3 % of its size a frame
    (kf_ref.drift_frames; the float64 filter keeps every pair inside half the gate, tests/test_kf_ref.py): ONE sixteen-frame epoch, sixteen one-frame
    epochs and the host path leave the same state and write the same rows (the first frame is test_planted_frame's)."""
    p = base_plan()
    frames = [frame_of(p, det) for det in K.drift_frames(p, 16)]
    host, dev, batch = import_plan(p), import_plan(p, device_assoc=1, epoch_frames=1), import_plan(p, epoch_frames=16)
    res = batch.update_batch(frames)
    for i, fr in enumerate(frames):
        for trk in (host, dev):
            trk.predict()
            trk.update_arrays(*fr)
        assert sorted(host.last_matches()) == sorted(dev.last_matches()) == sorted(res[i][2]), i
        assert {(t + 1, j) for t, j in p.pair.items()} <= set(res[i][2]), i           # every planted track is found in every frame
        assert np.array_equal(host.outputs()[0], dev.outputs()[0]) and np.array_equal(host.outputs()[0], res[i][0]), i
    a = host.export_arrays()
    assert a["track_id"][:len(p.pair)].tolist() == [t + 1 for t in sorted(p.pair)] and (a["hits"][:len(p.pair)] == 21).all()
    for other in (dev.export_arrays(), batch.export_arrays()):
        for key in STATE_KEYS:
            assert np.array_equal(a[key], other[key]), key


def test_pipeline_stepped_commit(gpu, engines):
    """Form 3.  A pipeline on the host chain ("device_assoc" 0) walks a launch group of four frames, the third of them EMPTY.  Tracker::update
    is given the next frame's detections, so the commit of a frame rides in trk_assoc_all_kernel in front of the next frame's rows:
      frame 0   Kalman updates and initiates, then the in-place predict and the cost rows of frame 1;
      frame 1   Kalman updates only -- the next frame has no detection, the blocks leave at the block-uniform `if (n <= 0) return`;
      frame 2   (empty) nothing to commit, the predict and the cost rows of frame 3 alone;
      frame 3   the last of the group: trk_commit_kernel (without galleries nobody is matched two frames after an update; 31 initiates).
    The state is planted in the pipeline's own tracker; every box
    lies left of the image, so nothing has a feature and the IoU stage alone pairs tracks and detections (unambiguous: asserted in
    tests/test_kf_ref.py).  A TrackerCore on the host path (form 2 in every frame) fed the same boxes must end in the same state bit for
    bit and write the same rows, and its first frame is held to float64 here as the planted frame's is."""
    p, xyxy, tlwh = pipeline_plan()
    none = np.zeros((0, 4), np.float32)
    xyxy, tlwh = xyxy[:2] + [none, xyxy[3]], tlwh[:2] + [none, tlwh[3]]
    n = len(p.det)
    conf, cls = np.full(n, 0.9, np.float32), np.zeros(n, np.int32)
    pipe = pkg("pipeline").TrackingPipeline(engines[0], engines[1], (720, 1280), batch=4, ring_frames=4, max_persons=64, dtype="fp16", inject=True,
                                            nn_budget=BUDGET)
    pipe.option("device_assoc", 0)
    pipe.option("taper", 0)                                         # one launch group of four frames, no shrinking tail
    pipe.upload(0, np.zeros((4, 720, 1280, 3), np.uint8))
    pipe.inject(0, [(b, conf[:len(b)], cls[:len(b)]) for b in xyxy])
    import_plan(p, trk=pipe.tracker_core, galleries=False)
    tracks, _ = pipe.run(0, 4)
    assert pipe.counters()["assoc_host_frames"] == 4
    host = import_plan(p, galleries=False)
    for f in range(4):
        host.predict()
        host.update_arrays(tlwh[f], conf[:len(tlwh[f])], cls[:len(tlwh[f])], None)
        rows = host.outputs()[0]
        assert [t[:5] for t in tracks[f]] == [tuple(r[:5]) for r in rows.tolist()], f
        assert len(rows) == (len(p.pair) if f < 2 else 0), f
        if f == 1:
            assert len(host.last_matches()) == len(p.pair) + 3     # the commit that meets the empty frame carries 31 Kalman updates
        if f == 0:
            after = host.export_arrays()
            ts = sorted(p.pair)
            assert sorted(host.last_matches()) == sorted((t + 1, p.pair[t]) for t in ts)
            row = {int(tid): k for k, tid in enumerate(after["track_id"])}
            got = {t: (after["mean"][row[t + 1]], after["cov"][row[t + 1]]) for t in ts}
            c, m, c2, m2 = step_figures(p, got)
            oc, om, oc2, om2 = step_figures(p, oracle_step(p))
            print(f"pipeline plan, host path frame 0: covariance {c:.2e} of {K.allow(oc):.2e}, mean {m:.2e} of {K.allow(om):.2e} in one piece; "
                  f"covariance {c2:.2e} of {K.allow(oc2):.2e}, mean {m2:.2e} of {K.allow(om2):.2e} from the fp32 predicted state")
            # measured on MI355X: 2.1e-7 of 1.3e-6, 3.0e-3 of 1.2e-2; 1.9e-7 of 1.3e-6, 1.4e-7 of 7.0e-7
            assert c <= K.allow(oc) and m <= K.allow(om) and c2 <= K.allow(oc2) and m2 <= K.allow(om2)
            assert_rows_equal_or_on_rounding_edge(rows[:, :4], np.rint(expected_rows(p)), expected_rows(p), "pipeline plan")
    a, b = host.export_arrays(), pipe.tracker_core.export_arrays()
    t = len(p.pair)
    assert len(a["track_id"]) == t + n and (a["gallery_len"] == 0).all() and (a["hits"][:t] == 7).all() and (a["time_since_update"][:t] == 2).all()
    for key in STATE_KEYS:
        assert np.array_equal(a[key], b[key]), key


# ---- form 6: a bank has no import, so the state is built by frames and taken from a host tracker fed the same
def bank_frames():
    """Four frames that raise fifteen confirmed tracks (every height at every centre, a = 0.5): the boxes drift by 0.4 % a frame."""
    boxes = np.array([(c - 0.25 * h, 0.75 * c + 5 - 0.5 * h, 0.5 * h, h) for h in K.HEIGHTS for c in K.CENTRES])
    feats = np.stack([K.feature(k) for k in range(len(boxes))])
    out = []
    for f in range(4):
        b = boxes.copy()
        b[:, :2] += 0.004 * f * b[:, 2:]
        out.append((b.astype(np.float32), np.full(len(b), 0.9, np.float32), np.zeros(len(b), np.int32), feats, np.ones(len(b), np.uint8)))
    return out


def test_bank_stream_planted_frame(gpu, lib):
    TC, Bank = pkg("core.tracker_core").TrackerCore, pkg("deepsort_bank").DeepSORTBank
    bank = Bank(2, nn_budget=BUDGET, feature_dim=K.DIM)
    bank.option("epoch_frames", 1)
    host = TC(nn_budget=BUDGET)
    build = bank_frames()
    other = [(f[0][:2] + np.float32(77), f[1][:2], f[2][:2], f[3][:2], f[4][:2]) for f in build[:2]]    # stream 0: two tracks, two frames
    bank.update_arrays([other, build])
    for fr in build:
        host.predict()
        host.update_arrays(*fr)
    before, b = host.export_arrays(), bank.export(1)
    for key in STATE_KEYS:
        assert np.array_equal(before[key], b[key]), key              # the planted state: the bank holds the host tracker's, bit for bit
    assert (before["state"] == 2).all() and (before["time_since_update"] == 0).all() and len(before["state"]) == 15
    p = K.plan_states(before["mean"], before["cov"], decoy_every=0, seed=6)
    fr = frame_of(p)
    res = bank.update_arrays([[other[0]], [fr]])
    host.predict()
    host.update_arrays(*fr)
    after, matches = bank.export(1), host.last_matches()
    for key in STATE_KEYS:
        assert np.array_equal(host.export_arrays()[key], after[key]), key
    assert np.array_equal(res[1][0][0], host.outputs()[0])
    # the frame's checks on the bank's own export (matches: the host tracker's, whose state the bank just equalled)
    ts = sorted(p.pair)
    assert sorted(matches) == sorted((t + 1, p.pair[t]) for t in ts)
    got = {t: (after["mean"][t], after["cov"][t]) for t in ts}
    c, m, c2, m2 = step_figures(p, got)
    oc, om, oc2, om2 = step_figures(p, oracle_step(p))
    print(f"bank stream 1: covariance {c:.2e} of {K.allow(oc):.2e}, mean {m:.2e} of {K.allow(om):.2e} in one piece; covariance {c2:.2e} of "
          f"{K.allow(oc2):.2e}, mean {m2:.2e} of {K.allow(om2):.2e} from the fp32 predicted state")
    # measured on MI355X: 1.5e-7 of 4.8e-7, 9.8e-2 of 3.9e-1; 1.5e-7 of 4.8e-7, 1.0e-7 of 4.8e-7
    assert c <= K.allow(oc) and m <= K.allow(om) and c2 <= K.allow(oc2) and m2 <= K.allow(om2)
    exp = expected_rows(p)
    assert_rows_equal_or_on_rounding_edge(res[1][0][0][:, :4], np.rint(exp), exp, "bank")
    z = K.xyah32(p.det)
    for q, j in enumerate(p.new):
        im, ic = O.kf_initiate(z[j])
        assert np.array_equal(after["mean"][15 + q], im) and np.array_equal(after["cov"][15 + q], ic), q
    kf = GpuKF(lib)
    pm, pp = kf.predict(p.mean, p.cov)
    um, uc = kf.update(pm, pp, z[[p.pair[t] for t in ts]])
    assert np.array_equal(um, after["mean"][:15]) and np.array_equal(uc, after["cov"][:15])


# ------------------------------------------------------------------------------------------------------------------ (c) ByteTrack
def test_bytetrack_every_frame_against_fp64(gpu):
    """ByteTrack's epoch kernel (kf_*_wave on every track), twelve frames one launch each, the state exported after every frame and every
    frame's step checked from the previous frame's exported fp32 state: initiate, predict + update, predict alone with mean[7] zeroed
    first for the lost track, and the update that re-activates it.  Every object grows by 1 % of its height a frame and its aspect by
    0.002 (kf_ref.bt_boxes), so the height velocity that the lost track loses is not 0: asserted below on the exported state, and on the
    float64 filter in tests/test_kf_ref.py."""
    bt = pkg("bytetrack").BYTETracker()
    bt.option("epoch_frames", 1)
    fig, _ = oracle_figures()
    prev, tid_of, worst, zeroed = None, {}, dict(update=[0.0, 0.0, 0.0, 0.0], predict=[0.0, 0.0]), 0
    allow_u = [0.0, 0.0, 0.0, 0.0]
    for f in range(1, 13):
        xyxy, who = K.bt_boxes(f)
        bt.update(xyxy, np.full(len(xyxy), 0.9, np.float32), np.zeros(len(xyxy), np.int32))
        tlwh = np.stack([xyxy[:, 0], xyxy[:, 1], xyxy[:, 2] - xyxy[:, 0], xyxy[:, 3] - xyxy[:, 1]], 1)          # fp32, as the tracker's entry does
        z = K.xyah32(tlwh)
        e = bt.export()
        assert len(e["track_id"]) == len(K.BT_OBJECTS), f
        row = {int(t): k for k, t in enumerate(e["track_id"])}
        if f == 1:
            for j, k in enumerate(who):                              # by position: the track that sits on object k's detection
                hit = [t for t, r in row.items() if np.array_equal(e["mean"][r][:4], z[j])]
                assert len(hit) == 1, (k, hit)
                tid_of[k] = hit[0]
                im, ic = O.kf_initiate(z[j])
                assert np.array_equal(e["mean"][row[hit[0]]], im) and np.array_equal(e["cov"][row[hit[0]]], ic), k
        else:
            for k in range(len(K.BT_OBJECTS)):
                r, q = row[tid_of[k]], prev[1][tid_of[k]]
                m0, p0 = prev[0]["mean"][q].copy(), prev[0]["cov"][q]
                if prev[0]["state"][q] != 1:                         # STrack.multi_predict: a track that is not Tracked loses its height velocity
                    if f == K.BT_GONE[0] + 1:                        # ... and it has one (0 from then on): a kernel that left it alone would predict another state
                        assert abs(m0[7]) > 1e-3 * m0[3], (f, m0[7])
                        assert not np.array_equal(O.kf_predict(m0, p0)[0], O.kf_predict(np.append(m0[:7], np.float32(0)), p0)[0]), f
                    m0[7] = 0
                    zeroed += 1
                pm, pp = O.kf_predict(m0, p0)
                if k in who:
                    assert e["state"][r] == 1 and e["end_frame"][r] == f, (f, k)
                    zz = z[who.index(k)]
                    got = (e["mean"][r], e["cov"][r])
                    om, oc = O.kf_update(pm, pp, zz)
                    for i, (a, b) in enumerate(zip(K.step_errs(*got, m0, p0, zz) + K.update_errs(*got, pm, pp, zz),
                                                   K.step_errs(om, oc, m0, p0, zz) + K.update_errs(om, oc, pm, pp, zz))):
                        worst["update"][i], allow_u[i] = max(worst["update"][i], a), max(allow_u[i], b)
                else:
                    assert k == K.BT_ABSENT and f in K.BT_GONE and e["state"][r] == 2 and e["end_frame"][r] == 4, (f, k)
                    assert np.array_equal(e["mean"][r], pm) and np.array_equal(e["cov"][r], pp), (f, k)     # predict: the restatement's bits
                    c, m = K.predict_errs(e["mean"][r], e["cov"][r], m0, p0)
                    worst["predict"] = [max(worst["predict"][0], c), max(worst["predict"][1], m)]
        prev = (e, row)
    lost = prev[0]["start_frame"][prev[1][tid_of[K.BT_ABSENT]]]
    assert lost == 1 and zeroed == 4                                 # the same track all along: lost in 5 (zeroed before the predicts of 6 .. 9), re-activated in 9
    print("bytetrack update: " + ", ".join(f"{a:.2e} of {K.allow(b):.2e}" for a, b in zip(worst["update"], allow_u))
          + f" (covariance, mean in one piece; covariance, mean from the fp32 predicted state); predict alone {worst['predict'][0]:.2e}, "
          f"{worst['predict'][1]:.2e} of {K.allow(fig['predict dt 1'][0]):.2e}, {K.allow(fig['predict dt 1'][1]):.2e}")
    # measured on MI355X: update 2.7e-7 of 1.0e-6, 1.4e-1 of 5.7e-1 in one piece; 2.6e-7 of 9.8e-7, 1.3e-7 of 7.5e-7 from the fp32 predicted state;
    # predict alone 9.8e-8, 2.6e-8 of 4.8e-7 (and the restatement's bits, asserted above)
    for a, b in zip(worst["update"], allow_u):
        assert a <= K.allow(b)
    assert worst["predict"][0] <= K.allow(fig["predict dt 1"][0]) and worst["predict"][1] <= K.allow(fig["predict dt 1"][1])
