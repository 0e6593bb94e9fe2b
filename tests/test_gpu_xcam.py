"""Cross-camera identities inside a tracker bank on the device (aic_xcam_*, csrc/kernels_xcam.hip).

The nearest kernel is held bit for bit to oracle/xcam_oracle.py::nearest_rows and to the kernel it restates (gallery_nearest_kernel through
aic_gallery_annotate); the pack kernels to the banks' own exports; the identities to the policy restatement of tests/test_xcam_host.py
applied to the oracle's tables.  Every comparison is np.array_equal except the one DeepSORT embedding check whose tolerance is derived
in its docstring."""
import ctypes as C

import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

from conftest import ROOT, pkg
from oracle import xcam_oracle as X
from test_xcam_host import PolicyRef

pytestmark = pytest.mark.gpu

TILES = (32, 64)            # rows and columns of a tile of xcam_nearest_kernel: 16 * R, R = 2 (XCAM_SMALL_ROWS) or 4; option "tile" forces one
K_CHUNK = 32                # XCAM_KC: the K range goes through LDS in chunks of this many floats
THR = 0.2


# ---------------------------------------------------------------------------------------------------- 1. nearest rows
def _unit(rng, n, dim):
    e = rng.standard_normal((n, dim)).astype(np.float32)
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32)


def _shards(rng, S, t_max, dim, counts, junk=True):
    """fp32 [S, t_max, 2 + dim]: counts[s] valid rows first (random unit rows, ids unique per stream); behind them invalid rows that
    hold junk embeddings, which nothing may read into a result."""
    g = np.zeros((S, t_max, 2 + dim), np.float32)
    for s in range(S):
        c = counts[s]
        g[s, :c, 0] = 1.0
        g[s, :c, 1] = rng.permutation(200)[:c] + 1
        g[s, :c, 2:] = _unit(rng, c, dim)
        if junk:
            g[s, c:, 1] = 77.0
            g[s, c:, 2:] = _unit(rng, t_max - c, dim) * 3.0
    return g


def _dot_above_one(rng, dim):
    """A unit row whose k-ascending fp32 self-product exceeds 1: the distance to a copy of itself clamps to +0."""
    for _ in range(2000):
        v = _unit(rng, 1, dim)[0]
        if np.cumsum((v * v).astype(np.float32), dtype=np.float32)[-1] > np.float32(1.0):
            return v
    raise AssertionError("no such row found")


def _cases():
    rng = np.random.default_rng(7)
    out = {}
    out["one-stream"] = _shards(rng, 1, 33, 32, [33])                              # S = 1: all -1
    for T in TILES:                                                                # t_max and counts one below, at, one above the tile
        for t_max in (T - 1, T, T + 1):
            out[f"edge-{t_max}"] = _shards(rng, 2, t_max, 4 if T == 32 else K_CHUNK + 4, [t_max, t_max - 1])
    out["empty-stream-512"] = _shards(rng, 3, 33, 512, [33, 0, 31])               # a stream with no valid row; 16 K-chunks
    out["mixed-counts"] = _shards(rng, 3, 65, K_CHUNK, [64, 65, 1])               # dim = one K-chunk; a tile pair inside one stream
    out["all-empty"] = _shards(rng, 3, 8, 32, [0, 0, 0])
    c33 = rng.integers(0, 17, 33)
    c33[[0, 5, 32]] = [16, 0, 0]
    out["33-streams-512"] = _shards(rng, 33, 16, 512, c33.tolist())              # more streams than a tile has rows; n = 528
    # exact ties: one embedding in cameras 1 and 2 (and twice in camera 2): camera 0's copy must pick the lowest row
    g = _shards(rng, 3, 12, 36, [5, 6, 7])
    g[0, 2, 2:] = g[1, 4, 2:] = g[2, 1, 2:] = g[2, 5, 2:] = _unit(rng, 1, 36)[0]
    out["ties"] = g
    # identical rows whose product rounds above 1 (distance clamps to +0) and antipodal rows (distance 2)
    g = _shards(rng, 3, 6, 64, [3, 3, 2])
    v = _dot_above_one(rng, 64)
    g[0, 0, 2:] = g[1, 1, 2:] = v
    g[2, 0, 2:] = -g[0, 1, 2:]
    g[2, 1, 2:] = -g[1, 0, 2:]
    out["clamp-antipodal"] = g
    return out


_CASES, _WANT = {}, {}


def _case(name):
    if not _CASES:
        _CASES.update(_cases())
    if name not in _WANT:
        _WANT[name] = X.nearest_rows(_CASES[name])                                # once per case, shared and left unchanged
    return _CASES[name], _WANT[name]


CASE_NAMES = ["one-stream", "edge-31", "edge-32", "edge-33", "edge-63", "edge-64", "edge-65", "empty-stream-512", "mixed-counts", "all-empty",
              "33-streams-512", "ties", "clamp-antipodal"]


def _annotate(g_dev, S, t_max, dim):
    L = pkg("_lib")
    n = S * t_max
    ids, nr, nd = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    L.call("aic_gallery_annotate", 0, None, C.c_void_p(g_dev.data_ptr()), S, 0, t_max, dim, THR, L.ptr(ids), L.ptr(nr), L.ptr(nd), None)
    return ids, nr, nd


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_nearest_rows_equal_the_oracle_and_the_rank_kernel(gpu, name, tile):
    g, want = _case(name)
    S, t_max, w = g.shape
    xc = pkg("xcam").CrossCamera(S, t_max, w - 2, THR)
    xc.option("tile", tile)
    xc.link_shards(g)                                                             # host memory, n_valid counted from the valid column
    got = xc.tables()
    for a, b, what in zip(got, want, ("track_id", "near_row", "near_dist")):
        assert np.array_equal(a, b), (name, tile, what, np.nonzero(a != b)[0][:8])
    assert np.array_equal(xc.shards(), g)
    ids, nr, nd = got
    mutual = (nr >= 0) & (nr[np.maximum(nr, 0)] == np.arange(len(nr)))
    assert np.array_equal(nd[mutual].view(np.uint32), nd[nr[mutual]].view(np.uint32))   # bit symmetry
    valid = g.reshape(-1, w)[:, 0] > 0.5
    assert (nr[~valid] == -1).all() and (ids[~valid] == -1).all() and (nd[~valid] == np.float32(1e5)).all()
    if S == 1 or name == "all-empty":
        assert (nr == -1).all()
    # device memory, with and without the caller's n_valid; the same shards through the rank path's kernel
    gd = torch.from_numpy(g).cuda()
    xd = pkg("xcam").CrossCamera(S, t_max, w - 2, THR)
    xd.option("tile", tile)
    xd.link_shards(gd, n_valid=(g[:, :, 0] > 0.5).sum(1))
    for a, b in zip(xd.tables(), got):
        assert np.array_equal(a, b)
    xd.link_shards(gd)
    for a, b in zip(xd.tables(), got):
        assert np.array_equal(a, b)
    for a, b in zip(_annotate(gd, S, t_max, w - 2), got):
        assert np.array_equal(a, b)
    xc.close(), xd.close()


def test_ties_clamp_and_antipodes_are_what_the_cases_say(gpu):
    """The special rows of the cases above do meet the situations they are named after (on the oracle's tables, which the kernel equals)."""
    g, (ids, nr, nd) = _case("ties")
    assert nr[0 * 12 + 2] == 1 * 12 + 4                                           # the lowest of rows 16, 25, 29
    assert nr[2 * 12 + 1] == 0 * 12 + 2 and nr[1 * 12 + 4] == 0 * 12 + 2
    assert nd[2] == nd[16] == nd[25] == nd[29]
    g, (ids, nr, nd) = _case("clamp-antipodal")
    assert nr[0] == 7 and nr[7] == 0 and nd[0] == 0.0 and not np.signbit(nd[0])   # 1 - dot < 0 clamps to +0
    d = np.maximum(np.float32(1.0) - np.cumsum((g[0, 1, 2:] * g[2, 0, 2:]).astype(np.float32), dtype=np.float32)[-1], 0)
    assert d > 1.99                                                               # the antipode is nobody's nearest row
    assert nr[1] != 12 and nr[12] != 1


def test_link_shards_rejections(gpu):
    L = pkg("_lib")
    rng = np.random.default_rng(3)
    g = _shards(rng, 2, 8, 16, [4, 3])
    bad = g.copy()
    bad[1, 5, 0] = 1.0                                                            # a valid row behind an invalid one
    xc = pkg("xcam").CrossCamera(2, 8, 16, THR)
    for arg in (bad, torch.from_numpy(bad).cuda()):                               # host: before the device; device: after the count
        with pytest.raises(L.AicError) as ei:
            xc.link_shards(arg)
        assert ei.value.code == L.ERR_INVALID and "stream 1" in str(ei.value) and "prefix" in str(ei.value)
        with pytest.raises(L.AicError):
            xc.tables()                                                           # no pass has completed
    with pytest.raises(L.AicError) as ei:
        xc.link_shards(g, n_valid=[4, 9])
    assert ei.value.code == L.ERR_INVALID
    with pytest.raises(L.AicError) as ei:
        xc.link_shards(g, n_valid=[4, 2])                                         # differs from the valid column
    assert ei.value.code == L.ERR_INVALID
    gd = torch.from_numpy(g).cuda()
    for nv in ([4, 2], [4, 5]):                                                   # device memory: held against the device's count, nothing is linked
        with pytest.raises(L.AicError) as ei:
            xc.link_shards(gd, n_valid=nv)
        assert ei.value.code == L.ERR_INVALID and "stream 1" in str(ei.value) and xc.size()["tracks"] == 0
    assert xc.link_shards(gd, n_valid=[4, 3]) == 0 and xc.link_shards(g) == 0 and xc.size()["tracks"] == 7
    with pytest.raises(ValueError):
        xc.link_shards(g[:, :4])
    xc.close()


# ---------------------------------------------------------------------------------------------------- persons for the banks
DIM = 32
BOX = lambda p: np.array([60.0 + 170.0 * p, 100.0, 50.0, 120.0], np.float32)     # noqa: E731 -- tlwh, far apart


def person_feature(p, cam, tick, scale=1.7):
    """Hand-made: person p's unit direction, a little camera- and tick-dependent noise, scaled off unit length (the device normalises)."""
    base = np.random.default_rng(1000 + p).standard_normal(DIM)
    base /= np.linalg.norm(base)
    noise = np.random.default_rng(5000 + 97 * p + 13 * cam + tick).standard_normal(DIM) * 0.02
    v = base + noise
    return (v / np.linalg.norm(v) * scale).astype(np.float32)


def deepsort_tick(persons, cam, tick):
    n = len(persons)
    tlwh = np.stack([BOX(p) for p in persons]).reshape(n, 4) if n else np.zeros((0, 4), np.float32)
    feats = np.stack([person_feature(p, cam, tick) for p in persons]) if n else np.zeros((0, DIM), np.float32)
    return (tlwh, np.full(n, 0.9, np.float32), np.zeros(n, np.int32), feats, np.ones(n, np.uint8))


def botsort_tick(persons, cam, tick, featless=()):
    n = len(persons)
    t = np.stack([BOX(p) for p in persons]).reshape(n, 4) if n else np.zeros((0, 4), np.float32)
    xyxy = np.concatenate([t[:, :2], t[:, :2] + t[:, 2:]], 1).astype(np.float32)
    feats = np.stack([person_feature(p, cam, tick) for p in persons]) if n else np.zeros((0, DIM), np.float32)
    valid = np.array([0 if p in featless else 1 for p in persons], np.int32)
    return (xyxy, np.full(n, 0.9, np.float32), np.zeros(n, np.int32), feats, None, valid)


def _unit64(rows):
    r = np.asarray(rows, np.float64)
    return r / np.linalg.norm(r, axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------------- 2. DeepSORT bank pack
def _expected_deepsort(bank, s, t_max):
    """(ids, raw newest gallery rows) of the stream's first t_max confirmed tracks with a gallery, in list order, from the bank's export."""
    e = bank.export(s)
    ids, rows = [], []
    for i, (tid, st, gl) in enumerate(zip(e["track_id"], e["state"], e["gallery_len"])):
        if st == 2 and gl > 0 and len(ids) < t_max:
            ids.append(int(tid))
            rows.append(bank.export_gallery(s, i, int(gl))[-1])
    return ids, np.array(rows, np.float32).reshape(len(ids), DIM)


def _check_pack(shard, s, ids, n_valid):
    assert n_valid == len(ids)
    assert shard[s, :n_valid, 0].tolist() == [1.0] * n_valid and (shard[s, n_valid:, :2] == 0).all()
    assert shard[s, :n_valid, 1].tolist() == [float(i) for i in ids]


def test_deepsort_bank_pack(gpu):
    """S = 3, max_tracks 16, dim 32, n_init 3, nn_budget 2; the cameras hold {4, 1, 0} persons, camera 1's one person being one of camera
    0's (with one person on camera 1 the cameras cannot share two; the identity test below shares two).  Flags, ids, order and n_valid
    are exact.  The embedding row is the device's fp32 normalisation (launch_normalize_rows) of the newest raw gallery row, compared
    with that raw row normalised in fp64.  Tolerance: NumPy's own fp32 normalisation of the same rows differs from fp64 by at most
    2.79e-8 here (measured again by this test); the device sums the squares in another order (one lane per element, then a butterfly:
    restated in NumPy it differs from fp64 by 2.69e-8 on these rows), so 4 x the NumPy figure = 1.11e-7 is allowed."""
    cams = [[0, 1, 2, 3], [2], []]
    bank = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=16, feature_dim=DIM, n_init=3, nn_budget=2)
    xc = pkg("xcam").CrossCamera(3, 16, DIM, THR)
    for tick in range(4):
        bank.update_arrays([[deepsort_tick(p, c, tick)] for c, p in enumerate(cams)])
        if tick == 1:                                                             # hits = 2 < n_init: every track is tentative
            assert bank.link_cameras(xc) == 0
            assert not xc.shards()[:, :, 0].any() and (xc.tables()[0] == -1).all()
    assert bank.link_cameras() == 1 and bank.xcam is xc
    shard = xc.shards()
    n_valid = (shard[:, :, 0] > 0.5).sum(1).tolist()
    assert n_valid == [4, 1, 0]
    worst_np, worst = 0.0, 0.0
    for s in range(3):
        ids, raw = _expected_deepsort(bank, s, 16)
        _check_pack(shard, s, ids, n_valid[s])
        if not ids:
            continue
        assert len(set(bank.export(s)["gallery_len"].tolist())) == 1 and bank.export(s)["gallery_len"][0] == 2   # the ring has wrapped
        newest = np.stack([person_feature(p, s, 3) for p in cams[s]])
        assert np.array_equal(raw, newest)                                        # the newest entry, not the oldest in the ring
        ref = _unit64(raw)
        np32 = raw / np.sqrt((raw * raw).sum(1, dtype=np.float32, keepdims=True))
        worst_np = max(worst_np, float(np.abs(np32.astype(np.float64) - ref).max()))
        worst = max(worst, float(np.abs(shard[s, :len(ids), 2:].astype(np.float64) - ref).max()))
    assert 0 < worst_np <= 2.8e-8, worst_np
    assert worst <= 4 * worst_np, (worst, worst_np)
    # t_max = 2 < 4 confirmed tracks: the first two in list order
    x2 = pkg("xcam").CrossCamera(3, 2, DIM, THR)
    x2.link_bank(bank)
    s2 = x2.shards()
    assert (s2[:, :, 0] > 0.5).sum(1).tolist() == [2, 1, 0]
    assert s2[0, :, 1].tolist() == shard[0, :2, 1].tolist() and np.array_equal(s2[0, :, 2:], shard[0, :2, 2:])
    # a bank of another shape is rejected before the device is touched
    L = pkg("_lib")
    for other in (pkg("deepsort_bank").DeepSORTBank(2, max_tracks=16, feature_dim=DIM), pkg("deepsort_bank").DeepSORTBank(3, max_tracks=16, feature_dim=64)):
        with pytest.raises(L.AicError) as ei:
            xc.link_bank(other)
        assert ei.value.code == L.ERR_INVALID
        other.close()
    for o in (xc, x2, bank):
        o.close()


# ---------------------------------------------------------------------------------------------------- 3. BoT-SORT bank pack
def test_botsort_bank_pack(gpu):
    """The same against BoTSORTBank.export: rows = the tracked list's activated tracks with a feature, in its order; the row is the slot's
    smoothed unit feature itself, so the embeddings are np.array_equal.  Camera 0 holds persons 0..3, person 1 never with a feature
    (tracked, absent), person 3 gone after tick 1 (lost, absent) and person 4 born at the last tick (not activated yet, absent)."""
    bank = pkg("botsort").BoTSORTBank(3, max_tracks=16, feature_dim=DIM)
    for tick in range(4):
        cam0 = [0, 1, 2, 3] if tick < 2 else [0, 1, 2] + ([4] if tick == 3 else [])
        bank.update_arrays([[botsort_tick(cam0, 0, tick, featless=(1,))], [botsort_tick([2], 1, tick)], [botsort_tick([], 2, tick)]])
    assert bank.link_cameras() == 1
    shard = bank.xcam.shards()
    n_valid = (shard[:, :, 0] > 0.5).sum(1).tolist()
    seen = []
    for s in range(3):
        e = bank.export(s)
        nt = e["n_tracked"]
        keep = [i for i in range(nt) if e["is_activated"][i] and e["has_feat"][i]]
        _check_pack(shard, s, [int(e["track_id"][i]) for i in keep], n_valid[s])
        assert np.array_equal(shard[s, :len(keep), 2:], e["smooth_feat"][keep])
        seen.append((nt, len(e["track_id"]), len(keep)))
    assert seen == [(4, 5, 2), (1, 1, 1), (0, 0, 0)]                            # camera 0: 4 tracked (one featureless, one not activated) + 1 lost
    L = pkg("_lib")
    for other in (pkg("botsort").BoTSORTBank(2, max_tracks=16, feature_dim=DIM), pkg("botsort").BoTSORTBank(3, max_tracks=16, feature_dim=64)):
        with pytest.raises(L.AicError) as ei:                                     # a bank of another shape
            bank.xcam.link_bank(other)
        assert ei.value.code == L.ERR_INVALID
        other.close()
    x2 = pkg("xcam").CrossCamera(3, 1, DIM, THR)                                 # t_max 1 < 2 eligible tracks: the first in list order
    x2.link_bank(bank)
    assert np.array_equal(x2.shards()[0, 0], shard[0, 0]) and (x2.shards()[:, :, 0] > 0.5).sum(1).tolist() == [1, 1, 0]
    for o in (x2, bank.xcam, bank):
        o.close()


# ---------------------------------------------------------------------------------------------------- 4. identities end to end
A, B, Cc, D = 0, 1, 2, 3


def _feed(kind, bank, cams, ticks, t0=0):
    for tick in range(t0, t0 + ticks):
        if kind == "deepsort":
            bank.update_arrays([[deepsort_tick(p, c, tick)] if p is not None else [] for c, p in enumerate(cams)])
        else:
            bank.update_arrays([[botsort_tick(p, c, tick)] if p is not None else [] for c, p in enumerate(cams)])


def test_the_generated_features_link_exactly_the_shared_persons():
    """The oracle alone, on the CPU, on the unit features the banks below are fed: the links are {A0-A1, B0-B1} and nothing else."""
    g = np.zeros((3, 4, 2 + DIM), np.float32)
    for c, persons in enumerate([[A, B], [A, B], [Cc]]):
        for r, p in enumerate(persons):
            f = person_feature(p, c, 3)
            g[c, r] = np.concatenate([[1.0, 10 * c + r + 1], f / np.linalg.norm(f)])
    ids, nr, nd = X.nearest_rows(g)
    ref = PolicyRef(3)
    assert ref.update(4, ids, nr, nd, THR) == 2
    assert ref.lookup(1, 11) == ref.lookup(0, 1) and ref.lookup(1, 12) == ref.lookup(0, 2) and ref.lookup(2, 21) == (2 << 32) | 21
    assert nd[0] < 0.05 and nd[8] > 0.5                                           # well inside / well outside the threshold


@pytest.mark.parametrize("kind", ["deepsort", "botsort"])
def test_identities_end_to_end(gpu, kind):
    if kind == "deepsort":
        bank = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=8, feature_dim=DIM, n_init=3, nn_budget=4)
    else:
        bank = pkg("botsort").BoTSORTBank(3, max_tracks=8, feature_dim=DIM)
    _feed(kind, bank, [[A, B], [A, B], [Cc]], 4)
    ref = PolicyRef(3)

    def link_and_check(want_links):
        assert bank.link_cameras() == want_links
        xc = bank.xcam
        shard = xc.shards()
        ids, nr, nd = X.nearest_rows(shard)                                       # the oracle on the read-back shard
        for a, b in zip(xc.tables(), (ids, nr, nd)):
            assert np.array_equal(a, b)
        assert ref.update(xc.t_max, ids, nr, nd, xc.max_cosine_distance) == want_links
        for s in range(3):
            local = shard[s, shard[s, :, 0] > 0.5, 1].astype(np.int32)
            assert xc.global_ids(s, local).tolist() == [ref.lookup(s, int(i)) for i in local] and (bank.global_ids(s, local) >= 0).all()
        return shard

    shard = link_and_check(2)
    ids0, ids1, ids2 = (shard[s, shard[s, :, 0] > 0.5, 1].astype(np.int32) for s in range(3))
    assert len(ids0) == len(ids1) == 2 and len(ids2) == 1
    g0 = bank.global_ids(0, ids0)
    assert np.array_equal(g0, bank.global_ids(1, ids1))                           # A0-A1, B0-B1
    assert g0.tolist() == [(0 << 32) | int(i) for i in ids0]                      # the smaller id is the root: camera 0's
    assert bank.global_ids(2, ids2).tolist() == [(2 << 32) | int(ids2[0])]        # C keeps its own id
    assert bank.global_ids(2, [99]).tolist() == [-1]
    assert bank.xcam.size() == dict(tracks=5, identities=3, links=2)
    link_and_check(0)                                                             # a second call adds no link
    # camera 1 reconnects and sees C and D: its recycled local ids are other people now
    bank.reset(1)
    ref.forget(1)
    assert bank.global_ids(1, ids1).tolist() == [-1, -1]
    _feed(kind, bank, [None, [Cc, D], None], 4, t0=4)
    shard = link_and_check(1)                                                     # C1-C2
    new1 = shard[1, shard[1, :, 0] > 0.5, 1].astype(np.int32)
    assert new1.tolist() == ids1.tolist()                                         # the same local ids again
    g1 = bank.global_ids(1, new1)
    assert g1[0] == (2 << 32) | int(ids2[0])                                      # C: camera 2's identity
    assert g1[1] == (1 << 44) | (1 << 32) | int(new1[1])                          # D: its own key, generation 1
    assert np.array_equal(bank.global_ids(0, ids0), g0)                           # camera 0's ids are unchanged
    bank.xcam.close(), bank.close()


# ---------------------------------------------------------------------------------------------------- 5. a stopped stream
@pytest.mark.parametrize("kind", ["deepsort", "botsort"])
def test_a_stopped_stream_is_rejected_until_reset(gpu, kind):
    L = pkg("_lib")
    if kind == "deepsort":
        bank = pkg("deepsort_bank").DeepSORTBank(3, max_tracks=4, feature_dim=DIM, n_init=1, nn_budget=4)
    else:
        bank = pkg("botsort").BoTSORTBank(3, max_tracks=4, feature_dim=DIM)
    _feed(kind, bank, [[A, B], [0, 1, 2, 3, 4, 5], [A]], 2)                        # camera 1 exhausts its 4 slots
    assert list(bank.failed) == [1]
    with pytest.raises(L.AicError) as ei:
        bank.link_cameras()
    assert ei.value.code == L.ERR_INVALID and "stream 1" in str(ei.value)
    assert bank.xcam.size()["tracks"] == 0                                        # nothing was linked
    bank.reset(1)
    _feed(kind, bank, [[A, B], [B], [A]], 2, t0=2)
    assert bank.link_cameras() == 2                                               # A0-A2, B0-B1
    bank.xcam.close(), bank.close()


@pytest.mark.parametrize("kind", ["deepsort", "botsort"])
def test_a_track_id_that_fp32_cannot_carry_fails_the_link(gpu, kind):
    """Ids travel as fp32 in the shard: 2^24 - 1 is the last one that does, exactly; a bank holding 2^24 fails with AIC_ERR_CAPACITY."""
    L = pkg("_lib")

    def bank_from(first):
        if kind == "deepsort":
            return pkg("deepsort_bank").DeepSORTBank(2, max_tracks=4, feature_dim=DIM, n_init=1, nn_budget=4, first_track_id=first)
        return pkg("botsort").BoTSORTBank(2, max_tracks=4, feature_dim=DIM, first_track_id=first)

    ok = bank_from((1 << 24) - 1)
    _feed(kind, ok, [[A], [A]], 2)
    assert ok.link_cameras() == 1
    assert ok.xcam.tables()[0][[0, 4]].tolist() == [(1 << 24) - 1] * 2 and ok.global_ids(1, [(1 << 24) - 1]).tolist() == [(1 << 24) - 1]
    big = bank_from((1 << 24) - 1)
    _feed(kind, big, [[A], [A, B]], 2)                                            # camera 1's second track takes id 2^24
    with pytest.raises(L.AicError) as ei:
        big.link_cameras()
    assert ei.value.code == L.ERR_CAPACITY and "stream 1" in str(ei.value) and "2^24" in str(ei.value)
    assert big.xcam.size()["tracks"] == 0                                         # nothing was linked
    for b in (ok, big):
        b.xcam.close(), b.close()


# ---------------------------------------------------------------------------------------------------- 6. the pipeline
def test_pipeline_links_the_cameras_of_a_botsort_bank(gpu):
    L = pkg("_lib")
    syn = pkg("synthetic")
    TP = pkg("pipeline").TrackingPipeline
    ypath, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    sc = syn.Scene(seed=5, n_targets=5)
    frames = sc.render_batch(0, 4)
    ticks = np.ascontiguousarray(np.repeat(frames, 2, axis=0))                    # both cameras are fed the same source, tick-major
    planted = [sc.detections(f // 2)[:3] for f in range(8)]

    def run(link):
        pipe = TP.botsort_bank(ypath, rpath, (720, 1280), cameras=2, batch=4, ring_frames=8, max_persons=16, dtype="fp16", inject=True)
        pipe.option("taper", 0)
        pipe.upload(0, ticks)
        pipe.inject(0, planted)
        rows, links = [], []
        for slot in (0, 4):                                                       # two run calls of two ticks
            rows += pipe.run(slot, 4)[0]
            if link:
                links.append(pipe.link_cameras())
        return pipe, rows, links

    plain, want, _ = run(False)
    pipe, got, links = run(True)
    assert got == want and sum(len(r) for r in got) > 8                           # the tracker's rows do not see the links
    shard = pipe.xcam.shards()
    nv = (shard[:, :, 0] > 0.5).sum(1)
    assert nv[0] == nv[1] > 0 and shard[0, :nv[0], 1].tolist() == shard[1, :nv[1], 1].tolist()
    assert sum(links) == nv[0]                                                    # every activated track, pairwise
    local = shard[0, :nv[0], 1].astype(np.int32)
    assert np.array_equal(pipe.global_ids(0, local), pipe.global_ids(1, local)) and pipe.global_ids(0, local).tolist() == local.tolist()
    assert pipe.link_cameras() == 0
    pipe.reset_stream(1)
    assert (pipe.global_ids(1, local) == -1).all() and np.array_equal(pipe.global_ids(0, local), local)
    # any other pipeline: rejected by the class and by the library
    bt = TP(ypath, None, (720, 1280), batch=4, ring_frames=4, max_persons=16, dtype="fp16", inject=True, tracker="bytetrack")
    with pytest.raises(ValueError):
        bt.link_cameras()
    n = C.c_int32()
    assert L.load().aic_pipeline_link_cameras(bt._h, pipe.xcam._h, C.byref(n)) == L.ERR_INVALID
    with pytest.raises(SystemExit):
        pkg("cli").main(["--link_cameras", "--input", "synthetic:1280x720:4:4:1", "--tracker", "botsort"])
    for p in (bt, plain, pipe):
        p.close()


def test_cli_link_cameras_writes_global_ids_parallel_to_the_tracks(gpu, tmp_path):
    """--inputs a,b --tracker botsort --link_cameras: two cameras on the same synthetic source; every JSON line carries "global_ids" as
    long as "tracks", a linked track of camera 1 carries camera 0's id, and the annotated frames are written (the overlay label path)."""
    import json
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    _, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    src = "synthetic:1280x720:5:8:1"
    rc = pkg("cli").main(["--inputs", f"{src},{src}", "--output_dir", str(tmp_path), "--yolo_engine", ypath, "--reid_engine", rpath,
                          "--tracker", "botsort", "--batch", "8", "--link_cameras"])
    assert rc == 0
    lines = []
    for k in range(2):
        (path,) = tmp_path.glob(f"*_s{k}.jsonl")
        lines.append([json.loads(l) for l in path.read_text().splitlines()])
        assert len(lines[k]) == 8 and len(list(tmp_path.glob(f"*_s{k}.*"))) >= 2  # the JSON lines and the annotated frames
        for fr in lines[k]:
            assert len(fr["global_ids"]) == len(fr["tracks"]) and all(isinstance(g, int) for g in fr["global_ids"])
    last0, last1 = lines[0][-1], lines[1][-1]
    assert last0["tracks"] == last1["tracks"] and len(last0["tracks"]) > 0        # the same source: the same rows on both cameras
    linked = [g for g in last1["global_ids"] if g >= 0]
    assert linked and last0["global_ids"] == last1["global_ids"]                  # camera 1 adopted camera 0's ids
    assert all(g == t[4] for g, t in zip(last0["global_ids"], last0["tracks"]) if g >= 0)   # camera 0: generation 0, stream 0 -> the local id
