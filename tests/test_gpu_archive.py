"""The identity archive on the device (aic_archive_*, csrc/kernels_archive.hip) against tests/archive_oracle.py.
Every comparison is np.array_equal: the int8 codes, the scales, and the keys, slots and distance bits of every search."""
import numpy as np
import pytest
import torch            # noqa: F401 -- before libaicam.so is loaded, as in the other GPU suites: one HIP runtime

import archive_oracle as A
from conftest import ROOT, pkg
from test_archive_host import KeyPolicyRef
from test_gpu_xcam import DIM as BANK_DIM, deepsort_tick

pytestmark = pytest.mark.gpu

THR = 0.2


def _arc(cap, dim):
    return pkg("archive").IdentityArchive(cap, dim), A.ArchiveRef(cap, dim)


def _rows(rng, n, dim):
    """Random directions at lengths 0.6..1.1 (the scales differ; a similarity rarely passes 1), nothing symmetric about them."""
    v = rng.standard_normal((n, dim))
    return (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.6, 1.1, (n, 1))).astype(np.float32)


def _put(arc, ref, keys, cams, tick, rows):
    arc.put(keys, cams, tick, rows)
    ref.put(keys, np.broadcast_to(np.asarray(cams), (len(keys),)), tick, rows)


def _same_contents(arc, ref):
    e = arc.export()
    n, dim = ref.hw, ref.dim
    assert len(e["keys"]) == n and arc.size() == ref.size()
    assert np.array_equal(e["keys"], np.asarray(ref.key, np.int64))
    occ = e["keys"] >= 0
    for name, want in (("cameras", ref.cam), ("t_first", ref.t_first), ("t_last", ref.t_last)):
        assert np.array_equal(e[name][occ], np.asarray(want)[occ]), name
    assert np.array_equal(e["scales"][occ].view(np.uint32), ref.scale[:n][occ].view(np.uint32))
    assert np.array_equal(e["rows"][occ][:, :dim], ref.q[:n][occ])
    assert not e["rows"][occ][:, dim:].any()                              # the padding up to the pitch is zero
    return e


def _same_search(arc, ref, queries, k, **flt):
    names = dict(since="t_lo", until="t_hi")
    got = arc.search(queries, k=k, **flt)
    want = ref.search(queries, k=k, **{names.get(a, a): v for a, v in flt.items()})
    for g, w, what in zip(got, want, ("keys", "slots", "dist")):
        assert g.shape == w.shape == (len(queries), k)
        if what == "dist":
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), (what, k, flt, np.argwhere(g != w)[:4].tolist())
    return got


# ---------------------------------------------------------------------------------------------------- 1. quantisation
@pytest.mark.parametrize("dim", [4, 36, 64, 512, 1024])
@pytest.mark.parametrize("n", [1, 17])
def test_put_codes_and_scales_equal_the_oracle(gpu, n, dim):
    rng = np.random.default_rng(1000 * n + dim)
    arc, ref = _arc(40, dim)
    rows = _rows(rng, n, dim)
    rows[0, dim // 2] = -1.5 * np.abs(rows[0]).max()                      # the maximum sits on a negative element
    _put(arc, ref, np.arange(n) + 100, np.arange(n) % 3, 4, rows)
    # m = 127 makes 127 / m = 1: the products are the elements, and these land exactly on x.5 (half to even, both signs)
    half = np.resize(np.array([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 63.5, -126.5, 126.5, 3.0, -4.0], np.float32), dim)
    _put(arc, ref, [7], [1], 5, half[None])
    e = _same_contents(arc, ref)
    s = ref.find(7)
    assert e["scales"][s] == 1.0 and e["rows"][s, :dim].tolist() == np.resize(np.array([127, 0, 2, 2, 0, -2, -2, 64, -126, 126, 3, -4]), dim).tolist()
    assert e["rows"][ref.find(100), dim // 2] == -127
    # a zero row, a NaN row and an infinite row: the call fails, the good rows beside them are not stored either, no slot changes
    L = pkg("_lib")
    for bad in (np.zeros(dim, np.float32), np.where(np.arange(dim) == dim - 1, np.nan, 1.0).astype(np.float32),
                np.where(np.arange(dim) == 0, np.inf, 1.0).astype(np.float32)):
        with pytest.raises(L.AicError) as ei:
            arc.put([100, 555, 556], 0, 9, np.stack([_rows(rng, 1, dim)[0], bad, _rows(rng, 1, dim)[0]]))
        assert ei.value.code == L.ERR_INVALID
        with pytest.raises(ValueError):
            ref.put([100, 555, 556], [0, 0, 0], 9, np.stack([rows[0], bad, rows[0]]))
    after = arc.export()
    assert all(np.array_equal(e[k], after[k], equal_nan=k == "scales") for k in e)
    arc.close()


@pytest.mark.parametrize("dim", [4, 36, 512])
def test_put_from_a_torch_tensor_on_the_device(gpu, dim):
    rng = np.random.default_rng(dim)
    arc, ref = _arc(8, dim)
    rows = _rows(rng, 5, dim)
    arc.put(np.arange(5), 2, 0, torch.from_numpy(rows).cuda())
    ref.put(np.arange(5), [2] * 5, 0, rows)
    _same_contents(arc, ref)
    _same_search(arc, ref, torch.from_numpy(_rows(rng, 3, dim)).cuda().cpu().numpy(), 4)
    got = arc.search(torch.from_numpy(rows[:2]).cuda(), k=1)
    want = ref.search(rows[:2], k=1)
    assert all(np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
               for g, w in zip(got, want))
    arc.close()


# ---------------------------------------------------------------------------------------------------- 2. search
QS = (1, 15, 16, 17, 64, 65)


@pytest.mark.parametrize("mult,off", [(0, 1), (0, 15), (0, 16), (0, 17), (1, -1), (1, 0), (1, 1), (2, 1)])
def test_search_at_the_edges_of_groups_blocks_and_sweeps(gpu, mult, off):
    """N around a group of 16 slots and around R, a block's slot range; Q around a tile of 16 and a sweep of 64; k = 1, 8, 32 (more than
    the rows there are, for the small N).  Queries are not rows and Q != N: a transposed tile cannot pass."""
    dim = 64
    arc, ref = _arc(200, dim)
    R = arc.block_rows(1)
    assert R == 64 == arc.block_rows(65)
    N = mult * R + off
    rng = np.random.default_rng(N)
    _put(arc, ref, np.arange(N) + 1000, np.arange(N) % 5, 3, _rows(rng, N, dim))
    queries = _rows(rng, max(QS), dim)
    for Q in QS:
        for k in (1, 8, 32):
            keys, slots, dist = _same_search(arc, ref, queries[:Q], k)
            assert (slots[:, :min(k, N)] >= 0).all() and (slots[:, N:] == -1).all() and (dist[:, N:] == 1e5).all() and (keys[:, N:] == -1).all()
    arc.close()


@pytest.mark.parametrize("dim", [4, 36, 64, 512, 1024])
def test_search_at_every_dimension_class(gpu, dim):
    """dim 4 and 36 (one K-step, mostly padding), 64 (one exactly), 512 (8 steps) and 1024 (16 steps, the third kernel)."""
    rng = np.random.default_rng(dim)
    arc, ref = _arc(200, dim)
    _put(arc, ref, np.arange(131), np.arange(131) % 7, 0, _rows(rng, 131, dim))
    q = _rows(rng, 40, dim)
    q[:3] = ref_rows = _rows(np.random.default_rng(dim), 131, dim)[[5, 70, 130]]    # three of the stored rows themselves
    for Q, k in ((40, 8), (17, 32), (1, 1)):
        got = _same_search(arc, ref, q[:Q], k)
    got = _same_search(arc, ref, q[:3] * np.float32(0.37), 1)             # another length, the same direction
    if dim >= 64:                                                         # (in 4 dimensions another row may well lie closer)
        assert got[1][:, 0].tolist() == [5, 70, 130]
    arc.close()


def test_largest_dot_identical_and_antipodal_rows(gpu):
    """dim 1024, every element +-1/32: every code is +-127 and scale * scale * 1024 * 127^2 == 1, so |dot| is the largest there is
    (below 2^24), the row itself is at distance +0 and its negative at exactly 2."""
    dim = 1024
    rng = np.random.default_rng(3)
    arc, ref = _arc(64, dim)
    signs = np.where(rng.random((20, dim)) < 0.5, -1.0, 1.0).astype(np.float32) / 32
    signs[1] = 1.0 / 32
    signs[2] = -signs[1]
    signs[11] = -signs[10]
    _put(arc, ref, np.arange(20), 0, 0, signs)
    e = arc.export()
    assert (np.abs(e["rows"]) == 127).all()
    keys, slots, dist = _same_search(arc, ref, signs[[1, 10]], 20)
    assert slots[0, 0] == 1 and dist[0, 0] == 0 and not np.signbit(dist[0, 0]) and slots[0, -1] == 2 and dist[0, -1] == 2.0
    assert slots[1, 0] == 10 and dist[1, 0] == 0 and slots[1, -1] == 11 and dist[1, -1] == 2.0
    # a random unit row against itself: the codes' similarity is 1 up to the quantisation error, on either side; max(+0, .) clamps
    unit = rng.standard_normal((4, dim))
    unit = (unit / np.linalg.norm(unit, axis=1, keepdims=True)).astype(np.float32)
    _put(arc, ref, np.arange(4) + 50, 0, 0, unit)
    keys, slots, dist = _same_search(arc, ref, unit, 1)
    assert slots[:, 0].tolist() == [20, 21, 22, 23] and (dist >= 0).all() and (dist < 0.01).all() and not np.signbit(dist).any()
    arc.close()


def test_exact_duplicates_across_a_block_boundary_come_lowest_slot_first(gpu):
    dim, k = 64, 8
    rng = np.random.default_rng(8)
    arc, ref = _arc(200, dim)
    rows = _rows(rng, 150, dim)
    dup = list(range(57, 71)) + [3, 140]                                  # 16 > k copies, on both sides of slot 64 = the second block's first
    rows[dup] = rows[60]
    _put(arc, ref, np.arange(150), 0, 0, rows)
    assert arc.block_rows(2) == 64
    q = np.stack([rows[60] * np.float32(0.9), _rows(rng, 1, dim)[0]])
    for kk in (1, k, 32):
        keys, slots, dist = _same_search(arc, ref, q, kk)
        want = sorted(dup)[:min(kk, 16)]
        assert slots[0, :len(want)].tolist() == want and len(set(dist[0, :len(want)].tolist())) == 1
    arc.close()


def test_junk_in_free_and_never_filled_slots_is_never_returned(gpu):
    """Every byte a search could wrongly read is junk first: an import fills 48 slots' rows, scales (NaN, infinities, huge) and metadata
    with it, marked free; a second import of 20 slots leaves the junk behind the high-water mark.  Then rows are put, removed, put."""
    dim = 36
    rng = np.random.default_rng(11)
    arc, ref = _arc(48, dim)
    junk = dict(keys=np.full(48, -1, np.int64), cameras=rng.integers(0, 9, 48).astype(np.int32), t_first=np.zeros(48, np.int64),
                t_last=rng.integers(0, 9, 48).astype(np.int64), rows=rng.integers(-128, 128, (48, arc.pitch)).astype(np.int8),
                scales=np.resize(np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-3, -1e-3], np.float32), 48))
    arc.import_(junk)
    assert arc.size() == 0 and arc.high_water() == 48
    q = _rows(rng, 20, dim)
    keys, slots, dist = arc.search(q, k=4)
    assert (slots == -1).all() and (keys == -1).all() and (dist == 1e5).all()
    arc.import_({k: v[:20] for k, v in junk.items()})                     # slots 20..47: junk that was never filled
    ref.hw, ref.key, ref.cam, ref.t_first, ref.t_last = 20, [-1] * 20, [0] * 20, [0] * 20, [0] * 20
    ref.q, ref.scale = np.zeros((20, dim), np.int8), np.zeros(20, np.float32)
    _put(arc, ref, np.arange(7) + 10, 1, 1, _rows(rng, 7, dim))          # the lowest free slots: 0..6
    assert [ref.find(10 + i) for i in range(7)] == list(range(7))
    _same_search(arc, ref, q, 4)
    _same_search(arc, ref, q, 32)
    arc.remove(12), ref.remove(12)
    arc.remove(15), ref.remove(15)
    arc.remove(999), ref.remove(999)
    _same_search(arc, ref, q, 32)
    _put(arc, ref, np.arange(16) + 100, 2, 2, _rows(rng, 16, dim))       # slots 2, 5, 7..20: past the imported high-water mark
    assert ref.hw == 21 and arc.high_water() == 21
    got = _same_search(arc, ref, q, 32)
    assert (got[1] >= 0).sum(1).tolist() == [21] * 20
    _same_contents(arc, ref)
    arc.clear()
    assert arc.size() == 0 and (arc.search(q, k=2)[1] == -1).all()
    arc.close()


def test_every_filter_at_its_edge(gpu):
    dim = 64
    rng = np.random.default_rng(21)
    arc, ref = _arc(100, dim)
    rows = _rows(rng, 70, dim)
    for t in range(7):                                                    # ticks 0..6, cameras 0..4
        _put(arc, ref, np.arange(10) + 10 * t + 500, np.arange(10) % 5, t, rows[10 * t:10 * t + 10])
    q = _rows(rng, 18, dim)
    _, slots, dist = _same_search(arc, ref, q, 32)
    # t_last == t_lo and t_last == t_hi are inside
    got = _same_search(arc, ref, q, 32, since=2, until=4)
    assert sorted(got[1][0].tolist()) == [-1, -1] + list(range(20, 50))
    got = _same_search(arc, ref, q, 32, since=3, until=3)
    assert sorted(got[1][5][:10].tolist()) == list(range(30, 40)) and (got[1][:, 10:] == -1).all()
    _same_search(arc, ref, q, 8, since=5)
    _same_search(arc, ref, q, 8, until=0)
    assert (_same_search(arc, ref, q, 8, since=4, until=3)[1] == -1).all()
    # dist == max_distance is inside: every query's own 5th distance as its bound
    got = _same_search(arc, ref, q, 32, max_distance=dist[:, 4].copy())
    assert np.array_equal(got[1][:, :5], slots[:, :5]) and (got[1][:, 5:] == -1).all()
    below = np.nextafter(dist[:, 4], np.float32(-1))
    got = _same_search(arc, ref, q, 32, max_distance=below)
    assert (got[1][:, 4:] == -1).all() and np.array_equal(got[1][:, :4], slots[:, :4])
    # the nearest row's camera / key excluded: the old second comes first
    got = _same_search(arc, ref, q, 8, exclude_key=_same_search(arc, ref, q, 1)[0][:, 0].copy())
    assert np.array_equal(got[1][:, :7], slots[:, 1:8])
    got = _same_search(arc, ref, q, 8, exclude_camera=(slots[:, 0] % 10 % 5).astype(np.int32))
    assert (got[1][:, 0] != slots[:, 0]).all()
    _same_search(arc, ref, q, 8, exclude_camera=3)
    # all at once, one value per query
    _same_search(arc, ref, q, 8, exclude_camera=np.arange(18) % 6 - 1, since=np.arange(18) % 4, until=np.arange(18) % 4 + 2,
                 exclude_key=500 + np.arange(18) * 3, max_distance=np.linspace(0.8, 1.2, 18).astype(np.float32))
    arc.close()


def test_an_eviction_between_two_searches(gpu, tmp_path):
    dim = 36
    rng = np.random.default_rng(31)
    arc, ref = _arc(20, dim)
    rows = _rows(rng, 26, dim)
    for t in range(4):
        _put(arc, ref, np.arange(5) + 5 * t, t, t, rows[5 * t:5 * t + 5])
    q = np.concatenate([rows[[0, 3, 21, 24]], _rows(rng, 3, dim)])
    got = _same_search(arc, ref, q, 3)
    assert got[1][:2, 0].tolist() == [0, 3]
    _put(arc, ref, [7, 100, 101, 102], 9, 4, rows[[7, 21, 22, 23]])       # an upsert (slot 7 now has t_last 4) and three evictions: slots 0, 1, 2
    assert ref.find(0) == -1 and ref.find(100) == 0 and ref.find(3) == 3 and ref.t_first[7] == 1 and ref.t_last[7] == 4
    got = _same_search(arc, ref, q, 3)
    assert got[1][1, 0] == 3 and got[1][2, 0] == 0 and got[0][2, 0] == 100 and 0 not in got[0][0]
    _put(arc, ref, [103, 104, 105], 9, 5, rows[[24, 25, 0]])              # slots 3, 4 (t_last 0), then 5 (t_last 1: slot 7 was refreshed)
    assert ref.find(105) == 5 and ref.find(7) == 7
    _same_search(arc, ref, q, 20)
    e = _same_contents(arc, ref)
    # save / load into another archive: the same answers, the same next slots
    path = str(tmp_path / "archive.npz")
    arc.save(path)
    other = pkg("archive").IdentityArchive(20, dim)
    other.load(path)
    assert all(np.array_equal(e[k], v) for k, v in other.export().items())
    for a in (arc, other):
        a.remove(8)
    ref.remove(8)
    for a in (arc, other):
        a.put([200], 1, 6, rows[11:12])
    ref.put([200], [1], 6, rows[11:12])
    assert ref.find(200) == 8
    _same_search(arc, ref, q, 20)
    _same_search(other, ref, q, 20)
    with pytest.raises(ValueError):
        pkg("archive").IdentityArchive(20, 64).load(path)
    arc.close(), other.close()


# ---------------------------------------------------------------------------------------------------- 3. returning tracks
def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def _ref_step(ref, pol, shards, tick, min_gap, thr):
    """The three steps a link pass adds with an archive attached, restated on the pass's shard array."""
    S, T, _ = shards.shape
    live = [(s * T + r, s, int(shards[s, r, 1]), pol.key(s, int(shards[s, r, 1])), shards[s, r, 2:]) for s in range(S) for r in range(T)
            if shards[s, r, 0] > 0.5]
    fresh = [x for x in live if ref.find(x[3]) < 0]
    out = []
    if fresh and ref.hw:
        keys, slots, dist = ref.search(np.stack([x[4] for x in fresh]), k=1, t_hi=tick - 1 - min_gap, max_distance=np.float32(thr))
        winner = {}
        for j in range(len(fresh)):
            s = int(slots[j, 0])
            if s >= 0 and (s not in winner or (dist[j, 0].view(np.uint32), fresh[j][0]) < (dist[winner[s], 0].view(np.uint32), fresh[winner[s]][0])):
                winner[s] = j
        for j in sorted(winner.values()):
            ak = int(keys[j, 0])
            pol.first.setdefault(ak, ak)
            pol.link_keys(fresh[j][3], ak)
            out.append((fresh[j][1], fresh[j][2], ak, float(dist[j, 0])))
    if live:
        ref.put([x[3] for x in live], [x[1] for x in live], tick, np.stack([x[4] for x in live]))
    return out


def test_returning_tracks_against_the_oracle(gpu):
    """S = 3, t_max = 8, dim 64, hand-made shards through link_shards.  Person p: camera 0 track 7 in passes 0..2, gone, then camera 1
    track 4 from pass 6 (reported once, and the two share a global id).  Person r: camera 2 track 3 in passes 0..6; from pass 7 camera 0
    track 9 -- the archived row is one pass old, min_gap = 1 keeps it from being reported.  Person u: camera 2 track 5 in passes 0..2; at pass 9 two new tracks resemble u: one of them gets the archived row."""
    S, T, dim = 3, 8, 64
    rng = np.random.default_rng(77)
    p, r, u = (_unit(rng.standard_normal(dim)) for _ in range(3))
    near = lambda v, seed: _unit(v + 0.02 * np.random.default_rng(seed).standard_normal(dim))      # noqa: E731
    X = pkg("xcam")
    xc, plain = X.CrossCamera(S, T, dim, THR), X.CrossCamera(S, T, dim, THR)
    arc, ref = _arc(64, dim)
    xc.attach_archive(arc)
    pol, pol_plain = KeyPolicyRef(S), KeyPolicyRef(S)
    seen = {}
    for tick in range(11):
        cams = [[], [], []]
        if tick <= 2:
            cams[0].append((7, near(p, tick)))
            cams[2].append((5, near(u, 100 + tick)))
        if tick <= 6:
            cams[2].append((3, near(r, 200 + tick)))
        if tick >= 6:
            cams[1].append((4, near(p, 300 + tick)))
        if tick >= 7:
            cams[0].append((9, near(r, 400 + tick)))
        if tick >= 9:
            cams[0].append((11, near(u, 500)))
            cams[1].append((12, near(u, 501)))
        shards = rng.standard_normal((S, T, 2 + dim)).astype(np.float32)  # junk behind the valid prefix
        shards[:, :, :2] = 0
        for s, rows in enumerate(cams):
            for i, (tid, v) in enumerate(rows):
                shards[s, i, 0], shards[s, i, 1], shards[s, i, 2:] = 1, tid, v
        links = xc.link_shards(shards)
        assert plain.link_shards(shards) == links                         # what a pass without an archive does is unchanged ...
        for a, b in zip(xc.tables(), plain.tables()):
            assert np.array_equal(a, b)
        assert np.array_equal(xc.shards(), shards)
        ids, nr, nd = xc.tables()
        assert pol.update(T, ids, nr, nd, THR) == links == pol_plain.update(T, ids, nr, nd, THR)
        want = _ref_step(ref, pol, shards, tick, 1, THR)
        got = xc.returning()
        assert got == want, (tick, got, want)
        seen[tick] = got
        _same_contents(arc, ref)
        for s in range(S):
            tids = [7, 9, 11, 4, 12, 3, 5, 99]
            assert xc.global_ids(s, tids).tolist() == [pol.lookup(s, t) for t in tids], (tick, s)
            assert plain.global_ids(s, tids).tolist() == [pol_plain.lookup(s, t) for t in tids]
        assert plain.returning() == []
    key = lambda s, t: (s << 32) | t                                      # noqa: E731
    assert [len(seen[t]) for t in range(11)] == [0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    assert seen[6][0][:3] == (1, 4, key(0, 7)) and 0 < seen[6][0][3] < THR
    assert xc.global_ids(1, [4])[0] == xc.global_ids(0, [7])[0] == key(0, 7) and plain.global_ids(1, [4])[0] == key(1, 4)
    assert seen[9][0][2] == key(2, 5) and seen[9][0][:2] in ((0, 11), (1, 12))
    assert xc.global_ids(0, [9])[0] == plain.global_ids(0, [9])[0] == key(0, 9)      # one pass after r left: not a return under min_gap = 1
    # strided rows read in place: a [2, 3, 2 + dim] shard array, deposited by a pass
    for d in (4, 36, 512):
        x2 = X.CrossCamera(2, 3, d, THR)
        a2, r2 = _arc(8, d)
        x2.attach_archive(a2)
        sh = _rows(rng, 6, 2 + d).reshape(2, 3, 2 + d)
        sh[:, :, 0], sh[:, :, 1] = [[1, 1, 0], [1, 0, 0]], [[5, 6, 0], [5, 0, 0]]
        x2.link_shards(sh)
        r2.put([5, 6, (1 << 32) | 5], [0, 0, 1], 0, sh[[0, 0, 1], [0, 1, 0], 2:])
        _same_contents(a2, r2)
        x2.close(), a2.close()
    # min_gap = 0 on a fresh pair: the row deposited one pass ago is reported
    x3 = X.CrossCamera(S, T, dim, THR)
    a3, _ = _arc(8, dim)
    x3.attach_archive(a3)
    x3.option("min_gap", 0)
    sh = np.zeros((S, T, 2 + dim), np.float32)
    sh[0, 0, 0], sh[0, 0, 1], sh[0, 0, 2:] = 1, 7, p
    x3.link_shards(sh)
    sh[0, 0, 1] = 8                                                       # the same row under a new id, one pass later
    x3.link_shards(sh)
    assert [g[:3] for g in x3.returning()] == [(0, 8, 7)]
    for o in (xc, plain, x3, arc, a3):
        o.close()


def test_a_deepsort_bank_deposits_its_shards(gpu):
    """2 cameras, 4 frames, link_cameras(archive=...): the archive holds what the oracle holds after the bank's own shard array."""
    cams = [[0, 1, 2], [1]]
    bank = pkg("deepsort_bank").DeepSORTBank(2, max_tracks=16, feature_dim=BANK_DIM, n_init=3, nn_budget=2)
    arc, ref = _arc(32, BANK_DIM)
    pol = KeyPolicyRef(2)
    for tick in range(4):
        bank.update_arrays([[deepsort_tick(p, c, tick)] for c, p in enumerate(cams)])
    for tick in range(2):
        bank.link_cameras(archive=arc)
        assert bank.xcam.archive is arc
        shards = bank.xcam.shards()
        assert (shards[:, :, 0] > 0.5).sum(1).tolist() == [3, 1]
        ids, nr, nd = bank.xcam.tables()
        pol.update(16, ids, nr, nd, bank.xcam.max_cosine_distance)
        assert _ref_step(ref, pol, shards, tick, 1, bank.xcam.max_cosine_distance) == bank.xcam.returning() == []
        e = _same_contents(arc, ref)
        assert e["t_first"].tolist() == [0] * 4 and e["t_last"].tolist() == [tick] * 4 and e["cameras"].tolist() == [0, 0, 0, 1]
    for o in (bank.xcam, bank, arc):
        o.close()


def test_cli_archive_reports_returning_tracks_across_two_runs(gpu, tmp_path):
    """--archive with --archive_file, twice on the same synthetic source: the first run saves what its passes deposited; the second loads
    it, its tracks are new keys (the cameras start a generation above the file's), and with --archive_min_gap 0 they are reported as
    returning with the first run's keys."""
    import json
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    _, rpath = pkg("engine_file").ensure_seeded_engines(ROOT)
    src = "synthetic:1280x720:5:8:1"
    path = tmp_path / "seen.npz"
    seen = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        rc = pkg("cli").main(["--inputs", f"{src},{src}", "--output_dir", str(out), "--yolo_engine", ypath, "--reid_engine", rpath, "--tracker", "botsort",
                              "--batch", "8", "--link_cameras", "--archive", "256", "--archive_file", str(path),
                              "--archive_min_gap", "0"])
        assert rc == 0 and path.exists()
        with np.load(path) as z:
            keys = z["keys"][z["keys"] >= 0]
        seen.append(set(keys.tolist()))
        ret = []
        for k in range(2):
            (jl,) = out.glob(f"*_s{k}.jsonl")
            for line in map(json.loads, jl.read_text().splitlines()):
                assert isinstance(line["returning"], list) and len(line["global_ids"]) == len(line["tracks"])
                ret += [tuple(r[:2]) for r in line["returning"]]
        if run == 0:
            assert seen[0] and all(k >> 44 == 0 for k in seen[0]) and not ret     # nothing to return to yet
        else:
            assert seen[0] < seen[1] and all(k >> 44 == 1 for k in seen[1] - seen[0])
            assert ret and {key for _, key in ret} <= seen[0]                     # the first run's rows answered
