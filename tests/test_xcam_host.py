"""Cross-camera identities of a bank (aic_xcam_*) without a GPU: the symbols, the rejections that come before the
device, the per-rank generation of the global-id table (aic_gid_forget_rank), the policy against a Python restatement, and the register
budget of the new kernels."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

NEW = tuple(f"aic_xcam_{f}" for f in ("create", "destroy", "option", "link_deepsort_bank", "link_botsort_bank", "link_shards", "tables",
                                      "shards", "global_ids", "size", "forget_stream")) + ("aic_gid_forget_rank", "aic_pipeline_link_cameras")


def test_symbols_declared_and_exported():
    L = pkg("_lib")
    hdr = open(os.path.join(ROOT, "include", "aicam.h")).read()
    lib = L.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in L.EXPORTS
        getattr(lib, name)
    assert pkg().CrossCamera is pkg("xcam").CrossCamera
    for bank in (pkg("deepsort_bank").DeepSORTBank, pkg("botsort").BoTSORTBank):
        assert issubclass(bank, pkg("xcam").CameraLinks) and issubclass(bank, pkg("bytetrack").TrackerBank)
        assert bank.reset is pkg("xcam").CameraLinks.reset                 # reset(stream) forgets the stream in the attached object
    assert not issubclass(pkg("bytetrack").BYTETrackerBank, pkg("xcam").CameraLinks)


# ---- rejections before the device (on a machine without one, anything that got past them would answer AIC_ERR_NO_DEVICE instead)
@pytest.mark.parametrize("args,word", [((0, 16, 32, 0.2), b"streams"), ((257, 16, 32, 0.2), b"streams"), ((-1, 16, 32, 0.2), b"streams"),
                                       ((4, 0, 32, 0.2), b"t_max"), ((4, 513, 32, 0.2), b"t_max"),
                                       ((4, 16, 0, 0.2), b"dim"), ((4, 16, 6, 0.2), b"dim"), ((4, 16, 1028, 0.2), b"dim"),
                                       ((4, 16, 32, -0.1), b"max_cosine_distance"), ((4, 16, 32, float("nan")), b"max_cosine_distance")])
def test_create_rejects_before_the_device(args, word):
    L = pkg("_lib")
    h = C.c_void_p()
    rc = L.load().aic_xcam_create(0, *args, C.byref(h))
    assert rc == L.ERR_INVALID and not h.value
    assert word in L.load().aic_last_error()


def test_null_handles_rejected():
    L = pkg("_lib")
    lib = L.load()
    n = C.c_int32()
    assert lib.aic_xcam_create(0, 4, 16, 32, 0.2, None) == L.ERR_INVALID
    assert lib.aic_xcam_link_deepsort_bank(None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.aic_xcam_link_botsort_bank(None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.aic_xcam_link_shards(None, None, None, L.HOST, C.byref(n)) == L.ERR_INVALID
    assert lib.aic_pipeline_link_cameras(None, None, C.byref(n)) == L.ERR_INVALID
    assert lib.aic_xcam_forget_stream(None, 0) == L.ERR_INVALID
    assert lib.aic_gid_forget_rank(None, 0) == L.ERR_INVALID


def test_no_device():
    L = pkg("_lib")
    if L.device_count() > 0:
        pytest.skip("a GPU is visible: covered by tests/test_gpu_xcam.py")
    h = C.c_void_p()
    assert L.load().aic_xcam_create(0, 4, 16, 32, 0.2, C.byref(h)) == L.ERR_NO_DEVICE and not h.value
    with pytest.raises(L.NoDeviceError):
        pkg("xcam").CrossCamera(4, 16, 32)


def test_python_rejections_need_no_device():
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline.link_cameras(type("P", (), dict(tracker_kind="bytetrack", cameras=0, xcam=None))())
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline.link_cameras(type("P", (), dict(tracker_kind="botsort", cameras=0, xcam=None))())
    with pytest.raises(SystemExit):
        pkg("cli").parse_arguments(["--link_cameras", "--tracker", "botsort", "--input", "a.npy"])
    with pytest.raises(SystemExit):
        pkg("cli").parse_arguments(["--link_cameras", "--tracker", "bytetrack", "--inputs", "a.npy,b.npy"])
    assert pkg("cli").parse_arguments(["--link_cameras", "--tracker", "botsort", "--inputs", "a.npy,b.npy"]).link_cameras


# ---- the policy, restated (csrc/global_id.cpp; shared with tests/test_gpu_xcam.py)
class PolicyRef:
    """A track is known by (generation, rank, track id); its global id is the key of the first sighting of its identity.  First sighting:
    its own key.  Rows i < j of different ranks that are each other's nearest row within the threshold (compared in fp32) unite, in
    ascending order of i; the smaller id is the root."""

    def __init__(self, world):
        self.world, self.first, self.parent, self.gen = world, {}, {}, {}

    def key(self, rank, tid):
        return (self.gen.get(rank, 0) << 44) | (rank << 32) | (tid & 0xffffffff)

    def find(self, g):
        while g in self.parent:
            g = self.parent[g]
        return g

    def update(self, t_max, ids, near, dist, thr):
        n, links = self.world * t_max, 0
        for i in range(n):
            if ids[i] >= 0:
                self.first.setdefault(self.key(i // t_max, int(ids[i])), self.key(i // t_max, int(ids[i])))
        for i in range(n):
            j = int(near[i])
            if ids[i] < 0 or j <= i or j >= n or ids[j] < 0 or int(near[j]) != i or not np.float32(dist[i]) <= np.float32(thr):
                continue
            a = self.find(self.first[self.key(i // t_max, int(ids[i]))])
            b = self.find(self.first[self.key(j // t_max, int(ids[j]))])
            if a != b:
                self.parent[max(a, b)] = min(a, b)
                links += 1
        return links

    def lookup(self, rank, tid):
        k = self.key(rank, tid)
        return self.find(self.first[k]) if k in self.first else -1

    def forget(self, rank):
        self.gen[rank] = self.gen.get(rank, 0) + 1


class Gid:
    def __init__(self, world):
        self.L, self.world = pkg("_lib"), world
        self.h = C.c_void_p()
        self.L.call("aic_gid_create", world, C.byref(self.h))

    def update(self, t_max, ids, near, dist, thr):
        n = C.c_int32()
        self.L.call("aic_gid_update", self.h, self.world, t_max, self.L.ptr(ids), self.L.ptr(near), self.L.ptr(dist), float(thr), C.byref(n))
        return n.value

    def lookup(self, rank, tid):
        g = C.c_int64()
        self.L.call("aic_gid_lookup", self.h, rank, tid, C.byref(g))
        return g.value

    def forget(self, rank):
        self.L.call("aic_gid_forget_rank", self.h, rank)

    def size(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self.L.call("aic_gid_size", self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def __del__(self):
        self.L.load().aic_gid_destroy(self.h)


def _table(world, t_max, pairs, ids, dist=0.05):
    """ids [world * t_max] (-1 = empty); pairs: (i, j) each other's nearest row at `dist` (or (i, j, d))."""
    n = world * t_max
    near, nd = np.full(n, -1, np.int32), np.full(n, 1e5, np.float32)
    for p in pairs:
        i, j, d = (p + (dist,))[:3]
        near[i], near[j], nd[i], nd[j] = j, i, d, d
    return np.asarray(ids, np.int32), near, nd


def test_policy_first_sighting_mutual_order_and_root():
    g, ref = Gid(3), PolicyRef(3)
    t = 4
    ids = [10, 11, -1, -1, 20, 21, 22, -1, 30, -1, -1, -1]
    # row 0 <-> row 4 mutual within the threshold; 1 <-> 5 mutual but too far; 6 -> 8 one-sided (8's nearest is 0)
    tid, near, nd = _table(3, t, [(0, 4), (1, 5, 0.5)], ids)
    near[6], nd[6], near[8], nd[8] = 8, 0.01, 0, 0.02
    for o in (g, ref):
        assert o.update(t, tid, near, nd, 0.2) == 1
    key = lambda r, i: (r << 32) | i                                      # noqa: E731 -- generation 0: today's keys
    assert g.lookup(0, 10) == g.lookup(1, 20) == key(0, 10)              # the smaller id is the root
    assert g.lookup(0, 11) == key(0, 11) and g.lookup(1, 21) == key(1, 21) and g.lookup(1, 22) == key(1, 22) and g.lookup(2, 30) == key(2, 30)
    assert g.lookup(2, 31) == -1 and g.lookup(0, 12) == -1
    assert g.size() == (6, 5, 1)
    # two more pairs in one update: (0, 11)-(1, 21) and (1, 22)-(2, 30), each rooted at its smaller id
    tid, near, nd = _table(3, t, [(1, 5), (6, 8)], ids)
    for o in (g, ref):
        assert o.update(t, tid, near, nd, 0.2) == 2
    tid, near, nd = _table(3, t, [(5, 8)], ids)                          # camera 1's track 21 now faces camera 2's 30: three cameras, one identity
    for o in (g, ref):
        assert o.update(t, tid, near, nd, 0.2) == 1
    assert g.lookup(2, 30) == g.lookup(1, 22) == g.lookup(1, 21) == g.lookup(0, 11) == key(0, 11)
    for r, i in ((0, 10), (0, 11), (1, 20), (1, 21), (1, 22), (2, 30), (2, 7)):
        assert g.lookup(r, i) == ref.lookup(r, i)
    # the same pairs again: nothing new
    assert g.update(t, tid, near, nd, 0.2) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_policy_agrees_with_the_library_on_seeded_tables(seed):
    rng = np.random.default_rng(seed)
    world, t = 5, 6
    n = world * t
    g, ref = Gid(world), PolicyRef(world)
    for step in range(6):
        ids = np.where(rng.random(n) < 0.7, rng.integers(1, 9, n), -1).astype(np.int32)
        for r in range(world):                                            # ids are unique within a camera
            seen = set()
            for k in range(r * t, (r + 1) * t):
                if ids[k] in seen:
                    ids[k] = -1
                seen.add(int(ids[k]))
        near = np.full(n, -1, np.int32)
        nd = np.full(n, 1e5, np.float32)
        for i in np.nonzero(ids >= 0)[0]:
            other = [j for j in np.nonzero(ids >= 0)[0] if j // t != i // t]
            if other:
                near[i] = rng.choice(other)
        for i in range(n):                                                # make about half of the pairs mutual, distances symmetric
            j = near[i]
            if j >= 0 and rng.random() < 0.5:
                near[j] = i
        for i in range(n):
            j = near[i]
            if j >= 0:
                nd[i] = np.float32(0.01 * ((min(i, j) * 31 + max(i, j) * 7 + step) % 40))
        assert g.update(t, ids, near, nd, 0.2) == ref.update(t, ids, near, nd, 0.2)
        if step == 3:
            g.forget(2), ref.forget(2)
        for r in range(world):
            for i in range(0, 10):
                assert g.lookup(r, i) == ref.lookup(r, i), (step, r, i)


def test_forget_rank():
    t = 2
    ids = [5, 6, 5, 7]
    g, old = Gid(2), Gid(2)
    tid, near, nd = _table(2, t, [(0, 2)], ids)
    assert g.update(t, tid, near, nd, 0.2) == old.update(t, tid, near, nd, 0.2) == 1
    before = [g.lookup(r, i) for r, i in ((0, 5), (0, 6), (1, 5), (1, 7))]
    assert before == [old.lookup(r, i) for r, i in ((0, 5), (0, 6), (1, 5), (1, 7))] == [5, 6, 5, (1 << 32) | 7]   # unchanged against the existing calls
    g.forget(0)
    assert g.lookup(0, 5) == -1 and g.lookup(0, 6) == -1                 # the old generation no longer resolves
    assert g.lookup(1, 5) == 5 and g.lookup(1, 7) == (1 << 32) | 7       # the peer that adopted camera 0's id keeps it
    # the recycled local id 5 on camera 0 is somebody else, seen beside camera 1's track 7
    tid, near, nd = _table(2, t, [(0, 3)], [5, -1, 5, 7])
    assert g.update(t, tid, near, nd, 0.2) == 1
    new5 = g.lookup(0, 5)
    assert new5 == (1 << 32) | 7 and new5 != before[0]                   # a new identity (root: the smaller id, camera 1's)
    assert g.lookup(1, 5) == 5
    tid, near, nd = _table(2, t, [], [6, -1, -1, -1])
    g.update(t, tid, near, nd, 0.2)
    assert g.lookup(0, 6) == (1 << 44) | 6                               # generation 1 key of (rank 0, id 6)
    L = pkg("_lib")
    assert L.load().aic_gid_forget_rank(g.h, 2) == L.ERR_INVALID and L.load().aic_gid_forget_rank(g.h, -1) == L.ERR_INVALID


def test_new_kernels_have_no_scratch_and_no_spills():
    """The budget of tests/test_host_logic.py::test_no_conv_kernel_spills for the kernels of kernels_xcam.hip, through tools/kernel_resources.py."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    tab = {k: r for k, r in kr.kernel_table(kr.Path(ROOT) / "ai-camera_amd" / "libaicam.so").items() if "xcam_" in k}
    for name in ("xcam_pack_deepsort_kernel", "xcam_pack_botsort_kernel", "xcam_count_kernel", "xcam_finalize_kernel"):
        assert sum(name in k for k in tab) == 1, (name, sorted(tab))
    assert sum("xcam_nearest_kernel" in k for k in tab) == 2             # the 32- and the 64-row tile
    bad = {k: r for k, r in tab.items() if r["scratch"] or r["vgpr_spills"]}
    assert not bad, bad
    # the tile kernels keep several blocks per CU: <= 128 registers (4 waves per SIMD) and <= 40 KiB of LDS (4 blocks in 160 KiB)
    for k, r in tab.items():
        if "xcam_nearest_kernel" in k:
            assert r["vgpr"] + r["agpr"] <= 128 and r["lds"] <= 40 * 1024, (k, r)
