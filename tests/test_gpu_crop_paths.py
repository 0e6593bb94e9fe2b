"""The crop resamplers on the device against the integer contract (oracle/image_oracle.py through tests/crop_cases.py), bit for bit:
np.array_equal everywhere, no tolerance.  What the cases reach and which wrong kernels they catch is proved on the CPU in
tests/test_crop_cases.py.

  crop_resize_kernel     through aic_crop_resize_ex: every output shape x layout x element type, byte loads (slack = 0) and the
                         aligned 12-byte loads (slack = 1), the bank at every byte offset of its buffer, frame_of over three frames,
                         a device-side crop count; the buffer around the bank holds 0xA5, the output is prefilled with 0xFF bytes
                         and valid with -1
  reid_stem_pool2_kernel the crop fused into the ReID stem, through aic_reid_embed_bank (set up as the pipeline's device-filtered
                         round): the stem's POOLED tensor and the embeddings against the same engine fed with the oracle's crops --
                         the crop kernel is not involved

A HIP error ends the session: nothing more is started on a device that has just faulted."""
import functools
import os

import numpy as np
import pytest

import crop_cases as K
import elt_ref as E
from conftest import pkg

pytestmark = pytest.mark.gpu
L = pkg("_lib")
ip = pkg("image_processing")

MODE_IDS = [f"mode{m}_{d}" for m, d in K.MODES]
SHAPE_IDS = [f"{h}x{w}" for h, w in K.CROP_SHAPES]


def _stop_on_runtime_error(fn):
    """The refusals these tests provoke are argument checks (ERR_INVALID, ERR_CAPACITY) made before any launch; anything else the
    library reports is a HIP error and ends the session."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        try:
            return fn(*a, **kw)
        except L.AicError as e:
            if e.code in (L.ERR_INVALID, L.ERR_CAPACITY):
                raise
            pytest.exit(f"{fn.__name__}: the library reported an error, stopping: {e}", returncode=1)
    return wrapped


def _case(shape):
    boxes, fo = K.boxes_for(shape)
    return K.bank(K.BANK_OF[shape]), boxes, fo


def _prefill_left(t):
    """Elements that still hold the entry's 0xFF prefill (a NaN of either width; no expected value is one)."""
    return int((t.view(np.uint8).reshape(-1, t.itemsize) == 0xFF).all(1).sum())


def _check(tag, got, gv, exp, ev):
    assert got.dtype == exp.dtype and got.shape == exp.shape, (tag, got.dtype, got.shape)
    assert gv.tolist() == ev.tolist(), (tag, "valid", gv.tolist(), ev.tolist())
    assert _prefill_left(got) == 0, (tag, "elements nothing stored", _prefill_left(got))
    if not np.array_equal(got, exp):
        bad = sorted({int(i) for i in np.argwhere(got != exp)[:, 0]})
        i = bad[0]
        where = np.argwhere(got[i] != exp[i])[0].tolist()
        raise AssertionError(f"{tag}: crops {bad} differ; crop {i} first at {where}: got {got[i][tuple(where)]}, expected {exp[i][tuple(where)]}")


# ------------------------------------------------------------------------------------------------------------------ crop kernel
@pytest.mark.parametrize("byte_offset", [0, 1, 2, 3])
@pytest.mark.parametrize("mode,dtype", K.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", K.CROP_SHAPES, ids=SHAPE_IDS)
@_stop_on_runtime_error
def test_crop_kernel_bit_exact(gpu, shape, mode, dtype, byte_offset):
    """Both load forms of one case in one test: slack = 0 (bytes) and slack = 1 (aligned 12-byte loads + alignbyte) each equal the
    oracle, and so each other."""
    frames, boxes, fo = _case(shape)
    exp, ev = K.expected(shape, mode, dtype)
    out = {}
    for slack in (0, 1):
        got, gv = ip.crop_resize_ex(frames, boxes, fo, shape, mode=mode, dtype=dtype, slack=slack, byte_offset=byte_offset)
        _check(f"{shape} mode {mode} {dtype} slack {slack} offset {byte_offset}", got, gv, exp, ev)
        out[slack] = got
    assert np.array_equal(out[0].view(np.uint8), out[1].view(np.uint8))


@pytest.mark.parametrize("n_live", [0, 1, 21, 22, 27], ids=lambda v: f"live{v}")
@pytest.mark.parametrize("mode,dtype", K.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", [(16, 64), (20, 24)], ids=["16x64", "20x24"])
@_stop_on_runtime_error
def test_crop_kernel_device_count(gpu, shape, mode, dtype, n_live):
    """n_dev: rows below min(n_live, n) as expected, the rows beyond all zero with valid == 0 (n = 22: n_live = 0, 1, n - 1, n, n + 5)."""
    frames, boxes, fo = _case(shape)
    n = len(boxes)
    assert n == 22
    exp, ev = K.expected(shape, mode, dtype, n_live=n_live)
    k = min(n_live, n)
    assert not exp[k:].any() and not ev[k:].any()
    for slack in (0, 1):
        got, gv = ip.crop_resize_ex(frames, boxes, fo, shape, mode=mode, dtype=dtype, slack=slack, byte_offset=1, n_live=n_live)
        _check(f"{shape} mode {mode} {dtype} slack {slack} n_live {n_live}", got, gv, exp, ev)
        assert not got[k:].any() and not gv[k:].any()


@_stop_on_runtime_error
def test_crop_kernel_without_frame_of_reads_frame_0(gpu):
    shape = (16, 64)
    frames, boxes, fo = _case(shape)
    exp, ev = K.expected(shape, mut="frame_of")             # (the "mutant" that ignores frame_of is what frame_of == NULL asks for)
    for slack in (0, 1):
        got, gv = ip.crop_resize_ex(frames, boxes, None, shape, slack=slack, byte_offset=3)
        _check(f"no frame_of, slack {slack}", got, gv, exp, ev)


@_stop_on_runtime_error
def test_crop_kernel_refusals(gpu):
    shape = (16, 64)
    frames, boxes, fo = _case(shape)
    with pytest.raises(L.AicError) as e:                    # the fp32 kernel has no NHWC4 store: refused in launch_crop_resize
        ip.crop_resize_ex(frames, boxes, fo, shape, mode=2, dtype="fp32")
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(L.AicError) as e:
        ip.crop_resize_ex(frames, boxes, fo, (8, 241))
    assert e.value.code == L.ERR_CAPACITY
    with pytest.raises(L.AicError) as e:                    # frame_of is checked on the host: no kernel sees an index outside the bank
        ip.crop_resize_ex(frames, boxes, np.full(len(boxes), K.N_FRAMES, np.int32), shape)
    assert e.value.code == L.ERR_INVALID
    with pytest.raises(L.AicError) as e:
        ip.crop_resize_ex(frames, boxes, fo, shape, byte_offset=4)
    assert e.value.code == L.ERR_INVALID
    got, gv = ip.crop_resize_ex(frames, boxes, fo, shape)   # ... and the library goes on working
    exp, ev = K.expected(shape)
    _check("after the refusals", got, gv, exp, ev)


@pytest.mark.parametrize("shape", K.CROP_SHAPES, ids=SHAPE_IDS)
@_stop_on_runtime_error
def test_product_entry_gives_the_same_bits(gpu, shape):
    """aic_crop_resize (one frame, NCHW fp32, byte loads) against the test entry at mode 0 on each frame of the bank."""
    frames, boxes, fo = _case(shape)
    for fi in range(K.N_FRAMES):
        a, av = ip.crops_from_boxes(frames[fi], boxes, shape)
        b, bv = ip.crop_resize_ex(frames, boxes, np.full(len(boxes), fi, np.int32), shape)
        assert av.tolist() == bv.tolist() and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (shape, fi)


# ------------------------------------------------------------------------------------------------------------------ fused stem
STEM_H = [16, 32, 128]


class _Stem:
    """An fp16 engine whose stem is fused and what it makes of the ORACLE's crops: the stem's pooled tensor and the embeddings, computed
    once and left unchanged.  H = 16, 32: elt_ref's stem2_H{H} graph (random non-zero weights, conv 3x3 + ReLU + max pool 3x3/2, W = 64);
    H = 128: the session's seeded ReID engine, the shape the pipeline runs, on the 262-row bank."""

    def __init__(self, H, tmp, reid_path):
        HipEngine = pkg("hip_engine").HipEngine
        self.shape = (H, 64)
        bank = K.STEM_BANK_OF[self.shape]
        self.frames = K.bank(bank)
        self.boxes, self.fo = K.boxes_for(self.shape, bank)
        self.n = len(self.boxes)
        if H == 128:
            self.path = reid_path
            g = E.ef.read_engine(reid_path)
            self.ybuf = next(o for o in g.ops if o[0] == E.ef.OP_MAXPOOL3S2)[4]           # the fused stem's output
            assert g.buffers[self.ybuf][:3] == (64, 32, 64)
        else:
            c = next(c for c in E.CASES if c.id == f"stem2_H{H}_fp16")
            B = E.build_graph(c)
            self.path = os.path.join(tmp, f"{c.id}.aicw")
            E.ef.write_engine(self.path, B.g)
            self.ybuf = B.bufs["y"]
        self.eng = HipEngine(self.path, dtype="fp16", max_items=self.n, warm_up=False)
        self.crops, self.valid = K.expected(self.shape, bank_name=bank)
        self.crops0, self.valid0 = K.expected(self.shape, mut="frame_of", bank_name=bank)     # what frame_of == NULL asks for: frame 0
        self.emb = self.eng.reid_infer_np(self.crops)
        self.pooled = self.eng.read_buffer_np(self.ybuf, self.n)
        assert self.pooled.shape == (self.n, H // 2, 32, 64) and self.pooled.dtype == np.float16
        self.emb.setflags(write=False), self.pooled.setflags(write=False)
        self.noise = np.random.default_rng(H).uniform(-1, 1, self.crops.shape).astype(np.float32)

    def dirty(self):
        """Another run in between: what the buffers hold is no longer the expectation, a kernel that stored nothing would show."""
        self.eng.reid_infer_np(self.noise)
        assert not np.array_equal(self.eng.read_buffer_np(self.ybuf, self.n), self.pooled)


@pytest.fixture(scope="module")
def stems(tmp_path_factory, engines):
    tmp = str(tmp_path_factory.mktemp("crop_stem"))
    made = {}

    def get(H):
        if H not in made:
            made[H] = _Stem(H, tmp, engines[1])
        return made[H]
    yield get
    for s in made.values():
        s.eng.close()


@pytest.mark.parametrize("byte_offset", [0, 1, 2, 3])
@pytest.mark.parametrize("H", STEM_H)
@_stop_on_runtime_error
def test_fused_stem_crop_bit_exact(gpu, stems, H, byte_offset):
    s = stems(H)
    assert len(set(s.fo.tolist())) == K.N_FRAMES and s.fo.tolist() != sorted(s.fo.tolist())
    s.dirty()
    emb, valid = s.eng.embed_bank_np(s.frames, s.boxes, s.fo, byte_offset=byte_offset)
    pooled = s.eng.read_buffer_np(s.ybuf, s.n)
    assert valid.tolist() == s.valid.tolist() and 0 < valid.sum() < s.n
    ok = valid == 1
    bad = [int(i) for i in np.flatnonzero(ok) if not np.array_equal(pooled[i], s.pooled[i])]
    assert not bad, f"H {H} offset {byte_offset}: the stem's pooled tensor differs for crops {bad}"
    assert pooled[ok].any()
    assert np.array_equal(emb[ok], s.emb[ok])
    # an empty box is a zero patch, which is what the oracle's zero crop becomes on the other path
    assert np.array_equal(pooled[~ok], s.pooled[~ok]) and np.array_equal(emb[~ok], s.emb[~ok])


@pytest.mark.parametrize("n_live", [1, 21, 22], ids=lambda v: f"live{v}")
@pytest.mark.parametrize("H", STEM_H)
@_stop_on_runtime_error
def test_fused_stem_device_count(gpu, stems, H, n_live):
    """n_items_dev: the rows below n_live are asserted; the kernels return early for the rest and leave them as they were."""
    s = stems(H)
    s.dirty()
    emb, valid = s.eng.embed_bank_np(s.frames, s.boxes, s.fo, byte_offset=2, n_live=n_live)
    pooled = s.eng.read_buffer_np(s.ybuf, s.n)
    assert valid[:n_live].tolist() == s.valid[:n_live].tolist()
    assert np.array_equal(pooled[:n_live], s.pooled[:n_live]) and pooled[:n_live].any()
    if H != 128:            # (behind the real engine's stem a device-side count may select other conv kernels: another summation order)
        assert np.array_equal(emb[:n_live], s.emb[:n_live])
    else:
        assert np.abs(emb[:n_live] - s.emb[:n_live]).max() < 1e-3     # two fp16 runs of the same crops: test_reid_large_batch_kernels' bound


@_stop_on_runtime_error
def test_fused_stem_without_frame_of_reads_frame_0(gpu, stems):
    s = stems(16)
    crops0, v0 = s.crops0, s.valid0
    ref = s.eng.reid_infer_np(crops0)
    pooled_ref = s.eng.read_buffer_np(s.ybuf, s.n)
    s.dirty()
    emb, valid = s.eng.embed_bank_np(s.frames, s.boxes, None, byte_offset=1)
    assert valid.tolist() == v0.tolist()
    assert np.array_equal(s.eng.read_buffer_np(s.ybuf, s.n), pooled_ref) and np.array_equal(emb, ref)


@_stop_on_runtime_error
def test_fused_stem_refusals(gpu, stems, tmp_path):
    HipEngine = pkg("hip_engine").HipEngine
    s = stems(16)

    def refused(eng, *a, **kw):
        with pytest.raises(L.AicError) as e:
            eng.embed_bank_np(*a, **kw)
        assert e.value.code == L.ERR_INVALID

    f32 = HipEngine(s.path, dtype="fp32", max_items=s.n, warm_up=False)          # not fp16: the stem is not fused at all
    small = HipEngine(s.path, dtype="fp16", max_items=s.n - 1, warm_up=False)    # n > max_items
    c = next(c for c in E.CASES if c.id == "stem1_H24_fp16")                     # fused, but the first stem form: no crop inside
    p24 = str(tmp_path / "stem1_H24.aicw")
    E.ef.write_engine(p24, E.build_graph(c).g)
    first = HipEngine(p24, dtype="fp16", max_items=s.n, warm_up=False)
    try:
        refused(f32, s.frames, s.boxes, s.fo)
        refused(small, s.frames, s.boxes, s.fo)
        refused(first, s.frames, s.boxes, s.fo)
        refused(s.eng, s.frames, s.boxes, np.full(s.n, -1, np.int32))
        refused(s.eng, s.frames, s.boxes, s.fo, byte_offset=-1)
    finally:
        for e in (f32, small, first):
            e.close()
    emb, valid = s.eng.embed_bank_np(s.frames, s.boxes, s.fo)                     # the engine's launch state was reset: it goes on working
    assert valid.tolist() == s.valid.tolist() and np.array_equal(emb, s.emb)
    assert np.array_equal(s.eng.reid_infer_np(s.crops), s.emb)
