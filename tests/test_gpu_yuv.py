"""NV12 / I420 <-> BGR24 on the device (aic_frames_to_bgr / aic_frames_from_bgr, the pipeline's unpack stage) against
tests/yuv_oracle.py: every comparison is np.array_equal.  Small frames walk every access path of kernels_yuv.hip (one block, strips with
a ragged tail, exact multiples of the strip; 8-byte, 4-byte and byte accesses), both memories and pitched layouts; a 512x512 frame carries
every (U, V) pair; the pipeline is checked at the ring and at its outputs."""
import numpy as np
import pytest
import torch            # (before libaicam.so is loaded, as in the other GPU suites: device tensors and the library share one HIP runtime)

import yuv_oracle as Y
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu

SIZES = ((2, 2), (2, 6), (4, 8), (6, 10), (2, 16), (4, 18), (8, 24), (6, 40), (16, 64), (10, 72))
FORMATS = ((Y.NV12, "nv12"), (Y.I420, "i420"))


def pitches(w):
    return (w, w + 2, (w + 63) // 64 * 64, w + 6)


def layouts(fmt, h, w):
    """(pitch, frame_stride, n) of the issue's grid: four pitches x n in {1, 3} x a tight and a padded frame_stride."""
    for pitch in pitches(w):
        for n in (1, 3):
            for pad in (0, 40):
                yield pitch, (pitch * h * 3 // 2 + pad if pad else 0), n


def dev_buffer(host, offset):
    """host bytes on the device, `offset` bytes past an allocation's base: (owner, view, address)."""
    buf = torch.zeros(host.size + 16, dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + host.size]
    view.copy_(torch.from_numpy(host.reshape(-1)))
    torch.cuda.synchronize()                                   # the conversions run on the library's own stream
    assert view.data_ptr() == buf.data_ptr() + offset and buf.data_ptr() % 256 == 0
    return buf, view, view.data_ptr()


@pytest.mark.parametrize("fmt,name", FORMATS)
def test_decode_equals_the_oracle_on_every_path(gpu, fmt, name):
    L = pkg("_lib")
    rng = np.random.default_rng(fmt)
    cases = 0
    for h, w in SIZES:
        for pitch, stride, n in layouts(fmt, h, w):
            src = rng.integers(0, 256, Y.buffer_bytes(fmt, n, h, w, pitch, stride), dtype=np.uint8)
            for matrix, rg in Y.SETS:
                want = Y.decode(src, fmt, (h, w), pitch, stride, matrix, rg, n=n)
                got = np.zeros_like(want)
                L.call("aic_frames_to_bgr", 0, L.ptr(src), n, h, w, fmt, pitch, stride, matrix, rg, L.HOST, L.ptr(got))
                assert np.array_equal(got, want), (name, "host", h, w, pitch, stride, n, matrix, rg)
                # device memory: aligned bases, the BGR destination 4 bytes past an allocation base, the YUV source 2 bytes past one
                for so, do in ((0, 0), (0, 4), (2, 0)):
                    _, _, sp = dev_buffer(src, so)
                    _, dv, dp = dev_buffer(np.zeros(want.size, np.uint8), do)
                    L.call("aic_frames_to_bgr", 0, L.ptr(sp), n, h, w, fmt, pitch, stride, matrix, rg, L.DEVICE, L.ptr(dp))
                    assert np.array_equal(dv.cpu().numpy().reshape(want.shape), want), (name, "device", so, do, h, w, pitch, stride, n, matrix, rg)
                cases += 1
    assert cases == len(SIZES) * 4 * 2 * 2 * 4


@pytest.mark.parametrize("fmt,name", FORMATS)
def test_encode_equals_the_oracle_and_leaves_the_padding(gpu, fmt, name):
    L = pkg("_lib")
    rng = np.random.default_rng(10 + fmt)
    for h, w in SIZES:
        for pitch, stride, n in layouts(fmt, h, w):
            bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
            fill = np.full(Y.buffer_bytes(fmt, n, h, w, pitch, stride), 0xA5, np.uint8)
            for matrix, rg in Y.SETS:
                want = Y.encode(bgr, fmt, pitch, stride, matrix, rg, out=fill.copy())
                assert pitch == w or (want == 0xA5).sum() >= n * h * (pitch - w)          # (the padding is there to be left alone)
                got = fill.copy()
                L.call("aic_frames_from_bgr", 0, L.ptr(bgr), n, h, w, fmt, pitch, stride, matrix, rg, L.HOST, L.ptr(got))
                assert np.array_equal(got, want), (name, "host", h, w, pitch, stride, n, matrix, rg)
                for so, do in ((0, 0), (4, 0), (0, 2)):
                    _, _, sp = dev_buffer(bgr, so)
                    _, dv, dp = dev_buffer(fill, do)
                    L.call("aic_frames_from_bgr", 0, L.ptr(sp), n, h, w, fmt, pitch, stride, matrix, rg, L.DEVICE, L.ptr(dp))
                    assert np.array_equal(dv.cpu().numpy(), want), (name, "device", so, do, h, w, pitch, stride, n, matrix, rg)


def test_python_wrappers_round_trip_the_oracle(gpu):
    F = pkg("frames")
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (3, 6, 40, 3), dtype=np.uint8)
    for fmt, name in FORMATS:
        for m, mn in ((Y.BT601, "bt601"), (Y.BT709, "bt709")):
            for r, rn in ((Y.LIMITED, "limited"), (Y.FULL, "full")):
                yuv = F.from_bgr(bgr, name, matrix=mn, range=rn)
                assert yuv.shape == (3, 9, 40) and np.array_equal(yuv, Y.encode(bgr, fmt, matrix=m, rng=r))
                assert np.array_equal(F.to_bgr(yuv, name, matrix=mn, range=rn), Y.decode(yuv, fmt, matrix=m, rng=r))
        out = np.full(Y.buffer_bytes(fmt, 3, 6, 40, 64, 700), 0xA5, np.uint8)
        assert F.from_bgr(bgr, name, pitch=64, frame_stride=700, out=out) is out
        assert np.array_equal(out, Y.encode(bgr, fmt, 64, 700, out=np.full(out.size, 0xA5, np.uint8)))
        assert np.array_equal(F.to_bgr(out, name, hw=(6, 40), pitch=64, frame_stride=700), Y.decode(out, fmt, (6, 40), 64, 700, n=3))
    assert np.array_equal(F.to_bgr(yuv[0], "i420"), Y.decode(yuv[:1], Y.I420))                  # one frame [H*3/2, W]


@pytest.fixture(scope="module")
def uv_frames():
    """[7, 768, 512] planes as NV12 of 512x512 frames whose 256x256 blocks carry every (U, V) pair: frame 0 with seeded random lumas, then
    all lumas forced to 0, 15, 16, 235, 236 and 255."""
    rng = np.random.default_rng(33)
    u, v = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    fr = np.empty((7, 768, 512), np.uint8)
    fr[0, :512] = rng.integers(0, 256, (512, 512), dtype=np.uint8)
    for i, level in enumerate((0, 15, 16, 235, 236, 255)):
        fr[1 + i, :512] = level
    fr[:, 512:, 0::2], fr[:, 512:, 1::2] = u, v
    return fr


@pytest.mark.parametrize("matrix,rg", Y.SETS)
def test_decode_covers_every_chroma_pair(gpu, uv_frames, matrix, rg):
    F = pkg("frames")
    mn, rn = ("bt601", "bt709")[matrix], ("limited", "full")[rg]
    want = Y.decode(uv_frames, Y.NV12, matrix=matrix, rng=rg)
    assert np.array_equal(F.to_bgr(uv_frames, "nv12", matrix=mn, range=rn), want)
    # the same samples as I420: de-interleave the chroma rows into a U plane and a V plane
    i420 = uv_frames.copy()
    i420[:, 512:] = np.concatenate([uv_frames[:, 512:, 0::2].reshape(7, 128, 512), uv_frames[:, 512:, 1::2].reshape(7, 128, 512)], 1)
    assert np.array_equal(F.to_bgr(i420, "i420", matrix=mn, range=rn), want)


# ------------------------------------------------------------------------------------------------------------------ the pipeline
N_CLIP = 12


@pytest.fixture(scope="module")
def clip():
    """12 frames of a synthetic scene at 720p: (nv12 [12, 1080, 1280] from the oracle's encoder, what the oracle decodes them to)."""
    sc = pkg("synthetic").Scene(seed=11, n_targets=12)
    yuv = Y.encode(sc.render_batch(0, N_CLIP), Y.NV12)
    return yuv, Y.decode(yuv, Y.NV12)


def _pipe(tracker, ring, batch, **kw):
    ef = pkg("engine_file")
    ypath, rpath = ef.ensure_trained_detector(ROOT), ef.ensure_seeded_engines(ROOT)[1]
    return pkg("pipeline").TrackingPipeline(ypath, None if tracker == "bytetrack" else rpath, (720, 1280), batch=batch, ring_frames=ring, max_persons=32,
                                            dtype="fp16", tracker=tracker, **kw)


def test_pipeline_ring_holds_the_oracles_decode(gpu, clip):
    yuv, bgr = clip
    pipe = _pipe("bytetrack", 6, 2, pixel_format="nv12")
    assert pipe.host_frame_shape == (1080, 1280)
    pipe.upload(0, yuv[:6])
    assert np.array_equal(pipe.read_frames(0, 6), bgr[:6])
    pipe.upload(4, yuv[7])                                     # one frame into a later slot; the others stay
    got = pipe.read_frames(3, 3)
    assert np.array_equal(got[0], bgr[3]) and np.array_equal(got[1], bgr[7]) and np.array_equal(got[2], bgr[5])
    # I420, then BT.709 full range, on the same pipeline between calls
    i420 = Y.encode(bgr[:6], Y.I420)
    pipe.set_pixel_format("i420")
    pipe.upload(0, i420)
    assert np.array_equal(pipe.read_frames(0, 6), Y.decode(i420, Y.I420))
    full = Y.encode(bgr[:6], Y.NV12, matrix=Y.BT709, rng=Y.FULL)
    pipe.set_pixel_format("nv12", "bt709", "full")
    pipe.upload(0, full)
    assert np.array_equal(pipe.read_frames(0, 6), Y.decode(full, Y.NV12, matrix=Y.BT709, rng=Y.FULL))
    # back to BGR: the ring takes the bytes as they come
    pipe.set_pixel_format("bgr24")
    pipe.upload(0, bgr[6:12])
    assert np.array_equal(pipe.read_frames(0, 6), bgr[6:12])
    L = pkg("_lib")
    for slot, count in ((-1, 1), (5, 2), (0, -1)):
        assert L.load().aic_pipeline_read_frames(pipe._h, slot, count, L.ptr(got)) == L.ERR_INVALID
    pipe.close()


@pytest.mark.parametrize("tracker", ("deepsort", "bytetrack"))
def test_pipeline_outputs_equal_the_bgr_pipelines(gpu, clip, tracker):
    """run_raw_from_host_passes over 12 NV12 frames, batch 4, ring 12, two passes (every ring and staging slot is reused under the unpack):
    n_tracks, rows and n_dets equal those of a BGR pipeline fed the oracle's decode of the same frames."""
    yuv, bgr = clip
    ref = _pipe(tracker, N_CLIP, 4)
    want = [x.copy() for x in ref.run_raw_from_host_passes(bgr, 2)]
    ref.close()
    assert want[2].sum() > 0 and want[0].sum() > 0                                    # the detector sees the scene, tracks are confirmed
    pipe = _pipe(tracker, N_CLIP, 4, pixel_format="nv12")
    got = pipe.run_raw_from_host_passes(yuv, 2)
    for g, w, what in zip(got, want, ("n_tracks", "rows", "n_dets")):
        assert np.array_equal(g, w), (tracker, what)
    assert np.array_equal(pipe.read_frames(0, N_CLIP), bgr)
    pipe.close()
    # a pipeline that took YUV first and is switched back to BGR between calls gives the BGR result
    pipe = _pipe(tracker, N_CLIP, 4, pixel_format="nv12")
    pipe.upload(0, yuv)
    pipe.set_pixel_format("bgr24")
    got = pipe.run_raw_from_host_passes(bgr, 2)
    for g, w, what in zip(got, want, ("n_tracks", "rows", "n_dets")):
        assert np.array_equal(g, w), (tracker, "switched back", what)
    pipe.close()


def test_pipeline_rejects_before_anything_changes(gpu):
    L = pkg("_lib")
    ef = pkg("engine_file")
    ypath = ef.ensure_seeded_engines(ROOT)[0]
    odd = pkg("pipeline").TrackingPipeline(ypath, None, (90, 161), batch=2, ring_frames=2, tracker="bytetrack")
    for v in (1, 2):
        assert L.load().aic_pipeline_option(odd._h, b"pixel_format", v) == L.ERR_INVALID and b"even" in L.load().aic_last_error()
    assert L.load().aic_pipeline_option(odd._h, b"pixel_format", 0) == L.OK
    for key, bad in ((b"pixel_format", (-1, 3)), (b"yuv_matrix", (-1, 2)), (b"yuv_range", (-1, 2))):
        for v in bad:
            assert L.load().aic_pipeline_option(odd._h, key, v) == L.ERR_INVALID, (key, v)
    odd.close()
    with pytest.raises(ValueError):
        pkg("pipeline").TrackingPipeline(ypath, None, (90, 160), batch=2, ring_frames=2, tracker="bytetrack", pixel_format="yuyv")
    pipe = pkg("pipeline").TrackingPipeline(ypath, None, (90, 160), batch=2, ring_frames=2, tracker="bytetrack", pixel_format="i420")
    with pytest.raises(AssertionError):
        pipe.upload(0, np.zeros((2, 90, 160, 3), np.uint8))                           # BGR-shaped frames for a YUV pipeline
    pipe.upload(0, np.zeros((2, 135, 160), np.uint8))
    pipe.close()


# ------------------------------------------------------------------------------------------------------------------ the CLI
def _cli(tmp_path, name, argv):
    import json
    out = tmp_path / name
    ypath = pkg("engine_file").ensure_trained_detector(ROOT)
    assert pkg("cli").main(argv + ["--tracker", "bytetrack", "--yolo_engine", ypath, "--output_dir", str(out)]) == 0
    files = sorted(out.iterdir())
    return ([[json.loads(l) for l in open(p)] for p in files if p.name.endswith(".jsonl")],
            [p for p in files if p.suffix in (".bgr24", ".nv12")])


def test_cli_takes_nv12_and_writes_nv12(gpu, clip, tmp_path):
    """Two raw: sources through one bank pipeline (--inputs, batch 4): fed NV12 and writing NV12, the tracks and the written pixels are those
    of the run fed the oracle's decode and writing BGR24 -- the drawn frames came back from the ring, the output went through from_bgr."""
    import json
    yuv, bgr = clip
    for d, data in (("yuv", yuv), ("bgr", bgr)):
        (tmp_path / d).mkdir()
        data[:4].tofile(tmp_path / d / "a.raw"), data[4:8].tofile(tmp_path / d / "b.raw")
    spec = lambda d: ",".join(f"raw:1280x720:{tmp_path / d / n}.raw" for n in "ab")       # noqa: E731
    lines_b, files_b = _cli(tmp_path, "out_bgr", ["--inputs", spec("bgr"), "--batch", "4"])
    lines_y, files_y = _cli(tmp_path, "out_yuv", ["--inputs", spec("yuv"), "--batch", "4", "--pixel_format", "nv12", "--output_pixel_format", "nv12"])
    assert lines_y == lines_b and len(lines_b) == 2 and all(len(l) == 4 for l in lines_b)
    assert sum(len(l["tracks"]) for ls in lines_b for l in ls) > 0
    assert [p.suffix for p in files_b] == [".bgr24"] * 2 and [p.suffix for p in files_y] == [".nv12"] * 2
    for pb, py in zip(files_b, files_y):
        drawn = np.fromfile(pb, np.uint8).reshape(4, 720, 1280, 3)
        assert np.array_equal(np.fromfile(py, np.uint8).reshape(4, 1080, 1280), Y.encode(drawn, Y.NV12))
        meta = json.load(open(str(py) + ".json"))
        assert (meta["pixel_format"], meta["yuv_matrix"], meta["yuv_range"], meta["frames"]) == ("nv12", "bt601", "limited", 4)
    # --batch 1: every frame goes through frames.to_bgr before the plugin classes; the tracks are the BGR run's
    one_b, _ = _cli(tmp_path, "one_bgr", ["--input", f"raw:1280x720:{tmp_path / 'bgr' / 'a.raw'}"])
    one_y, _ = _cli(tmp_path, "one_yuv", ["--input", f"raw:1280x720:{tmp_path / 'yuv' / 'a.raw'}", "--pixel_format", "nv12"])
    assert one_y == one_b and len(one_b[0]) == 4
