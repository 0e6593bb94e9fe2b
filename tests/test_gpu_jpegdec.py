"""The JPEG decoding stage on the device (aic_jpegdec_*) against tests/jpegdec_oracle.py, byte for byte: every
well-formed case from host and device memory into host and device memory, mixed banks with refused files between good ones, invariance
under banking, launch cuts and call order, the round trip with the device encoder without a host copy of pixels, and the pipeline's
upload_jpeg.  Every corrupt stream in here went through the CPU build of the same decoder under the sanitizers first
(tests/test_jpegdec_host.py); none is meant to fault, each must come back as a status."""
import numpy as np
import pytest
import torch

import jpeg_oracle as E
import jpegdec_cases as K
import jpegdec_oracle as D
from conftest import ROOT, pkg

pytestmark = pytest.mark.gpu


def by_size(cases):
    out = {}
    for c in cases:
        out.setdefault(c[2], []).append(c)
    return out


def explain(J, dec, buf, off, k, got, want, coef):
    """Where image k first differs, and whether the coefficients already do."""
    at = int(np.flatnonzero(got.reshape(-1) != want.reshape(-1))[0])
    y, x, c = np.unravel_index(at, want.shape)
    dc = dec.coefficients(buf, off, k)
    return f"first differing byte {at} (y {y}, x {x}, channel {c}): {got.reshape(-1)[at]} for {want.reshape(-1)[at]}; coefficients " + (
        "equal: the IDCT or the colour stage" if np.array_equal(dc, coef) else "already differ: the entropy stage")


@pytest.mark.parametrize("variant", ["host-to-host", "device-to-host", "device+3-to-device+3"])
def test_every_well_formed_case_equals_the_oracle(gpu, variant):
    J, ref = pkg("jpegdec"), K.reference()
    for (h, w), cases in by_size(K.well_formed()).items():
        dec = J.JpegDecoder(h, w, max_images=len(cases))
        buf, off = J.pack([c[1] for c in cases])
        n, fb = len(cases), h * w * 3
        if variant == "host-to-host":
            bgr, st, rs = dec.decode_packed(buf, off)
        else:
            shift = 3 if "+3" in variant else 0
            d = torch.zeros(buf.size + shift, dtype=torch.uint8, device="cuda")
            d[shift:] = torch.from_numpy(buf.copy()).cuda()
            if shift:
                raw = torch.full((n * fb + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                out = raw[35:35 + n * fb].view(n, h, w, 3)                    # 32 canary bytes + 3: an odd address
                assert out.data_ptr() % 4 == 3
                res, st, rs = dec.decode_packed(d[shift:], off, out=out)
                torch.cuda.synchronize()
                assert res is out and (raw[:35] == 0xA5).all() and (raw[35 + n * fb:] == 0xA5).all(), "bytes outside the output were written"
                bgr = out.cpu().numpy()
            else:
                bgr, st, rs = dec.decode_packed(d, off)
        assert not st.any() and not rs.any(), [(cases[k][0], D.REASONS[rs[k]]) for k in np.flatnonzero(st)]
        for k, c in enumerate(cases):
            want = ref[c[0]][0]
            assert np.array_equal(bgr[k], want), (c[0], explain(J, dec, buf, off, k, bgr[k], want, ref[c[0]][2]))
        for k in (0, n - 1):
            assert np.array_equal(dec.coefficients(buf, off, k), ref[cases[k][0]][2]), cases[k][0]
        assert dec.counters()["images"] == n and dec.counters()["bytes_out"] == n * fb and dec.counters()["bytes_in"] == buf.size
        dec.close()


def test_one_call_mixes_samplings_table_sets_restart_intervals_and_gray(gpu):
    J, ref = pkg("jpegdec"), K.reference()
    cases = [c for c in K.well_formed() if c[2] == (17, 33)]
    info = [ref[c[0]][1] for c in cases]
    assert {i["sampling"] for i in info} >= {400, 444, 422, 420} and len({i["restart"] for i in info}) >= 3
    dec = J.JpegDecoder(17, 33, max_images=len(cases))
    bank, st, rs = dec.decode([c[1] for c in cases])
    assert not st.any()
    for k, c in enumerate(cases):                                             # a bank equals single-image calls
        one, s1, _ = dec.decode([c[1]])
        assert not s1.any() and np.array_equal(one[0], bank[k]) and np.array_equal(bank[k], ref[c[0]][0]), c[0]
    dec.close()


def test_refused_images_between_good_ones(gpu):
    J = pkg("jpegdec")
    good = [c[1] for c in K.well_formed() if c[2] == (16, 16)]
    bad = [c[1] for c in K.refused()] + [c[1] for c in K.mutations()[:600] if c[2] == (16, 16)]
    want = [D.decode(f, (16, 16)) for f in bad]
    assert len({i["reason"] for _, i in want}) >= 12 and sum(b is not None for b, _ in want) >= 20       # some mutations still decode
    files, kinds = [], []
    for k, f in enumerate(bad):                                               # good, bad, good, bad ...
        files += [good[k % len(good)], f]
    dec = J.JpegDecoder(16, 16, max_images=len(files))
    buf, off = J.pack(files)
    out = torch.full((len(files), 16, 16, 3), 0x5A, dtype=torch.uint8, device="cuda")
    _, st, rs = dec.decode_packed(torch.from_numpy(buf.copy()).cuda(), off, out=out)
    got = out.cpu().numpy()
    clean, st0, _ = dec.decode(good)
    assert not st0.any()
    for k, (bgr, info) in enumerate(want):
        assert st[2 * k] == 0 and np.array_equal(got[2 * k], clean[k % len(good)]), k      # the neighbours: as in a call without the refused
        assert (st[2 * k + 1], rs[2 * k + 1]) == (info["status"], info["reason"]), (k, D.REASONS[rs[2 * k + 1]], D.REASONS[info["reason"]])
        if bgr is None:
            assert (got[2 * k + 1] == 0x5A).all(), (k, "a refused slot was written")
        else:
            assert np.array_equal(got[2 * k + 1], bgr), k
    host, st2, rs2 = dec.decode_packed(buf, off, out=np.full((len(files), 16, 16, 3), 0x5A, np.uint8))       # the same into host memory
    assert np.array_equal(host, got) and np.array_equal(st2, st) and np.array_equal(rs2, rs)
    c = dec.counters()
    assert c["images"] == 2 * len(files) + len(good) and c["refused"] == 2 * int((st != 0).sum())
    dec.close()


def test_launch_cuts_and_call_order_change_nothing(gpu):
    J, ref = pkg("jpegdec"), K.reference()
    cases = [c for c in K.well_formed() if c[2] == (48, 80)]
    files = [c[1] for c in cases] * 12                                        # about 2.5 MB of coefficients
    dec = J.JpegDecoder(48, 80, max_images=len(files))
    whole, st, _ = dec.decode(files)
    assert not st.any() and all(np.array_equal(whole[k], ref[cases[k % len(cases)][0]][0]) for k in range(len(files)))
    dec.option("launch_budget_mb", 1)                                         # several launches
    cut, st, _ = dec.decode(files)
    assert not st.any() and np.array_equal(cut, whole)
    other, st, _ = dec.decode([E.encode(K.image("primaries", 48, 80), 30, 2, 444)] * 3)       # other tables on the same handle
    assert not st.any() and np.array_equal(other[0], D.decode(E.encode(K.image("primaries", 48, 80), 30, 2, 444))[0])
    again, st, _ = dec.decode(files[:len(cases)])
    assert not st.any() and np.array_equal(again, whole[:len(cases)])
    dec.close()


@pytest.mark.parametrize("sub", ["420", "444"])
def test_round_trip_with_the_device_encoder_stays_on_the_device(gpu, sub):
    J, Enc = pkg("jpegdec"), pkg("jpeg").JpegEncoder
    frames = np.stack([K.image(kind, 48, 80, 4) for kind in ("noise", "primaries", "smooth")])
    enc, dec = Enc((48, 80), max_images=3, quality=85, restart=2, subsampling=sub), J.JpegDecoder(48, 80, max_images=3)
    d_frames = torch.from_numpy(frames).cuda()
    d_files = torch.zeros(3 * enc.worst_case_bytes(), dtype=torch.uint8, device="cuda")
    _, off, st = enc.encode_packed(d_frames, device_frames=True, out=d_files)
    assert not st.any()
    d_out = torch.zeros((3, 48, 80, 3), dtype=torch.uint8, device="cuda")
    _, st, rs = dec.decode_packed(d_files, off, out=d_out)                    # offset-addressed inside the larger buffer
    assert not st.any()
    want = [E.encode(f, 85, 2, int(sub)) for f in frames]
    assert d_files[:int(off[-1])].cpu().numpy().tobytes() == b"".join(want)
    got = d_out.cpu().numpy()
    for k in range(3):
        assert np.array_equal(got[k], D.decode(want[k], (48, 80))[0]), k
    enc.close(), dec.close()


@pytest.fixture(scope="module")
def clip():
    """8 synthetic 360 x 640 frames as quality-10 files (few symbols: the oracle decodes them in about two seconds) and the oracle's pixels."""
    syn = pkg("synthetic")
    sc = syn.Scene(seed=5, n_targets=4, width=640, height=360, w_range=(30.0, 60.0), h_range=(90.0, 150.0), y_range=(30.0, 200.0))
    frames = sc.render_batch(0, 8)
    files = [E.encode(f, 10, 0, 420) for f in frames]
    return sc, files, np.stack([D.decode(f, (360, 640))[0] for f in files])


@pytest.mark.parametrize("inject", [True, False])
def test_pipeline_upload_jpeg_equals_upload_of_the_decoded_frames(gpu, engines, clip, inject):
    sc, files, decoded = clip
    TP = pkg("pipeline").TrackingPipeline
    kw = dict(batch=8, ring_frames=8, max_persons=16, dtype="fp16", inject=inject)
    a, b = TP(engines[0], engines[1], (360, 640), **kw), TP(engines[0], engines[1], (360, 640), **kw)
    st, rs = a.upload_jpeg(0, files)
    assert not st.any() and not rs.any()
    assert np.array_equal(a.read_frames(0, 8), decoded)
    b.upload(0, decoded)
    if inject:
        planted = [sc.detections(f)[:3] for f in range(8)]
        a.inject(0, planted), b.inject(0, planted)
    ta, da = a.run(0, 8, want_dets=True)
    tb, db = b.run(0, 8, want_dets=True)
    assert ta == tb
    if inject:
        assert any(len(t) for t in tb)
    for x, y in zip(da, db):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))
    # a refused file leaves its slot's earlier contents, the neighbours are replaced
    torn = [files[1], files[0][:-1], files[2]]
    st, rs = a.upload_jpeg(3, torn)
    assert st.tolist() == [0, pkg("_lib").ERR_FORMAT, 0] and rs.tolist() == [0, D.TRUNCATED, 0]
    now = a.read_frames(3, 3)
    assert np.array_equal(now[0], decoded[1]) and np.array_equal(now[1], decoded[4]) and np.array_equal(now[2], decoded[2])
    tracks, dets, st, rs = b.run_from_jpeg(files[:4], slot=4)                 # upload_jpeg, then run
    assert not st.any() and len(tracks) == 4 and np.array_equal(b.read_frames(4, 4), decoded[:4])


def test_cli_reads_back_the_motion_jpeg_it_wrote(gpu, tmp_path, monkeypatch, capsys):
    ypath, _ = pkg("engine_file").ensure_seeded_engines(ROOT)
    cli, J = pkg("cli"), pkg("jpegdec")
    monkeypatch.setattr(cli, "probe_cv2", lambda: None)                       # headerless frames out, whatever is installed
    H, W, T = 112, 192, 4
    tail = ["--yolo_engine", ypath, "--tracker", "bytetrack", "--output_filename", "out"]
    assert cli.main(["--input", f"synthetic:{W}x{H}:2:{T}:1", "--output_dir", str(tmp_path / "a"), "--output_codec", "mjpeg", "--jpeg_restart", "5"] + tail) == 0
    clip = tmp_path / "a" / "out.mjpeg"
    buf, off = J.split_mjpeg(clip)
    assert off.size == T + 1
    files = [buf[off[k]:off[k + 1]].tobytes() for k in range(T)]
    decoded = np.stack([D.decode(f, (H, W))[0] for f in files])
    (tmp_path / "npy").mkdir()
    np.save(tmp_path / "npy" / "out.npy", decoded)                             # the same stem: the info panel prints the source's name
    for argv, name, stems in ((["--input", "{}"], "one", ["out"]), (["--inputs", "{},{}", "--batch", "2"], "two", ["out_s0", "out_s1"])):
        for src, where in ((str(clip), "mjpeg"), (str(tmp_path / "npy" / "out.npy"), "npy")):
            assert cli.main([a.format(src, src) for a in argv] + ["--output_dir", str(tmp_path / name / where)] + tail) == 0
        got, want = ([p.read_text() for p in sorted((tmp_path / name / where).glob("*.jsonl"))] for where in ("mjpeg", "npy"))
        assert len(got) == len(stems) and all(g.count("\n") == T for g in got) and got == want, name      # the same tracks line by line
        for stem in stems:                                                    # decoded on the device = the oracle's frames through the same run
            got, want = ((tmp_path / name / where / (stem + ".bgr24")).read_bytes() for where in ("mjpeg", "npy"))
            assert len(got) == len(want) == T * H * W * 3
            if name == "two":                                                 # (one source: the frames carry the run's measured FPS as text)
                assert got == want, (name, stem)
    # the round trip: --input clip.mjpeg --output_codec mjpeg
    assert cli.main(["--input", str(clip), "--output_dir", str(tmp_path / "b"), "--output_codec", "mjpeg"] + tail) == 0
    assert J.split_mjpeg(tmp_path / "b" / "out.mjpeg")[1].size == T + 1
    # a refused frame: one line with the reason, the previous frame in its place
    k = files[1].index(b"\xff\xd0", 629)
    torn = [files[0], files[1][:k] + files[1][k + 2:], files[2]]
    (tmp_path / "torn.mjpeg").write_bytes(b"".join(torn))
    capsys.readouterr()
    assert cli.main(["--input", str(tmp_path / "torn.mjpeg"), "--output_dir", str(tmp_path / "c"), "--no_save"] + tail) == 0
    assert "frame 1 refused (RESTART_SEQUENCE)" in capsys.readouterr().out
    name, frames, size = cli.frame_source(str(tmp_path / "torn.mjpeg"))
    frames = list(frames)
    assert size[:2] == (W, H) and len(frames) == 3 and np.array_equal(frames[1], decoded[0]) and np.array_equal(frames[2], decoded[2])
