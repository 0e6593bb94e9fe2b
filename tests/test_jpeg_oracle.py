"""tests/jpeg_oracle.py, the JPEG stage's specification, checked on its own: the known answers of the format's
text, the header marker by marker, the tables, that the cases of tests/jpeg_cases.py reach the parts of the format they are there for,
and -- where Pillow imports -- that an independent decoder reads every file and finds the quality of its own encoder in them."""
import hashlib
import io
import struct

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_oracle as O

KNOWN = ((16, 16, 85, 0, 420, 737, "704bf57189ace3d3"), (8, 8, 85, 0, 444, 652, "8ead36301e02481f"), (17, 33, 50, 0, 420, 861, "d2c4cecb8403b17c"),
         (17, 33, 50, 2, 444, 919, "89a6e8e07f50483d"), (40, 56, 100, 3, 420, 4756, "c1d4eb064c057cfb"), (40, 56, 1, 1, 444, 871, "9bc48487ec53b466"))
CASES = {c.name: c for c in JC.cases()}


@pytest.mark.parametrize("h,w,q,r,sub,size,sha", KNOWN)
def test_known_answers(h, w, q, r, sub, size, sha):
    data = O.encode(O.known_answer_image(h, w), q, r, sub)
    assert len(data) == size and hashlib.sha256(data).hexdigest()[:16] == sha


def segments(data):
    """[(marker, payload)] of the segments before the entropy data, and the offset behind them."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xFF
        marker, (n,) = data[at + 1], struct.unpack(">H", data[at + 2:at + 4])
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out, at


@pytest.mark.parametrize("h,w,q,r,sub", ((16, 16, 85, 0, 420), (17, 33, 50, 2, 444), (720, 1280, 100, 0, 420), (1, 1, 1, 65535, 444), (16384, 16384, 75, 7, 420)))
def test_header_is_629_bytes_and_parses(h, w, q, r, sub):
    hdr = O.header(h, w, q, r, sub)
    seg, end = segments(hdr)
    assert len(hdr) == end == O.HEADER_BYTES == 629
    assert [m for m, _ in seg] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert seg[0][1] == b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    ql, qc = O.tables(q)
    assert seg[1][1] == bytes([0]) + bytes(ql[O.ZIGZAG].tolist()) and seg[2][1] == bytes([1]) + bytes(qc[O.ZIGZAG].tolist())
    assert seg[3][1] == bytes([8]) + struct.pack(">HH", h, w) + bytes([3, 1, 0x22 if sub == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for (m, p), cls_id, (counts, symbols) in zip(seg[4:8], (0x00, 0x10, 0x01, 0x11), O.HUFF_SPECS):
        assert p == bytes([cls_id]) + bytes(counts) + bytes(symbols) and sum(counts) == len(symbols)
    assert struct.unpack(">H", seg[8][1])[0] == O.geometry(h, w, r, sub)["ri"] == (r or -(-w // (16 if sub == 420 else 8)))
    assert seg[9][1] == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def test_tables():
    # libjpeg's scaling of the Annex K tables: spot values worked by hand, the clamps, and the monotony in between
    expect = {1: (255, 255, 255, 255), 25: (32, 22, 198, 34), 50: (16, 11, 99, 17), 75: (8, 6, 50, 9), 100: (1, 1, 1, 1)}
    for q, (l0, l1, l63, c0) in expect.items():
        ql, qc = O.tables(q)
        assert ql.dtype == np.uint8 and ql.shape == qc.shape == (64,)
        assert (int(ql[0]), int(ql[1]), int(ql[63]), int(qc[0])) == (l0, l1, l63, c0), q
    assert np.array_equal(O.tables(50)[0], O.BASE_LUMA) and np.array_equal(O.tables(50)[1], O.BASE_CHROMA)
    prev = O.tables(1)
    for q in range(2, 101):
        cur = O.tables(q)
        assert all((c <= p).all() and c.min() >= 1 for c, p in zip(cur, prev))
        prev = cur
    for bad in (0, 101, -1):
        with pytest.raises(ValueError):
            O.tables(bad)


def stats(c):
    """What a case's coefficients make the entropy coder do."""
    coef = O.coefficients(c.image, c.quality, c.subsampling).astype(np.int32)
    g = O.geometry(*c.image.shape[:2], c.restart, c.subsampling)
    dc_cat = ac_cat = zrl = 0
    for i in range(g["intervals"]):
        part = coef[i * g["ri"]:(i + 1) * g["ri"]]
        comps = [part[:, :-2].reshape(-1, 64), part[:, -2], part[:, -1]]
        for blocks in comps:
            diffs = np.diff(np.concatenate([[0], blocks[:, 0]]))
            dc_cat = max(dc_cat, max(O.category(d) for d in diffs))
        for b in part.reshape(-1, 64):
            nz = np.nonzero(b[1:])[0] + 1
            ac_cat = max(ac_cat, max((O.category(v) for v in b[nz]), default=0))
            zrl += int(((np.diff(np.concatenate([[0], nz])) - 1) // 16).sum())
    data = O.encode(c.image, c.quality, c.restart, c.subsampling)[O.HEADER_BYTES:-2]
    return dict(dc_cat=dc_cat, ac_cat=ac_cat, zrl=zrl, no_eob=int((coef.reshape(-1, 64)[:, 63] != 0).sum()), stuffed=data.count(b"\xff\x00"),
                rst=[data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7], max_q=int(max(t.max() for t in O.tables(c.quality))),
                dc_only=bool((coef.reshape(-1, 64)[:, 1:] == 0).all()), blocks=coef.shape[0] * coef.shape[1], bytes=len(data))


def test_cases_reach_what_they_are_there_for():
    s = stats(CASES["noise-q100-r0-444"])
    assert s["stuffed"] > 0 and s["no_eob"] > 0
    s = stats(CASES["noise-q1-r0-420"])
    assert s["max_q"] == 255
    assert stats(CASES["block_checkerboard-q100-r0-444"])["dc_cat"] == 11
    s = stats(CASES["pixel_checkerboard-q100-r0-444"])
    assert s["ac_cat"] == 10 and s["stuffed"] > 0
    for name in ("one_high_frequency-q50-r0-444", "one_high_frequency-q50-r0-420"):    # a run of 62 zeros: ZRL three times per luma block
        s = stats(CASES[name])
        assert s["zrl"] == 3 * 4 and s["no_eob"] == 4, (name, s)
    s = stats(CASES["one_high_frequency-q100-r0-444"])                        # (at q100 the pixels' rounding adds a few +-1: shorter runs)
    assert s["no_eob"] == 4 and s["ac_cat"] == 9
    for sub in (420, 444):
        s = stats(CASES[f"flat-q85-r0-{sub}"])
        assert s["dc_only"] and s["dc_cat"] == 0
        assert stats(CASES[f"tall-q85-r0-{sub}"])["rst"] == [0xD0 + (i & 7) for i in range(9 if sub == 420 else 19)]
    assert len(stats(CASES["tall-q85-r3-420"])["rst"]) == 3 and len(stats(CASES["tall-q85-r1-444"])["rst"]) == 39
    assert stats(CASES["tall-q85-r65535-444"])["rst"] == []
    for sub in (420, 444):                                                    # one interval far longer than any LDS tile
        s = stats(CASES[f"chunk_walk-q100-r65535-{sub}"])
        assert s["rst"] == [] and s["bytes"] > 4 * 16384 and s["blocks"] > 256
    # every case stays inside the categories the standard tables have codes for (the encoder asserts it while coding)
    assert all(len(JC.expected(name)) > O.HEADER_BYTES + 2 for name in CASES)


def test_worst_case_and_default_sizes():
    assert O.worst_case_bytes(16, 16, 0, 444) == 629 + 416 * 12 + 2 * 2 + 2 and O.default_max_bytes(17, 33, 0, 420) == 629 + 3 * 32 * 48 + 2 * 2 + 2
    for name, c in CASES.items():
        assert len(JC.expected(name)) <= O.worst_case_bytes(*c.image.shape[:2], c.restart, c.subsampling), name


# ---- an independent decoder ------------------------------------------------------------------------------------------------------------

def decode(data):
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(data))
    im.load()
    return im


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def test_every_case_decodes_with_the_right_size_and_tables():
    pytest.importorskip("PIL")
    for name, c in CASES.items():
        im = decode(JC.expected(name))
        h, w = c.image.shape[:2]
        assert im.size == (w, h) and im.mode == "RGB", name
        ql, qc = O.tables(c.quality)
        got = im.quantization
        for want, key in ((ql, 0), (qc, 1)):
            t = list(got[key])
            assert t == want.tolist() or t == want[O.ZIGZAG].tolist(), (name, key)   # natural order, or zigzag in older Pillow releases


def test_checkerboard_and_flat_decode_nearly_losslessly():
    pytest.importorskip("PIL")
    for name in ("block_checkerboard-q100-r0-444", "block_checkerboard-q100-r0-420", "flat-q100-r0-444", "flat-q50-r0-420", "flat-q1-r0-420"):
        c = CASES[name]
        rgb = np.asarray(decode(JC.expected(name)))
        assert psnr(rgb, c.image[:, :, ::-1]) >= 60, name


@pytest.mark.parametrize("hw", ((128, 64), (136, 200)))
def test_quality_and_size_next_to_pillows_own_encoder(hw):
    Image = pytest.importorskip("PIL.Image")
    img = JC.scene(*hw, seed=9)
    rgb = np.ascontiguousarray(img[:, :, ::-1])
    for q in (50, 85, 95):
        for sub, pil_sub in ((420, 2), (444, 0)):
            mine = O.encode(img, q, 0, sub)
            buf = io.BytesIO()
            Image.fromarray(rgb).save(buf, "JPEG", quality=q, subsampling=pil_sub, optimize=False)
            theirs = buf.getvalue()
            p_mine, p_theirs = psnr(np.asarray(decode(mine)), rgb), psnr(np.asarray(decode(theirs)), rgb)
            print(hw, q, sub, "PSNR", round(p_mine, 3), round(p_theirs, 3), "bytes", len(mine), len(theirs), round(len(mine) / len(theirs), 3))
            assert p_mine >= p_theirs - 0.25, (q, sub, p_mine, p_theirs)
            assert len(mine) <= 1.10 * len(theirs), (q, sub, len(mine), len(theirs))
