"""tests/jpegdec_oracle.py against what it specifies, on the CPU: its pixels equal libjpeg's (Pillow) on every
well-formed case of both encoders, its coefficients are the ones the encoder's specification wrote, every refusal carries its reason, and
the parse never reads outside the file."""
import io

import numpy as np
import pytest

import jpeg_oracle as E
import jpegdec_cases as K
import jpegdec_oracle as D


def test_pixels_equal_libjpeg_on_every_well_formed_case():
    Image = pytest.importorskip("PIL.Image")
    ref, seen = K.reference(), set()
    for name, f, size in K.well_formed():
        bgr, info, _ = ref[name]
        assert info["status"] == 0 and bgr.shape == (*size, 3) and bgr.dtype == np.uint8, (name, info)
        if name.startswith("planted"):
            continue                                                          # out-of-range values: held to the oracle only
        pil = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[:, :, ::-1]
        assert np.array_equal(bgr, pil), (name, int(np.abs(bgr.astype(int) - pil).max()), int((bgr != pil).sum()))
        seen.add(info["sampling"])
    assert seen == {400, 444, 422, 420}


def test_the_cases_cover_what_the_issue_lists():
    names = [c[0] for c in K.well_formed()]
    info = {n: K.reference()[n][1] for n in names}
    for h, w in K.SIZES:
        assert any(i["height"] == h and i["width"] == w and i["sampling"] == s for i in info.values() for s in (420,)), (h, w)
        assert any(i["height"] == h and i["width"] == w and i["sampling"] == 444 for i in info.values()), (h, w)
    assert {1, 3, 65535} <= {i["restart"] for i in info.values()} and any(i["intervals"] == 1 and i["restart"] == 65535 for i in info.values())
    assert info["enc-tall-24x2048"]["intervals"] == 256
    assert info["no-dht"]["status"] == 0 and b"\xff\xc4" not in K.well_formed()[names.index("no-dht")][1][:200]
    assert np.array_equal(K.reference()["no-dht"][0], D.decode(E.encode(K.image("noise", 17, 33, 11), 85, 1, 420))[0])
    base = D.decode(E.encode(K.image("noise", 17, 33, 11), 85, 1, 420))[0]
    assert np.array_equal(K.reference()["com-app-fill"][0], base)             # segments and fill bytes change nothing
    assert len(K.refused()) >= 20 and len({c[3] for c in K.refused()}) == 13  # every reason of the enum


def test_coefficients_are_the_encoders():
    for (h, w), sub, q, r in (((17, 33), 420, 85, 0), ((17, 33), 444, 50, 1), ((48, 80), 420, 100, 3), ((1, 1), 444, 1, 65535), ((16, 16), 420, 50, 65535)):
        img = K.image("noise", h, w, 9)
        c = D.coefficients(E.encode(img, q, r, sub), (h, w))
        assert c.dtype == np.int16 and np.array_equal(c[:, :, E.ZIGZAG], E.coefficients(img, q, sub)), (h, w, sub, q, r)


def test_planted_block_wraps_and_is_defined():
    bgr, info, c = K.reference()["planted-1023-q255"]
    assert info["status"] == 0 and np.abs(c[0, 0]).min() == 1023
    w = (c[0, 0].astype(np.int64) * 255).reshape(8, 8)                        # the same pass without wraparound gives other values: it did wrap
    with np.errstate(over="ignore"):
        exact, wrapped = D._idct_pass([w[k] for k in range(8)], 11), D._idct_pass([w[k].astype(np.int32) for k in range(8)], 11)
        rows_exact = D._idct_pass([np.stack(exact)[:, k] for k in range(8)], 18)
        rows_wrapped = D._idct_pass([np.stack(wrapped)[:, k] for k in range(8)], 18)
    assert not np.array_equal(np.stack(rows_exact), np.stack(rows_wrapped).astype(np.int64))
    assert np.array_equal(np.clip(np.stack(rows_wrapped, -1) + 128, 0, 255), D.idct(c[:1, :1], np.full(64, 255, np.int32))[0, 0])


class Fenced:
    """A read-only view of exactly the file: an index outside [0, len) raises, a negative one as well."""

    def __init__(self, data):
        self.data = bytes(data)

    def __len__(self):
        return len(self.data)

    def __getitem__(self, k):
        if isinstance(k, slice):
            assert (k.start is None or 0 <= k.start <= len(self.data)) and (k.stop is None or 0 <= k.stop <= len(self.data)), k
            return self.data[k]
        assert 0 <= k < len(self.data), k
        return self.data[k]


def test_every_refusal_carries_its_reason_and_the_parse_stays_inside_the_file():
    for name, f, size, reason in K.refused():
        bgr, info = D.decode(memoryview(f), size)
        assert bgr is None and info["status"] == D.ERR_FORMAT and info["reason"] == reason, (name, D.REASONS[info["reason"]], D.REASONS[reason])
    a = E.encode(K.image("noise", 17, 33, 2), 85, 1, 420)
    for cut in range(len(a)):                                                 # every proper prefix: a reason, never an index outside
        try:
            D.parse(Fenced(a[:cut]), None)
        except D.Refused as e:
            assert e.reason in (D.TRUNCATED, D.NOT_JPEG), (cut, e.reason)
        else:
            raise AssertionError(f"a file cut at {cut} was accepted")


def test_probe_reports_the_header():
    f = E.encode(K.image("smooth", 17, 33), 85, 0, 420)
    assert D.probe(f) == dict(status=0, reason=0, width=33, height=17, components=3, sampling=420, restart=3, intervals=2,
                              entropy_offset=E.HEADER_BYTES, entropy_bytes=len(f) - E.HEADER_BYTES - 2)
    assert D.probe(b"") == dict(status=D.ERR_FORMAT, reason=D.NOT_JPEG, width=0, height=0, components=0, sampling=0, restart=0, intervals=0,
                                entropy_offset=0, entropy_bytes=0)
