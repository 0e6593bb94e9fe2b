"""The files the JPEG decoding stage is tested on, built once per process: well-formed files from the project's own
encoder specification (tests/jpeg_oracle.py), from Pillow where it imports, and derived from those; refused files, each with the reason it
must carry; seeded single-byte and truncation mutations of three small files.  Every case is (name, file bytes, (height, width) asked
for); refused() adds the reason.  reference() holds the oracle's answer to every case, computed once."""
import functools
import io

import numpy as np

import jpeg_oracle as E
import jpegdec_oracle as D


def image(kind, h, w, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "blocks":                                                       # a checkerboard of 8 x 8 blocks
        return np.repeat(((((y >> 3) + (x >> 3)) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == "pixels":                                                       # a checkerboard of pixels
        return np.repeat((((y + x) & 1) * 255).astype(np.uint8)[:, :, None], 3, 2)
    if kind == "primaries":
        table = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
        return table[((x >> 2) + (y >> 2)) % 8]
    if kind == "flat":
        return np.full((h, w, 3), (40, 128, 200), np.uint8)
    if kind == "smooth":
        return E.known_answer_image(h, w)
    raise ValueError(kind)


SIZES = ((1, 1), (8, 8), (16, 16), (17, 33), (33, 17), (48, 80))
RESTARTS = (1, 3, 0, 65535)                                                    # 0 = one MCU row
QUALITIES = (1, 50, 100)
KINDS = ("noise", "blocks", "pixels", "primaries", "flat")


def segments(f):
    """[(marker, start, end)] of a file's segments up to and including SOS."""
    out, pos = [], 2
    while True:
        while f[pos + 1] == 0xFF:                                              # fill bytes
            pos += 1
        m, n = f[pos + 1], (f[pos + 2] << 8) | f[pos + 3]
        out.append((m, pos, pos + 2 + n))
        pos += 2 + n
        if m == 0xDA:
            return out


def cut(f, marker, which=None):
    """The file without its segments of one marker (which: only that occurrence)."""
    out, last, k = bytearray(), 0, 0
    for m, a, b in segments(f):
        if m == marker:
            if which is None or which == k:
                out += f[last:a]
                last = b
            k += 1
    return bytes(out + f[last:])


def sos_end(f):
    return segments(f)[-1][2]


def splice(f, marker, payload):
    """The file with a segment put in front of its first DQT."""
    a = next(s for s in segments(f) if s[0] == 0xDB)[1]
    n = len(payload) + 2
    return f[:a] + bytes([0xFF, marker, n >> 8, n & 255]) + payload + f[a:]


def planted():
    """One 8 x 8 4:4:4 picture whose luma block holds +-1023 in every coefficient under Q = 255: the IDCT's int32 wraps."""
    c = np.zeros((1, 3, 64), np.int16)
    c[0, 0] = np.where(np.arange(64) & 1, -1023, 1023)
    c[0, 1, :8] = 1023
    return E.header(8, 8, 1, 0, 444) + E.entropy(c, 1) + b"\xff\xd9"


def _pillow():
    try:
        from PIL import Image
        return Image
    except Exception:
        return None


@functools.lru_cache(None)
def well_formed():
    out, i = [], 0
    for h, w in SIZES:
        for sub in (420, 444):
            for _ in range(2):
                r, q, kind = RESTARTS[i % 4], QUALITIES[i % 3], KINDS[i % 5]
                out.append((f"enc-{h}x{w}-{sub}-r{r}-q{q}-{kind}", E.encode(image(kind, h, w, i), q, r, sub), (h, w)))
                i += 1
    for kind in KINDS:                                                         # every content at one size, both samplings
        for sub in (420, 444):
            out.append((f"enc-17x33-{sub}-{kind}", E.encode(image(kind, 17, 33, 7), 85, 0, sub), (17, 33)))
    out.append(("enc-tall-24x2048", E.encode(image("smooth", 2048, 24), 50, 1, 420), (2048, 24)))    # 256 intervals: m wraps 32 times
    Image = _pillow()
    if Image is not None:
        for h, w in ((17, 33), (48, 80)):
            rgb = image("noise", h, w, 3)[:, :, ::-1]
            for ss in (0, 1, 2):
                for kw in (dict(), dict(optimize=True), dict(restart_marker_rows=1), dict(restart_marker_blocks=2, optimize=True)):
                    b = io.BytesIO()
                    try:
                        Image.fromarray(rgb).save(b, "JPEG", quality=85, subsampling=ss, **kw)
                    except Exception:
                        continue                                              # this Pillow has no restart_marker_*
                    out.append((f"pil-{h}x{w}-ss{ss}-" + ("-".join(kw) or "plain"), b.getvalue(), (h, w)))
            b = io.BytesIO()
            Image.fromarray(rgb[:, :, 0]).save(b, "JPEG", quality=90)
            out.append((f"pil-{h}x{w}-gray", b.getvalue(), (h, w)))
    base = E.encode(image("noise", 17, 33, 11), 85, 1, 420)
    out.append(("no-dht", cut(base, 0xC4), (17, 33)))                          # Annex K by default
    f = splice(splice(base, 0xFE, b"a comment"), 0xE1, b"Exif\0\0" + bytes(40))
    a = next(s for s in segments(f) if s[0] == 0xC0)[1]
    f = f[:a] + b"\xff\xff\xff" + f[a:]                                        # fill bytes before SOF0
    k = f.index(b"\xff\xd1", sos_end(f))
    f = f[:k] + b"\xff\xff" + f[k:-2] + b"\xff" + f[-2:]                       # before RST1 and before EOI
    out.append(("com-app-fill", f, (17, 33)))
    out.append(("planted-1023-q255", planted(), (8, 8)))
    return tuple(out)


@functools.lru_cache(None)
def refused():
    R = D
    a = E.encode(image("noise", 16, 16, 5), 85, 1, 444)                        # 4 intervals
    e0 = sos_end(a)
    marks = [a.index(bytes([0xFF, 0xD0 + k]), e0) for k in range(3)]
    dri = next(s for s in segments(a) if s[0] == 0xDD)[1]
    sof = next(s for s in segments(a) if s[0] == 0xC0)[1]
    dqt = next(s for s in segments(a) if s[0] == 0xDB)[1]
    one = E.encode(image("noise", 16, 16, 6), 100, 65535, 444)                 # a single interval

    def patch(f, at, b):
        return f[:at] + bytes(b) + f[at + len(bytes(b)):]

    bits = E._Bits()
    bits.put(*E.CODES[0][0])
    for _ in range(4):                                                         # 15 zeros and a one, four times: the last run passes 63
        bits.put(*E.CODES[1][0xF1])
        bits.put_value(1, 1)
    out = [
        ("truncated-header", a[:10], (16, 16), R.TRUNCATED),
        ("truncated-table", a[:dqt + 30], (16, 16), R.TRUNCATED),
        ("truncated-interval", a[:(marks[0] + marks[1]) // 2], (16, 16), R.TRUNCATED),
        ("truncated-before-eoi", a[:-1], (16, 16), R.TRUNCATED),
        ("marker-dropped", a[:marks[1]] + a[marks[1] + 2:], (16, 16), R.RESTART_SEQUENCE),
        ("markers-swapped", patch(patch(a, marks[0] + 1, [0xD1]), marks[1] + 1, [0xD0]), (16, 16), R.RESTART_SEQUENCE),
        ("dri-disagrees", patch(a, dri + 4, [0, 2]), (16, 16), R.RESTART_SEQUENCE),
        ("no-code-matches", one[:e0] + b"\xff\x00\xff\x00\xff\x00" + one[-2:], (16, 16), R.BAD_CODE),
        ("run-past-63", E.header(8, 8, 50, 0, 444) + bits.stuffed() + b"\xff\xd9", (8, 8), R.BAD_CODE),
        ("overrun", one[:-12] + one[-2:], (16, 16), R.OVERRUN),
        ("other-size", a, (16, 24), R.SIZE_MISMATCH),
        ("progressive", patch(a, sof + 1, [0xC2]), (16, 16), R.NOT_BASELINE),
        ("arithmetic", patch(a, sof + 1, [0xC9]), (16, 16), R.NOT_BASELINE),
        ("twelve-bit", patch(a, sof + 4, [12]), (16, 16), R.PRECISION),
        ("cmyk", patch(a, sof + 9, [4]), (16, 16), R.COMPONENTS),
        ("adobe-rgb", splice(a, 0xEE, b"Adobe\0\x64\0\0\0\0\0"), (16, 16), R.COMPONENTS),
        ("sampling-4x1", patch(a, sof + 11, [0x41]), (16, 16), R.SAMPLING),
        ("dqt-16-bit", patch(a, dqt + 4, [0x10]), (16, 16), R.BAD_TABLE),
        ("dqt-missing", cut(a, 0xDB, 1), (16, 16), R.MISSING_TABLE),
        ("dht-missing", cut(a, 0xC4, 3), (16, 16), R.MISSING_TABLE),
        ("second-scan", a[:marks[0]] + b"\xff\xc4" + a[marks[0]:], (16, 16), R.BAD_SCAN),
        ("scan-before-frame", cut(a, 0xC0), (16, 16), R.BAD_SCAN),
        ("not-a-jpeg", b"GIF89a" + bytes(64), (16, 16), R.NOT_JPEG),
        ("empty", b"", (16, 16), R.NOT_JPEG),
    ]
    return tuple(out)


@functools.lru_cache(None)
def mutations(n=2000, seed=20):
    """n single-byte and truncation mutations of three small files: most are refused, some still decode -- the oracle says which."""
    files = [(E.encode(image("noise", 8, 8, 1), 85, 0, 444), (8, 8)), (E.encode(image("noise", 16, 16, 2), 50, 1, 420), (16, 16)),
             (E.encode(image("smooth", 16, 24, 3), 85, 2, 444), (16, 24))]
    rng, out = np.random.default_rng(seed), []
    for i in range(n):
        f, size = files[i % 3]
        if i % 4 == 3:
            m = f[:int(rng.integers(0, len(f)))]
        else:                                                                  # two in three land in the entropy data
            lo = sos_end(f) - 14 if (i // 3) % 3 else 0
            at = int(rng.integers(lo, len(f)))
            m = f[:at] + bytes([int(rng.integers(0, 256))]) + f[at + 1:]
        out.append((f"mut-{i}", m, size))
    return tuple(out)


@functools.lru_cache(None)
def reference():
    """{name: (bgr or None, info, coefficients or None)} of every well-formed and refused case, by the oracle."""
    out = {}
    for name, f, size, *_ in well_formed() + refused():
        bgr, info = D.decode(memoryview(f), size)
        out[name] = (bgr, info, D.coefficients(f, size) if bgr is not None else None)
    return out


def dump(path, cases):
    """The cases and the oracle's answers as the stand-alone probe reads them: per case int32 height, width, reason, file bytes,
    coefficient count; the file; the coefficients (int16)."""
    with open(path, "wb") as fh:
        fh.write(np.int32(len(cases)).tobytes())
        for name, f, size, *_ in cases:
            try:
                c, reason = D.coefficients(memoryview(f), size).reshape(-1), 0
            except D.Refused as e:
                c, reason = np.zeros(0, np.int16), e.reason
            fh.write(np.array([size[0], size[1], reason, len(f), c.size], np.int32).tobytes() + bytes(f) + c.astype(np.int16).tobytes())
