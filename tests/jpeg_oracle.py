"""The JPEG stage's specification (aic_jpeg_*) in NumPy and plain Python, integer arithmetic only: baseline
sequential DCT, 8 bit, YCbCr (JFIF, full range), 4:2:0 or 4:4:4, the Annex K Huffman tables, restart markers always on.  The device
encoder's bytes equal encode()'s; coefficients() exposes the quantised coefficients in the device's layout, so a difference can be
pinned to the transform or to the entropy coder.  No decoder and no imaging library in here."""
import numpy as np

HEADER_BYTES = 629

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
                   56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])   # natural index of zigzag position k

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32)

T = np.array([[1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448],
              [2009, 1703, 1138, 400, -400, -1138, -1703, -2009],
              [1892, 784, -784, -1892, -1892, -784, 784, 1892],
              [1703, -400, -2009, -1138, 1138, 2009, 400, -1703],
              [1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448],
              [1138, -2009, 400, 1703, -1703, -400, 2009, -1138],
              [784, -1892, 1892, -784, -784, 1892, -1892, 784],
              [400, -1138, 1703, -2009, 2009, -1703, 1138, -400]], np.int64)

# Annex K.3: (the 16 code counts by length, the symbols in code order) of DC luma, AC luma, DC chroma, AC chroma
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
            0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
HUFF_SPECS = (DC_LUMA, AC_LUMA, DC_CHROMA, AC_CHROMA)                       # in the file's order: DC0 AC0 DC1 AC1


def huffman_codes(spec):
    """{symbol: (code, length)} of a (counts, symbols) table, Annex C."""
    counts, symbols = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


CODES = [huffman_codes(s) for s in HUFF_SPECS]


def _sub(subsampling):
    s = int(subsampling)
    if s not in (420, 444):
        raise ValueError("subsampling must be 420 or 444")
    return s


def tables(quality):
    """(luma [64], chroma [64]) uint8 quantisation tables in natural order, libjpeg's quality scaling."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be in 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * s + 50) // 100, 1, 255).astype(np.uint8) for b in (BASE_LUMA, BASE_CHROMA))


def geometry(h, w, restart, subsampling):
    """dict(mcu, bpm, mcus_x, mcus_y, n_mcu, ri, intervals): MCU size, blocks per MCU, the MCU grid, MCUs per interval, intervals."""
    sub = _sub(subsampling)
    if not (1 <= h <= 16384 and 1 <= w <= 16384):
        raise ValueError("height and width must be in 1..16384")
    if not 0 <= int(restart) <= 65535:
        raise ValueError("restart must be in 0..65535")
    mcu = 16 if sub == 420 else 8
    mx, my = -(-w // mcu), -(-h // mcu)
    ri = int(restart) or mx
    return dict(mcu=mcu, bpm=6 if sub == 420 else 3, mcus_x=mx, mcus_y=my, n_mcu=mx * my, ri=ri, intervals=-(-(mx * my) // ri))


def default_max_bytes(h, w, restart=0, subsampling=420):
    g = geometry(h, w, restart, subsampling)
    return HEADER_BYTES + 3 * g["mcus_x"] * g["mcu"] * g["mcus_y"] * g["mcu"] + 2 * g["intervals"] + 2


def worst_case_bytes(h, w, restart=0, subsampling=420):
    g = geometry(h, w, restart, subsampling)
    return HEADER_BYTES + 416 * g["bpm"] * g["n_mcu"] + 2 * g["intervals"] + 2


def header(h, w, quality=85, restart=0, subsampling=420):
    """The 629 bytes before the entropy data."""
    sub, g = _sub(subsampling), geometry(h, w, restart, subsampling)
    out = bytearray(b"\xff\xd8")
    out += b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    for i, t in enumerate(tables(quality)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(t[ZIGZAG].tolist())
    out += b"\xff\xc0\x00\x11\x08" + bytes([h >> 8, h & 255, w >> 8, w & 255, 3, 1, 0x22 if sub == 420 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for cls_id, (counts, symbols) in zip((0x00, 0x10, 0x01, 0x11), HUFF_SPECS):
        n = 2 + 1 + 16 + len(symbols)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, cls_id]) + bytes(counts) + bytes(symbols)
    out += b"\xff\xdd\x00\x04" + bytes([g["ri"] >> 8, g["ri"] & 255])
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def ycbcr(bgr):
    """int32 planes Y, Cb, Cr of a [h, w, 3] BGR uint8 image."""
    p = np.asarray(bgr).astype(np.int32)
    b, g, r = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, mcu):
    h, w = plane.shape
    return np.pad(plane, ((0, -h % mcu), (0, -w % mcu)), mode="edge")


def _blocks(plane):
    """[by, bx, 8, 8] blocks of a plane whose sides are multiples of 8."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def fdct_quant(blocks, qtable):
    """Quantised coefficients [..., 64] in natural order (int32) of sample blocks [..., 8, 8]."""
    s = blocks.astype(np.int64) - 128
    a = (np.einsum("ux,...yx->...yu", T, s) + 256) >> 9
    f = (np.einsum("vy,...yu->...vu", T, a) + 2048) >> 12
    assert np.abs(a).max(initial=0) < 2 ** 31 and np.abs(f).max(initial=0) < 2 ** 31
    q = qtable.astype(np.int64).reshape(8, 8)
    c = np.sign(f) * ((np.abs(f) + 4 * q) // (8 * q))
    return c.reshape(*c.shape[:-2], 64).astype(np.int32)


def coefficients(bgr, quality=85, subsampling=420):
    """int16 [n_mcu, blocks per MCU, 64]: the quantised coefficients, zigzag order, MCU-interleaved (Y.. Cb Cr) -- the layout of the
    device's coefficient buffer."""
    sub = _sub(subsampling)
    bgr = np.asarray(bgr)
    if bgr.ndim != 3 or bgr.shape[2] != 3 or bgr.dtype != np.uint8:
        raise ValueError("bgr must be uint8 [h, w, 3]")
    ql, qc = tables(quality)
    mcu = 16 if sub == 420 else 8
    y, cb, cr = (_pad(p, mcu) for p in ycbcr(bgr))
    if sub == 420:
        cb, cr = ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2 for p in (cb, cr))
    cy, ccb, ccr = fdct_quant(_blocks(y), ql), fdct_quant(_blocks(cb), qc), fdct_quant(_blocks(cr), qc)
    my, mx = ccb.shape[:2]
    if sub == 420:
        cy = cy.reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
    else:
        cy = cy.reshape(my, mx, 1, 64)
    out = np.concatenate([cy, ccb[:, :, None], ccr[:, :, None]], axis=2).reshape(my * mx, -1, 64)
    return out[:, :, ZIGZAG].astype(np.int16)


def category(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    """A bit string written MSB first: whole bytes leave the accumulator as they fill."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        if self.n >= 64:
            keep = self.n % 8
            self.out += (self.acc >> keep).to_bytes((self.n - keep) // 8, "big")
            self.acc, self.n = self.acc & ((1 << keep) - 1), keep

    def put_value(self, v, cat):
        if cat:
            self.put(v if v >= 0 else v + (1 << cat) - 1, cat)

    def stuffed(self):
        """The bits padded with ones to a byte boundary, every 0xFF followed by 0x00."""
        pad = -self.n % 8
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        return bytes(self.out + acc.to_bytes(n // 8, "big")).replace(b"\xff", b"\xff\x00")


def encode_block(bits, zz, pred, dc_codes, ac_codes):
    """One block of 64 zigzag coefficients; returns its DC."""
    dc = int(zz[0])
    cat = category(dc - pred)
    assert cat <= 11, "DC difference beyond category 11"
    bits.put(*dc_codes[cat])
    bits.put_value(dc - pred, cat)
    last = 0
    for k in (np.nonzero(zz[1:])[0] + 1).tolist():
        run, last = k - last - 1, k
        while run > 15:
            bits.put(*ac_codes[0xF0])
            run -= 16
        v = int(zz[k])
        cat = category(v)
        assert 1 <= cat <= 10, "AC coefficient beyond category 10"
        bits.put(*ac_codes[(run << 4) | cat])
        bits.put_value(v, cat)
    if zz[63] == 0:
        bits.put(*ac_codes[0x00])
    return dc


def entropy(coefs, ri):
    """The entropy data of coefficients() output with ri MCUs per restart interval: stuffed intervals with RSTm between them."""
    n_mcu, bpm = coefs.shape[:2]
    out = bytearray()
    n_int = -(-n_mcu // ri)
    for i in range(n_int):
        bits, pred = _Bits(), [0, 0, 0]
        for m in range(i * ri, min((i + 1) * ri, n_mcu)):
            for b in range(bpm):
                comp = 0 if b < bpm - 2 else b - (bpm - 3)
                t = 0 if comp == 0 else 2
                pred[comp] = encode_block(bits, coefs[m, b], pred[comp], CODES[t], CODES[t + 1])
        out += bits.stuffed()
        if i < n_int - 1:
            out += bytes([0xFF, 0xD0 + (i & 7)])
    return bytes(out)


def encode(bgr, quality=85, restart=0, subsampling=420):
    """The complete JFIF file of a [h, w, 3] BGR uint8 image."""
    bgr = np.asarray(bgr)
    c = coefficients(bgr, quality, subsampling)
    h, w = bgr.shape[:2]
    g = geometry(h, w, restart, subsampling)
    return header(h, w, quality, restart, subsampling) + entropy(c, g["ri"]) + b"\xff\xd9"


def known_answer_image(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(16 * x + y) & 255, (16 * y + 3 * x) & 255, (x * y + 7) & 255], axis=-1).astype(np.uint8)
