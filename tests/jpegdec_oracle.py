"""The JPEG decoding stage's specification (aic_jpegdec_*) in NumPy and plain Python, integer arithmetic only:
baseline sequential DCT, 8 bit, one interleaved scan, gray or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, any tables, any restart interval.  The
device's pixels equal decode()'s byte for byte and its coefficient buffer equals coefficients(); a refused file carries the same reason.
Huffman decoding is Annex F, the inverse DCT libjpeg's jidctint (ISLOW) in wrapping int32, upsampling libjpeg's triangle filters over the
component's own samples, colour libjpeg's 16-bit fixed point.  No imaging library in here."""
import numpy as np

from jpeg_oracle import HUFF_SPECS, ZIGZAG

ERR_FORMAT = -6
REASONS = ("OK", "TRUNCATED", "NOT_JPEG", "NOT_BASELINE", "PRECISION", "COMPONENTS", "SAMPLING", "SIZE_MISMATCH", "BAD_TABLE", "MISSING_TABLE",
           "BAD_SCAN", "RESTART_SEQUENCE", "BAD_CODE", "OVERRUN")
(OK, TRUNCATED, NOT_JPEG, NOT_BASELINE, PRECISION, COMPONENTS, SAMPLING, SIZE_MISMATCH, BAD_TABLE, MISSING_TABLE, BAD_SCAN, RESTART_SEQUENCE,
 BAD_CODE, OVERRUN) = range(14)
DIM_MAX = 16384


class Refused(Exception):
    def __init__(self, reason):
        super().__init__(REASONS[reason])
        self.reason = reason


def _huff_ok(counts):
    code = 0
    for length in range(1, 17):
        code += counts[length - 1]
        if code > (1 << length):
            return False
        code <<= 1
    return True


def parse(file, size=None):
    """The header of a file up to the entropy data: dict(width, height, components, sampling, restart, intervals, entropy_offset,
    entropy_bytes, hs, vs, mcus_x, mcus_y, quant [components][64] natural order, huff [components] of ((counts, symbols) DC, AC)).
    size = (height, width) the picture must have.  Raises Refused.  file: bytes, a memoryview or anything indexed like them; only
    file[i] with 0 <= i < len(file) and slices inside that range are read."""
    f = file
    n = len(f)
    if n < 2 or f[0] != 0xFF or f[1] != 0xD8:
        raise Refused(NOT_JPEG)
    quant, huff, frame, ri, adobe, pos = {}, {}, None, 0, -1, 2
    while True:
        if pos + 2 > n:
            raise Refused(TRUNCATED)
        if f[pos] != 0xFF:
            raise Refused(NOT_JPEG)
        m = f[pos + 1]
        if m == 0xFF:                                             # a fill byte
            pos += 1
            continue
        pos += 2
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD8:
            raise Refused(NOT_JPEG)
        if m == 0xD9:
            raise Refused(BAD_SCAN)
        if pos + 2 > n:
            raise Refused(TRUNCATED)
        length = (f[pos] << 8) | f[pos + 1]
        if length < 2:
            raise Refused(NOT_JPEG)
        if pos + length > n:
            raise Refused(TRUNCATED)
        seg = bytes(f[pos + 2:pos + length])
        pos += length
        if m == 0xC0:
            if frame is not None:
                raise Refused(NOT_BASELINE)
            if len(seg) < 6:
                raise Refused(NOT_JPEG)
            if seg[0] != 8:
                raise Refused(PRECISION)
            if seg[5] not in (1, 3):
                raise Refused(COMPONENTS)
            if len(seg) != 6 + 3 * seg[5]:
                raise Refused(NOT_JPEG)
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            if not (1 <= h <= DIM_MAX and 1 <= w <= DIM_MAX) or (size is not None and (h, w) != tuple(size)):
                raise Refused(SIZE_MISMATCH)
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(seg[5])]
            if len(comps) == 1:
                ok = comps[0][1:3] == (1, 1)
            else:
                ok = comps[0][1:3] in ((1, 1), (2, 1), (2, 2)) and comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1)
            if not ok:
                raise Refused(SAMPLING)
            if any(c[3] > 3 for c in comps):
                raise Refused(BAD_TABLE)
            frame = (h, w, comps)
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF):
            raise Refused(NOT_BASELINE)
        elif m == 0xDB:
            k = 0
            while k < len(seg):
                if seg[k] >> 4 or (seg[k] & 15) > 3 or k + 65 > len(seg):
                    raise Refused(BAD_TABLE)
                t = np.zeros(64, np.int32)
                t[ZIGZAG] = np.frombuffer(seg[k + 1:k + 65], np.uint8)
                quant[seg[k] & 15] = t
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                if (seg[k] >> 4) > 1 or (seg[k] & 15) > 1 or k + 17 > len(seg):
                    raise Refused(BAD_TABLE)
                counts = list(seg[k + 1:k + 17])
                if sum(counts) > 256 or k + 17 + sum(counts) > len(seg) or not _huff_ok(counts):
                    raise Refused(BAD_TABLE)
                huff[(seg[k] >> 4, seg[k] & 15)] = (counts, list(seg[k + 17:k + 17 + sum(counts)]))
                k += 17 + sum(counts)
        elif m == 0xDD:
            if len(seg) != 2:
                raise Refused(NOT_JPEG)
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xEE:
            if len(seg) >= 12 and seg[:5] == b"Adobe":
                adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Refused(BAD_SCAN)
            h, w, comps = frame
            if len(seg) < 1 or seg[0] != len(comps) or len(seg) != 4 + 2 * seg[0]:
                raise Refused(BAD_SCAN)
            sel = []
            for i, c in enumerate(comps):
                if seg[1 + 2 * i] != c[0] or (seg[2 + 2 * i] >> 4) > 1 or (seg[2 + 2 * i] & 15) > 1:
                    raise Refused(BAD_SCAN)
                sel.append((seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15))
            if tuple(seg[-3:]) != (0, 63, 0):
                raise Refused(BAD_SCAN)
            if len(comps) == 3 and adobe == 0:
                raise Refused(COMPONENTS)
            if any(c[3] not in quant for c in comps):
                raise Refused(MISSING_TABLE)
            if not huff:                                          # the Motion-JPEG convention: no DHT at all means Annex K
                huff = {(0, 0): HUFF_SPECS[0], (1, 0): HUFF_SPECS[1], (0, 1): HUFF_SPECS[2], (1, 1): HUFF_SPECS[3]}
            if any((0, td) not in huff or (1, ta) not in huff for td, ta in sel):
                raise Refused(MISSING_TABLE)
            if n - pos < 2 or f[n - 2] != 0xFF or f[n - 1] != 0xD9:
                raise Refused(TRUNCATED)
            hs, vs = comps[0][1:3]
            mx, my = -(-w // (8 * hs)), -(-h // (8 * vs))
            return dict(width=w, height=h, components=len(comps), sampling=400 if len(comps) == 1 else {(1, 1): 444, (2, 1): 422, (2, 2): 420}[(hs, vs)],
                        restart=ri, intervals=-(-(mx * my) // ri) if ri else 1, entropy_offset=pos, entropy_bytes=n - 2 - pos, hs=hs, vs=vs,
                        mcus_x=mx, mcus_y=my, quant=[quant[c[3]] for c in comps], huff=[(huff[(0, td)], huff[(1, ta)]) for td, ta in sel])
        # APPn, COM and every other segment: skipped


def intervals(ent, expected):
    """[(start, end)] of the restart intervals of the entropy bytes `ent`, found by their RSTm markers."""
    b = np.frombuffer(bytes(ent), np.uint8)
    ff = np.flatnonzero(b[:-1] == 0xFF) if len(b) else np.zeros(0, np.int64)
    nxt = b[ff + 1]
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    if (~rst & (nxt != 0) & (nxt != 0xFF)).any():                 # another marker inside the scan
        raise Refused(BAD_SCAN)
    at = ff[rst]
    if len(at) != expected - 1 or ((b[at + 1] & 7) != (np.arange(len(at)) & 7)).any():
        raise Refused(RESTART_SEQUENCE)
    starts, ends = [0] + (at + 2).tolist(), at.tolist() + [len(b)]
    return list(zip(starts, ends))


_LUT = {}


def _lut16(spec):
    """lut[the next 16 bits] = length << 8 | symbol, 0 where no code matches."""
    key = (tuple(spec[0]), tuple(spec[1]))
    if key not in _LUT:
        lut, code, k = np.zeros(65536, np.int32), 0, 0
        for length in range(1, 17):
            for _ in range(spec[0][length - 1]):
                lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | spec[1][k]
                code, k = code + 1, k + 1
            code <<= 1
        _LUT[key] = lut.tolist()
    return _LUT[key]


class _Reader:
    """The bits of one interval: up to the first 0xFF that no 0x00 follows, 0xFF 0x00 unstuffed.  No bits are invented: a symbol that
    needs more than there are is OVERRUN."""

    def __init__(self, data):
        data = bytes(data)
        k = 0
        while True:
            k = data.find(b"\xff", k)
            if k < 0 or k + 1 >= len(data) or data[k + 1] != 0:
                break
            k += 2
        if k >= 0:
            data = data[:k]
        data = data.replace(b"\xff\x00", b"\xff")
        self.total, self.pos = 8 * len(data), 0
        self.v = int.from_bytes(data + b"\0\0\0\0", "big")
        self.width = self.total + 32

    def peek16(self):
        return (self.v >> (self.width - self.pos - 16)) & 0xFFFF

    def take(self, k):
        v = (self.v >> (self.width - self.pos - k)) & ((1 << k) - 1)
        self.pos += k
        if self.pos > self.total:
            raise Refused(OVERRUN)
        return v

    def symbol(self, lut):
        e = lut[self.peek16()]
        if e == 0:
            raise Refused(OVERRUN if self.total - self.pos < 16 else BAD_CODE)
        self.take(e >> 8)
        return e & 255

    def extend(self, s):
        v = self.take(s)
        return v if v >> (s - 1) else v - (1 << s) + 1


def _block(r, dc, ac, pred, out):
    s = r.symbol(dc)
    if s > 11:
        raise Refused(BAD_CODE)
    pred += r.extend(s) if s else 0
    if not -32768 <= pred <= 32767:
        raise Refused(BAD_CODE)
    out[0] = pred
    k = 1
    while k < 64:
        rs = r.symbol(ac)
        run, s = rs >> 4, rs & 15
        if s == 0:
            if run != 15:
                break
            if k + 16 > 64:
                raise Refused(BAD_CODE)
            k += 16
            continue
        k += run
        if s > 10 or k > 63:
            raise Refused(BAD_CODE)
        out[ZIGZAG[k]] = r.extend(s)
        k += 1
    return pred


def _coefficients(file, p):
    f = memoryview(file)
    ent = f[p["entropy_offset"]:p["entropy_offset"] + p["entropy_bytes"]]
    n_mcu, ncomp = p["mcus_x"] * p["mcus_y"], p["components"]
    bpm = 1 if ncomp == 1 else p["hs"] * p["vs"] + 2
    comp_of = [0] * (bpm - ncomp + 1) + [1, 2][:ncomp - 1]
    luts = [(_lut16(d), _lut16(a)) for d, a in p["huff"]]
    ri = p["restart"] or n_mcu
    out = np.zeros((n_mcu, bpm, 64), np.int32)
    for k, (lo, hi) in enumerate(intervals(ent, p["intervals"])):
        r, pred = _Reader(ent[lo:hi]), [0, 0, 0]
        for m in range(k * ri, min((k + 1) * ri, n_mcu)):
            for b in range(bpm):
                c = comp_of[b]
                pred[c] = _block(r, luts[c][0], luts[c][1], pred[c], out[m, b])
    return out.astype(np.int16)


def coefficients(file, size=None):
    """int16 [MCUs, blocks per MCU, 64]: the quantised coefficients in natural order, MCU-interleaved (Y.. Cb Cr) -- the layout of the
    device's coefficient buffer.  [..., jpeg_oracle.ZIGZAG] is the encoder's layout.  Raises Refused."""
    return _coefficients(file, parse(file, size))


def _i32(x):
    return np.asarray(x, np.int64).astype(np.int32)


def _idct_pass(v, shift):
    """One jidctint pass over v[0..7] (int32 arrays), wrapping int32 arithmetic throughout."""
    c = np.int32
    z2, z3 = v[2], v[6]
    z1 = (z2 + z3) * c(4433)
    tmp2 = z1 + z3 * c(-15137)
    tmp3 = z1 + z2 * c(6270)
    tmp0 = (v[0] + v[4]) << c(13)
    tmp1 = (v[0] - v[4]) << c(13)
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[7], v[5], v[3], v[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * c(9633)
    tmp0, tmp1, tmp2, tmp3 = tmp0 * c(2446), tmp1 * c(16819), tmp2 * c(25172), tmp3 * c(12299)
    z1, z2, z3, z4 = z1 * c(-7373), z2 * c(-20995), z3 * c(-16069) + z5, z4 * c(-3196) + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = c(1 << (shift - 1))
    s = c(shift)
    return [(tmp10 + tmp3 + r) >> s, (tmp11 + tmp2 + r) >> s, (tmp12 + tmp1 + r) >> s, (tmp13 + tmp0 + r) >> s,
            (tmp13 - tmp0 + r) >> s, (tmp12 - tmp1 + r) >> s, (tmp11 - tmp2 + r) >> s, (tmp10 - tmp3 + r) >> s]


def idct(coef, q):
    """uint8 samples [..., 8, 8] of coefficients [..., 64] (natural order) and a quantisation table [64]: coef * Q, columns with
    (x + 2^10) >> 11, rows with (x + 2^17) >> 18, + 128, clamped.  int32 two's complement with wraparound, whatever the input."""
    with np.errstate(over="ignore"):
        w = (coef.astype(np.int32) * q.astype(np.int32)).reshape(*coef.shape[:-1], 8, 8)
        cols = _idct_pass([w[..., k, :] for k in range(8)], 11)           # cols[k][..., column]
        ws = np.stack(cols, axis=-2)                                      # [..., row, column]
        rows = _idct_pass([ws[..., :, k] for k in range(8)], 18)          # rows[k][..., row]
        out = np.stack(rows, axis=-1) + np.int32(128)
    return np.clip(out, 0, 255).astype(np.uint8)


def _plane(samples, mx, my, bh, bv):
    """[my * bv * 8, mx * bh * 8] plane of samples [my * mx, bv * bh, 8, 8]."""
    return samples.reshape(my, mx, bv, bh, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * bv * 8, mx * bh * 8)


def upsample_h2v1(c):
    """libjpeg's triangle filter along x: [h, cw] -> [h, 2 cw], edges replicated."""
    c = c.astype(np.int32)
    left, right = np.concatenate([c[:, :1], c[:, :-1]], 1), np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int32)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out


def upsample_h2v2(c):
    """libjpeg's triangle filter along both axes: [ch, cw] -> [2 ch, 2 cw], edges replicated."""
    c = c.astype(np.int32)
    up, down = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int32)
    for row, near in ((0, up), (1, down)):
        s = 3 * c + near
        left, right = np.concatenate([s[:, :1], s[:, :-1]], 1), np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[row::2, 0::2] = (3 * s + left + 8) >> 4
        out[row::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def colour(y, cb, cr):
    """BGR uint8 [h, w, 3] of full-resolution int32 planes."""
    y, cb, cr = y.astype(np.int32), cb.astype(np.int32) - 128, cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def pixels(coef, p):
    """BGR uint8 [h, w, 3] of coefficients() output and the parse."""
    h, w, hs, vs, mx, my = p["height"], p["width"], p["hs"], p["vs"], p["mcus_x"], p["mcus_y"]
    ny = hs * vs
    y = _plane(idct(coef[:, :ny], p["quant"][0]), mx, my, hs, vs)[:h, :w]
    if p["components"] == 1:
        return np.repeat(y[:, :, None], 3, 2)
    ch, cw = -(-h // vs), -(-w // hs)
    c = [_plane(idct(coef[:, ny + k:ny + k + 1], p["quant"][1 + k]), mx, my, 1, 1)[:ch, :cw] for k in range(2)]
    if (hs, vs) == (2, 2):
        c = [upsample_h2v2(x) for x in c]
    elif (hs, vs) == (2, 1):
        c = [upsample_h2v1(x) for x in c]
    return colour(y, c[0][:h, :w], c[1][:h, :w])


def info_of(p=None, reason=OK):
    keys = ("width", "height", "components", "sampling", "restart", "intervals", "entropy_offset", "entropy_bytes")
    out = dict(status=ERR_FORMAT if reason else 0, reason=reason)
    out.update({k: (p[k] if p else 0) for k in keys})
    return out


def probe(file, size=None):
    """What aic_jpegdec_probe reports: the header's fields, or status ERR_FORMAT and the reason with every field zero."""
    try:
        return info_of(parse(file, size))
    except Refused as e:
        return info_of(None, e.reason)


def decode(file, size=None):
    """(bgr uint8 [h, w, 3] or None, info): info as probe(), with the reason of a refusal the entropy data caused as well."""
    try:
        p = parse(file, size)
        return pixels(_coefficients(file, p), p), info_of(p)
    except Refused as e:
        return None, info_of(None, e.reason)
