"""Cases and expected tensors for the crop resamplers (csrc/kernels_pre.hip crop_resize_kernel in its byte, wide and 2x2 forms; the
crop fused into the ReID stem, csrc/kernels_conv_direct.hip reid_stem_pool2_kernel), every output layout.  Plain NumPy + the integer
contract of oracle/image_oracle.py; no GPU here.  tests/test_gpu_crop_paths.py runs the cases on the device and compares with
np.array_equal; tests/test_crop_cases.py proves on the CPU that the cases reach every path and that wrong kernels would fail them.

Banks.  Three frames of uniform u8 noise: any wrong tap, frame or channel changes the pixel.  Width 139: the row pitch is 417 bytes,
1 (mod 4), and with 45 rows a frame is 18 765 bytes, 1 (mod 4): rows and frames start at every byte alignment, which is what the
aligned 12-byte loads of the wide path and of the fused stem shift by.  70 rows for the crops of 32 rows (their exact 2x box is 64
rows high).  The bank a shape runs on is BANK_OF; 8 x 240 and the project's 128 x 64 are larger than twice any box of these frames,
so there every crop is interpolated and nearly every one enlarged, and the 2x2 path is pinned at the other three shapes.  The fused stem
also runs at the project's own 128 x 64 (the session's ReID engine) on a third bank of 262 rows, which holds the 256 x 128 box of its
2x2 path (STEM_BANK_OF).

Boxes (boxes_for): 22 per (bank, shape), see the comments there.  frame_of is a fixed shuffle over all three frames; the boxes that
end on the bank's last pixel lie in the last frame.

Expectation (expected): oracle/image_oracle.py crops_to_batch per box on frames[frame_of[i]] for mode 0; the same values moved to
NHWC, rounded to float16 where the layout is fp16, zero in lanes 3..7 (mode 1) or lane 3 (mode 2); an invalid crop or one at or past
n_live is all zero with valid == 0.

Mutants (expected(..., mut=)): the expectation a wrong kernel would meet, computed by resample_flat, a restatement of the oracle's
arithmetic on the flat byte array of the bank (so that a tap outside the crop reads what lies there: the neighbouring pixel, the next
frame, or FILL, the byte the test entries surround the bank with).  Unmutated it equals the oracle (asserted on the CPU).

Two mutants one might expect here cannot change any output and are therefore asserted to be EQUIVALENT, not to be caught:
  floor instead of truncation: the two differ only for negative coordinates, trunc(v) and floor(v) are then both <= 0: as x1 / y1
    both clamp to 0, as x2 / y2 both give an empty box (x2 <= 0 <= x1).  What is observable is any other rounding of positive
    coordinates: the mutant "rint" rounds to nearest.
  the 2x2 area path not taken: at scale exactly 2 the linear taps are (2d, 2d + 1) with weights 1024 / 1024 and never clamp, and the
    fixed point is exact: (1024 * (((a + b) * 1024) >> 4)) >> 16 == a + b, so the result is (a + b + c + d + 2) >> 2 either way.
    What is observable is the path taken when it must not be: the mutants "area2_w" / "area2_h" test one dimension only and meet the
    near misses (2 ow +- 1 wide, 2 oh +- 1 high)."""
import numpy as np

from oracle import image_oracle as I

FILL = 0xA5                      # what aic_crop_resize_ex / aic_reid_embed_bank put around the bank
N_FRAMES = 3
BANKS = {"45x139": (45, 139), "70x139": (70, 139), "262x139": (262, 139)}
CROP_SHAPES = [(16, 64), (32, 64), (20, 24), (8, 240), (128, 64)]      # 20: not a multiple of the kernel's 16 rows per block; 240: its width limit
STEM_SHAPES = [(16, 64), (32, 64)]
BANK_OF = {(16, 64): "45x139", (32, 64): "70x139", (20, 24): "45x139", (8, 240): "45x139", (128, 64): "70x139"}
STEM_BANK_OF = {(16, 64): "45x139", (32, 64): "70x139", (128, 64): "262x139"}
MODES = [(0, "fp32"), (1, "fp32"), (1, "fp16"), (2, "fp16")]
MUTANTS = ("frame_of", "rint", "area2_w", "area2_h", "right_tap", "vertical_clamp", "bgr", "dead")
EQUIVALENT = ("floor", "no_area2")

_cache = {}


def bank(name):
    """[3, h, w, 3] u8 noise."""
    if ("bank", name) not in _cache:
        h, w = BANKS[name]
        a = np.random.default_rng(1000 + h).integers(0, 256, (N_FRAMES, h, w, 3), dtype=np.uint8)
        a.setflags(write=False)
        _cache["bank", name] = a
    return _cache["bank", name]


def area2_fits(shape, bank_name=None):
    fh, fw = BANKS[bank_name or BANK_OF[shape]]
    return 2 * shape[0] <= fh and 2 * shape[1] <= fw


def boxes_for(shape, bank_name=None):
    """-> (boxes [22, 4] fp32 xyxy, frame_of [22] int32) for an output shape on a bank (default: BANK_OF[shape])."""
    oh, ow = shape
    H, W = BANKS[bank_name or BANK_OF[shape]]
    L = N_FRAMES - 1
    rows = [
        ((0, 0, W, H), 0),                                   # 0 the whole frame
        ((3, 2, 3 + 2 * ow, 2 + 2 * oh), 1),                 # 1 exactly 2x at an interior origin: the 2x2 path
        ((W - 2 * ow, H - 2 * oh, W, H), L),                 # 2 exactly 2x, ending on the last pixel of the bank
        ((3, 2, 3 + 2 * ow + 1, 2 + 2 * oh), 0),             # 3-6 the near misses of the 2x2 path
        ((3, 2, 3 + 2 * ow - 1, 2 + 2 * oh), 1),
        ((3, 2, 3 + 2 * ow, 2 + 2 * oh + 1), 2),
        ((3, 2, 3 + 2 * ow, 2 + 2 * oh - 1), 0),
        ((5, 3, 5 + ow, 3 + oh), 1),                         # 7 scale 1: the last column's right tap clamps
        ((W - 1, H - 1, W, H), L),                           # 8 1 x 1: the last pixel of the bank, interpolated
        ((70, 1, 71, H - 1), 2),                             # 9 one pixel wide
        ((2, 20, W - 3, 21), 0),                             # 10 one pixel high
        ((-0.9, -0.9, 30.7, 25.2), 1),                       # 11 -0.9 truncates to 0; 30.7 to 30
        ((100.5, 30.2, W + 20, H + 9), 2),                   # 12 a corner beyond the frame
        ((W, 3, W + 10, 20), 1),                             # 13 x1 == fw: empty
        ((60, 30, 50, 10), 2),                               # 14 inverted: empty
        ((10.2, 10.1, 10.9, 30), 1),                         # 15 below one pixel after truncation: empty
        ((-3.0e9, -3.0e9, 3.0e9, 3.0e9), 2),                 # 16 beyond int32: the whole frame
        ((3.0e9, 3.0e9, -3.0e9, -3.0e9), 0),                 # 17 ... and inverted: empty
        ((7.3, 4.6, 120.8, 40.2), 1),                        # 18 a fractional box: 113 x 36
        ((50.5, 10.5, 61.2, 17.9), 0),                       # 19 a small one: 11 x 7, enlarged at every shape
        ((W - 2, 0, W, H), 2),                               # 20 the last two columns, every row
        ((0, H - 9, W, H), L),                               # 21 the last nine rows: ends on the last pixel of the bank
    ]
    return np.array([r[0] for r in rows], np.float32), np.array([r[1] for r in rows], np.int32)


def clip_box(b, fh, fw, rounding="trunc"):
    """deepsort_tracker.py:148-153: int() then clamp -> (x1, y1, x2, y2), valid."""
    to_int = {"trunc": int, "floor": lambda v: int(np.floor(v)), "rint": lambda v: int(np.rint(v))}[rounding]
    x1, y1, x2, y2 = (to_int(float(v)) for v in b)
    x1, y1, x2, y2 = max(0, x1), max(0, y1), min(fw, x2), min(fh, y2)
    return (x1, y1, x2, y2), (x1 < x2 and y1 < y2)


def taps(dst, src, clamp):
    """image_oracle.resize_linear_u8's taps: (i0, i1, w0, w1).  clamp "x": index clamped and the weight forced onto the surviving tap;
    "y": rows clipped, weights kept; "x_keep": a mutant -- a right tap beyond the last column is read where it lies, weight kept."""
    s, f, _ = I._coeffs(dst, src)
    if clamp == "y":
        i0, i1 = np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1)
    else:
        lo, hi = s < 0, s >= src - 1
        if clamp == "x_keep":
            hi = np.zeros_like(hi)
        f = np.where(lo | hi, np.float32(0), f)
        s = np.where(lo, 0, np.where(hi, src - 1, s))
        i0, i1 = s, (s + 1 if clamp == "x_keep" else np.minimum(s + 1, src - 1))
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return i0.astype(np.int64), i1.astype(np.int64), w0, w1


def flat_bank(frames):
    """The bank as the device holds it: its bytes with 16 FILL bytes in front and behind -> (flat int64 array, index of byte 0)."""
    flat = np.full(frames.size + 32, FILL, np.int64)
    flat[16:16 + frames.size] = frames.reshape(-1)
    return flat, 16


def resample_flat(frames, fi, box, oh, ow, area2=None, xclamp="x", yclamp="y"):
    """u8 [oh, ow, 3] BGR of one valid crop (x1, y1, x2, y2) of frame fi, addressed as bytes of the whole bank."""
    _, fh, fw, _ = frames.shape
    buf, z = flat_bank(frames)
    flat = lambda a: np.where((a >= 0) & (a < len(buf)), buf[np.clip(a, 0, len(buf) - 1)], FILL)      # noqa: E731 (a mutant may read anywhere)
    pitch = fw * 3
    x1, y1, x2, y2 = box
    sw, sh = x2 - x1, y2 - y1
    base = z + fi * fh * pitch
    c = np.arange(3)
    if (sw == 2 * ow and sh == 2 * oh) if area2 is None else area2:
        a = base + (y1 + 2 * np.arange(oh))[:, None, None] * pitch + (x1 + 2 * np.arange(ow))[None, :, None] * 3 + c
        return ((flat(a) + flat(a + 3) + flat(a + pitch) + flat(a + pitch + 3) + 2) >> 2).astype(np.uint8)
    xi0, xi1, xw0, xw1 = taps(ow, sw, xclamp)
    yi0, yi1, yw0, yw1 = taps(oh, sh, "y" if yclamp == "y" else "x")

    def hrow(yi):
        r = base + (y1 + yi)[:, None, None] * pitch
        return flat(r + (x1 + xi0)[None, :, None] * 3 + c) * xw0[None, :, None] + flat(r + (x1 + xi1)[None, :, None] * 3 + c) * xw1[None, :, None]
    out = (((yw0[:, None, None] * (hrow(yi0) >> 4)) >> 16) + ((yw1[:, None, None] * (hrow(yi1) >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def normalise(u8_bgr, swap=True):
    """image_processing.py:126-131: BGR -> RGB, (x / 255 - mean) / std in fp32 -> [3, oh, ow]."""
    rgb = u8_bgr[:, :, ::-1] if swap else u8_bgr
    return np.transpose((rgb.astype(np.float32) / 255.0 - I.IMAGENET_MEAN) / I.IMAGENET_STD, (2, 0, 1))


def nchw(frames, boxes, frame_of, shape, mut=None):
    """-> (fp32 [n, 3, oh, ow], valid [n]): the oracle for mut None, else the mutated restatement."""
    oh, ow = shape
    _, fh, fw, _ = frames.shape
    n = len(boxes)
    out, valid = np.zeros((n, 3, oh, ow), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        fi = 0 if mut == "frame_of" else int(frame_of[i])
        if mut is None:
            out[i:i + 1], valid[i:i + 1] = I.crops_to_batch(frames[fi], boxes[i:i + 1], shape)
            continue
        box, ok = clip_box(boxes[i], fh, fw, mut if mut in ("floor", "rint") else "trunc")
        if not ok:
            continue
        sw, sh = box[2] - box[0], box[3] - box[1]
        area2 = {"no_area2": False, "area2_w": sw == 2 * ow, "area2_h": sh == 2 * oh}.get(mut)
        u8 = resample_flat(frames, fi, box, oh, ow, area2, "x_keep" if mut == "right_tap" else "x", "x" if mut == "vertical_clamp" else "y")
        out[i], valid[i] = normalise(u8, swap=mut != "bgr"), 1
    return out, valid


def layout(x, mode, dtype):
    """fp32 [n, 3, oh, ow] -> the tensor of a mode: 0 as it is; 1 [n, oh, ow, 8] of dtype; 2 float16 [n, oh, ow, 4]; spare lanes zero."""
    if mode == 0:
        return x
    n, _, oh, ow = x.shape
    out = np.zeros((n, oh, ow, 8 if mode == 1 else 4), np.float16 if (mode == 2 or dtype == "fp16") else np.float32)
    out[..., :3] = x.transpose(0, 2, 3, 1)           # (rounds to nearest even where the layout is float16, as the kernel's conversion does)
    return out


def expected(shape, mode=0, dtype="fp32", n_live=None, mut=None, n=None, bank_name=None):
    """-> (tensor, valid) the kernels must produce for the case of `shape`: boxes_for(shape)[:n] on its bank."""
    bank_name = bank_name or BANK_OF[shape]
    boxes, fo = boxes_for(shape, bank_name)
    n = len(boxes) if n is None else n
    key = ("nchw", shape, bank_name, mut if mut != "dead" else None)
    if key not in _cache:
        x, v = nchw(bank(bank_name), boxes, fo, shape, key[3])
        x.setflags(write=False), v.setflags(write=False)
        _cache[key] = x, v
    x, v = (a[:n].copy() for a in _cache[key])
    if n_live is not None and mut != "dead":
        x[max(n_live, 0):] = 0
        v[max(n_live, 0):] = 0
    return layout(x, mode, dtype), v


def stats(shape, bank_name=None):
    """What the case of `shape` reaches, from the oracle's own arithmetic: the byte alignments of the left taps of the interpolated
    crops (address relative to the bank's first byte), and the indices of the crops of each kind."""
    bank_name = bank_name or BANK_OF[shape]
    boxes, fo = boxes_for(shape, bank_name)
    oh, ow = shape
    frames = bank(bank_name)
    _, fh, fw, _ = frames.shape
    pitch, last = fw * 3, frames.size - 1
    r = dict(align=set(), clamped=[], area2=[], area2_last=[], interp_last=[], invalid=[], enlarged=[], frames=set())
    for i, b in enumerate(boxes):
        (x1, y1, x2, y2), ok = clip_box(b, fh, fw)
        if not ok:
            r["invalid"].append(i)
            continue
        r["frames"].add(int(fo[i]))
        sw, sh = x2 - x1, y2 - y1
        ends_last = int(fo[i]) * fh * pitch + (y2 - 1) * pitch + (x2 - 1) * 3 + 2 == last
        if sw == 2 * ow and sh == 2 * oh:
            r["area2"].append(i)
            if ends_last:
                r["area2_last"].append(i)
            continue
        xi0, xi1, _, _ = taps(ow, sw, "x")
        yi0, yi1, _, _ = taps(oh, sh, "y")
        for yi in (yi0, yi1):
            a = int(fo[i]) * fh * pitch + (y1 + yi)[:, None] * pitch + (x1 + xi0)[None, :] * 3
            r["align"] |= set(np.unique(a & 3).tolist())
        if (xi1 == xi0).any():
            r["clamped"].append(i)
        if ends_last:
            r["interp_last"].append(i)
        if sw < ow or sh < oh:
            r["enlarged"].append(i)
    return r
