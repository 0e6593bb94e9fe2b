// kernels_jpegdec.hip -- the device half of the JPEG decoding stage (jpegdec.hpp): restart markers, entropy decoding,
// dequantisation + inverse DCT, upsampling + colour.  Integer arithmetic only; tests/jpegdec_oracle.py is the specification.  The bit
// reader and the block decoder are jpegdec_decode.hpp, which the CPU compiles too.
#include "jpegdec.hpp"

namespace aic {

namespace {

// ---- restart markers: count per chunk, scan, write -------------------------------------------------------------------------------
// One block per image, thread t owns the bytes [t * chunk, (t + 1) * chunk) of the entropy data.  Whether a byte starts a marker depends
// on it and the next byte alone (jd_marker_at), so the chunks are independent; a marker's rank among the image's markers -- which
// interval it ends -- comes from the scan of the chunks' counts.
__global__ __launch_bounds__(256) void jpegdec_markers_kernel(const uint8_t* __restrict__ files, const JdImage* __restrict__ recs, int32_t* err,
                                                               int64_t* __restrict__ ivl_lo, int64_t* __restrict__ ivl_hi) {
    __shared__ int s_cnt[256];
    __shared__ int s_bad;
    const int img = blockIdx.x, t = threadIdx.x;
    if (err[img] != JD_ERR_NONE) return;                                       // the whole block
    const JdImage& r = recs[img];
    const uint8_t* ent = files + r.ent_off;
    const int64_t len = r.ent_len, chunk = (len + 255) / 256;
    const int64_t lo = t * chunk < len ? t * chunk : len, hi = lo + chunk < len ? lo + chunk : len;
    int count = 0, foreign = 0, m = 0;
    for (int64_t p = lo; p < hi; ++p) {
        const int kind = jd_marker_at(ent, p, len, &m);
        count += kind == 1, foreign |= kind == 2;
    }
    if (t == 0) s_bad = 0;
    s_cnt[t] = count;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {                                       // inclusive scan
        const int v = t >= d ? s_cnt[t - d] : 0;
        __syncthreads();
        s_cnt[t] += v;
        __syncthreads();
    }
    if (foreign) atomicOr(&s_bad, 1);
    __syncthreads();
    const bool fits = s_cnt[255] == r.intervals - 1;                           // only then has every marker a row in the interval table
    int k = s_cnt[t] - count, wrong = 0;
    if (fits) {
        int64_t* out_lo = ivl_lo + r.ivl_off;
        int64_t* out_hi = ivl_hi + r.ivl_off;
        for (int64_t p = lo; p < hi; ++p)
            if (jd_marker_at(ent, p, len, &m) == 1) {
                wrong |= m != (k & 7);
                out_hi[k] = p, out_lo[k + 1] = p + 2;
                ++k;
            }
        if (t == 0) out_lo[0] = 0, out_hi[r.intervals - 1] = len;
    }
    if (wrong) atomicOr(&s_bad, 2);
    __syncthreads();
    if (t == 0) {
        if (s_bad & 1) atomicMin(&err[img], (int32_t)JD_BAD_SCAN);
        else if (!fits || (s_bad & 2)) atomicMin(&err[img], (int32_t)JD_RESTART_SEQUENCE);
    }
}

// ---- entropy decoding: one lane per restart interval ------------------------------------------------------------------------------
// Block (x, image) decodes the image's intervals 64 x .. 64 x + 63 with the image's table set in LDS.  A lane that meets an error
// leaves (interval + 1) << 8 | reason in the image's word when that is smaller than what is there, so the first interval's reason
// stands whatever the order the lanes finish in.
__global__ __launch_bounds__(64) void jpegdec_entropy_kernel(const uint8_t* __restrict__ files, const JdImage* __restrict__ recs,
                                                              const JdTables* __restrict__ tabs, const int64_t* __restrict__ ivl_lo,
                                                              const int64_t* __restrict__ ivl_hi, int32_t* err, int16_t* __restrict__ coef) {
    __shared__ JdTables tab;
    const int img = blockIdx.y, t = threadIdx.x;
    if (err[img] < 256) return;                                               // refused by the header or the markers; a neighbour lane's error is no reason to stop
    const JdImage& r = recs[img];
    const int k0 = blockIdx.x * 64;
    if (k0 >= r.intervals) return;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs + r.tabset);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&tab);
    for (int i = t; i < (int)(sizeof(JdTables) / 4); i += 64) dst[i] = src[i];
    __syncthreads();
    const int k = k0 + t;
    if (k >= r.intervals) return;
    const int reason = jd_interval(r, tab, files + r.ent_off, ivl_lo[r.ivl_off + k], ivl_hi[r.ivl_off + k], k, coef + r.blk_off * 64);
    if (reason) atomicMin(&err[img], (int32_t)(((uint32_t)(k + 1) << 8) | (uint32_t)reason));
}

// ---- dequantisation and inverse DCT -----------------------------------------------------------------------------------------------
// One pass of libjpeg's jidctint (ISLOW; CONST_BITS 13, PASS1_BITS 2) over v[0..7], in place.  uint32 multiplies and adds, cast back
// for the arithmetic shift: int32 two's complement with wraparound, as the oracle's np.int32.
template <int SHIFT>
__device__ __forceinline__ void jd_idct8(uint32_t (&v)[8]) {
    uint32_t z2 = v[2], z3 = v[6];
    uint32_t z1 = (z2 + z3) * 4433u;
    uint32_t tmp2 = z1 + z3 * (uint32_t)-15137;
    uint32_t tmp3 = z1 + z2 * 6270u;
    uint32_t tmp0 = (v[0] + v[4]) << 13, tmp1 = (v[0] - v[4]) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v[7], tmp1 = v[5], tmp2 = v[3], tmp3 = v[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
    z1 *= (uint32_t)-7373, z2 *= (uint32_t)-20995, z3 = z3 * (uint32_t)-16069 + z5, z4 = z4 * (uint32_t)-3196 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr uint32_t R = 1u << (SHIFT - 1);
    v[0] = (uint32_t)((int32_t)(tmp10 + tmp3 + R) >> SHIFT), v[7] = (uint32_t)((int32_t)(tmp10 - tmp3 + R) >> SHIFT);
    v[1] = (uint32_t)((int32_t)(tmp11 + tmp2 + R) >> SHIFT), v[6] = (uint32_t)((int32_t)(tmp11 - tmp2 + R) >> SHIFT);
    v[2] = (uint32_t)((int32_t)(tmp12 + tmp1 + R) >> SHIFT), v[5] = (uint32_t)((int32_t)(tmp12 - tmp1 + R) >> SHIFT);
    v[3] = (uint32_t)((int32_t)(tmp13 + tmp0 + R) >> SHIFT), v[4] = (uint32_t)((int32_t)(tmp13 - tmp0 + R) >> SHIFT);
}

// 8 lanes per block, 32 blocks per workgroup: lane c does column c, the workspace crosses LDS, lane r does row r and stores its 8 bytes.
__global__ __launch_bounds__(256) void jpegdec_idct_kernel(const JdImage* __restrict__ recs, const JdTables* __restrict__ tabs, const int32_t* __restrict__ err,
                                                            const int16_t* __restrict__ coef, uint8_t* __restrict__ samples) {
    __shared__ uint32_t ws[32][8][9];
    const int img = blockIdx.y, g = threadIdx.x >> 3, lane = threadIdx.x & 7;
    if (err[img] != JD_ERR_NONE) return;                                       // the whole block
    const JdImage& r = recs[img];
    const int bpm = jd_bpm(r), ny = bpm - (r.ncomp - 1);
    const int64_t n_blk = (int64_t)r.mcus_x * r.mcus_y * bpm, blk = (int64_t)blockIdx.x * 32 + g;
    const bool live = blk < n_blk;
    uint32_t v[8];
    if (live) {
        const int b = (int)(blk % bpm), c = b < ny ? 0 : b - ny + 1;
        const uint16_t* q = tabs[r.tabset].q[r.tq[c] & 3];
        const int16_t* in = coef + (r.blk_off + blk) * 64;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (uint32_t)(int32_t)in[k * 8 + lane] * (uint32_t)q[k * 8 + lane];
        jd_idct8<11>(v);
#pragma unroll
        for (int k = 0; k < 8; ++k) ws[g][k][lane] = v[k];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = ws[g][lane][k];
    jd_idct8<18>(v);
    uint8_t* out = samples + (r.blk_off + blk) * 64 + lane * 8;              // 8-byte aligned: hipMalloc's base + a multiple of 8
    uint32_t w[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int s = (int32_t)v[k] + 128;
        w[k >> 2] |= (uint32_t)(s < 0 ? 0 : s > 255 ? 255 : s) << (8 * (k & 3));
    }
    *reinterpret_cast<uint2*>(out) = make_uint2(w[0], w[1]);
}

// ---- upsampling and colour --------------------------------------------------------------------------------------------------------
// The samples are kept as the IDCT left them, [MCU, block, 8, 8]: sample (y, x) of a component with bh x bv blocks per MCU.
__device__ __forceinline__ int jd_sample(const uint8_t* __restrict__ s, const JdImage& r, int bpm, int first, int bh, int bv, int y, int x) {
    const int64_t mcu = (int64_t)(y / (8 * bv)) * r.mcus_x + x / (8 * bh);
    const int b = first + ((y >> 3) % bv) * bh + ((x >> 3) % bh);
    return s[(mcu * bpm + b) * 64 + (y & 7) * 8 + (x & 7)];
}

// One thread per pixel.  Chroma: libjpeg's triangle filters over the component's own ceil(w / 2) x ceil(h / 2) (4:2:2: ceil(w / 2) x h)
// samples, edges replicated -- the MCU padding is never read.
__global__ __launch_bounds__(256) void jpegdec_colour_kernel(const JdImage* __restrict__ recs, int h, int w, const int32_t* __restrict__ err,
                                                              const uint8_t* __restrict__ samples, uint8_t* __restrict__ out) {
    const int img = blockIdx.y;
    if (err[img] != JD_ERR_NONE) return;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)h * w) return;
    const JdImage& r = recs[img];
    const int y = (int)(idx / w), x = (int)(idx % w), bpm = jd_bpm(r), ny = bpm - (r.ncomp - 1);
    const uint8_t* s = samples + r.blk_off * 64;
    const int Y = jd_sample(s, r, bpm, 0, r.hs, r.vs, y, x);
    int B = Y, G = Y, R = Y;
    if (r.ncomp == 3) {
        int c[2];
        const int cw = (w + r.hs - 1) / r.hs, ch = (h + r.vs - 1) / r.vs;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (r.hs == 1) {
                c[k] = jd_sample(s, r, bpm, ny + k, 1, 1, y, x);
            } else {
                const int cx = x >> 1, cxn = (x & 1) ? (cx + 1 < cw ? cx + 1 : cw - 1) : (cx > 0 ? cx - 1 : 0);
                if (r.vs == 1) {
                    c[k] = (3 * jd_sample(s, r, bpm, ny + k, 1, 1, y, cx) + jd_sample(s, r, bpm, ny + k, 1, 1, y, cxn) + ((x & 1) ? 2 : 1)) >> 2;
                } else {
                    const int cy = y >> 1, cyn = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
                    const int s0 = 3 * jd_sample(s, r, bpm, ny + k, 1, 1, cy, cx) + jd_sample(s, r, bpm, ny + k, 1, 1, cyn, cx);
                    const int s1 = 3 * jd_sample(s, r, bpm, ny + k, 1, 1, cy, cxn) + jd_sample(s, r, bpm, ny + k, 1, 1, cyn, cxn);
                    c[k] = (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;
                }
            }
        }
        const int cb = c[0] - 128, cr = c[1] - 128;
        R = Y + ((91881 * cr + 32768) >> 16);
        G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        B = Y + ((116130 * cb + 32768) >> 16);
        R = R < 0 ? 0 : R > 255 ? 255 : R, G = G < 0 ? 0 : G > 255 ? 255 : G, B = B < 0 ? 0 : B > 255 ? 255 : B;
    }
    uint8_t* o = out + ((int64_t)img * h * w + idx) * 3;
    o[0] = (uint8_t)B, o[1] = (uint8_t)G, o[2] = (uint8_t)R;
}

}  // namespace

void launch_jpegdec_markers(const uint8_t* files, const JdImage* recs, int n_images, int32_t* err, int64_t* ivl_lo, int64_t* ivl_hi, hipStream_t s) {
    jpegdec_markers_kernel<<<dim3(n_images), dim3(256), 0, s>>>(files, recs, err, ivl_lo, ivl_hi);
    KCHECK();
}

void launch_jpegdec_entropy(const uint8_t* files, const JdImage* recs, int n_images, int max_intervals, const JdTables* tabs, const int64_t* ivl_lo,
                            const int64_t* ivl_hi, int32_t* err, int16_t* coef, hipStream_t s) {
    jpegdec_entropy_kernel<<<dim3(ceil_div(max_intervals, 64), n_images), dim3(64), 0, s>>>(files, recs, tabs, ivl_lo, ivl_hi, err, coef);
    KCHECK();
}

void launch_jpegdec_idct(const JdImage* recs, int n_images, int64_t max_blocks, const JdTables* tabs, const int32_t* err, const int16_t* coef,
                         uint8_t* samples, hipStream_t s) {
    jpegdec_idct_kernel<<<dim3(ceil_div(max_blocks, 32), n_images), dim3(256), 0, s>>>(recs, tabs, err, coef, samples);
    KCHECK();
}

void launch_jpegdec_colour(const JdImage* recs, int n_images, int h, int w, const int32_t* err, const uint8_t* samples, uint8_t* out, hipStream_t s) {
    jpegdec_colour_kernel<<<dim3(ceil_div((long)h * w, 256), n_images), dim3(256), 0, s>>>(recs, h, w, err, samples, out);
    KCHECK();
}

}  // namespace aic
