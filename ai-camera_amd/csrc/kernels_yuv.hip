// kernels_yuv.hip -- NV12 / I420 -> BGR24 and back over a bank of frames in one launch (yuv.hpp).
//
// One lane owns a strip of 8 pixels x 2 rows = four 2x2 blocks: 16 luma bytes, 4 U and 4 V bytes (each chroma byte is loaded once) and
// 2 x 24 BGR bytes.  ACC picks the access width, never the arithmetic, so every path writes the same bytes:
//   ACC 8: w, pitch, frame_stride multiples of 8 and both bases 8-byte aligned: luma rows and NV12 chroma as 8-byte, I420 chroma as 4-byte,
//          BGR as three 8-byte accesses per row (adjacent lanes are adjacent in x: a wave covers 512 luma and 1536 BGR bytes of a row);
//   ACC 4: the same, the BGR side only 4-byte aligned (ring slots start at slot * h * w * 3): six 4-byte accesses per row;
//   ACC 1: any even w, any legal pitch, any base: byte accesses, the last strip of a row 2, 4 or 6 pixels wide.
// Arithmetic: tests/yuv_oracle.py, int32 throughout (the oracle asserts that nothing reaches 2^31).  No LDS, plain vector stores.
#include "yuv.hpp"

namespace aic {

namespace {

constexpr int STRIP = 8;
constexpr int HALF = 1 << (YUV_SHIFT - 1);

struct YuvArgs {
    uint8_t* yuv;              // the conversion's source is only read
    uint8_t* bgr;
    int h, w, strips;          // strips per row pair
    size_t pitch, frame_stride;
    YuvCoeffs c;
};

// clamp(v >> S, 0, 255), written as clamp first, shift second (the same value: the shift is monotonic and 255 = ((256 << S) - 1) >> S).
// On purpose: for the shift-then-clamp form of two neighbouring bytes the compiler selects gfx950's v_ashr_pk_u8_i32 and ORs further bytes
// into the upper half of its result, and on the MI355X that upper half was not zero -- bytes 2 and 3 of such words came out OR-ed with
// stray bits (found by tests/test_gpu_yuv.py).
template <int S>
__device__ __forceinline__ unsigned shift_clamp8(int v) { return (unsigned)min(max(v, 0), (256 << S) - 1) >> S; }
__device__ __forceinline__ unsigned byte_of(const unsigned* words, int i) { return (words[i >> 2] >> ((i & 3) * 8)) & 255u; }

// n_bytes <= 4 * WORDS bytes at p into words (little endian).  ACC 8 / 4: whole words, p aligned to ACC; ACC 1: byte loads, the rest zero.
template <int ACC, int WORDS>
__device__ __forceinline__ void load_words(const uint8_t* p, int n_bytes, unsigned (&words)[WORDS]) {
    if constexpr (ACC == 8 && WORDS % 2 == 0) {
#pragma unroll
        for (int i = 0; i < WORDS / 2; ++i) {
            const uint2 v = reinterpret_cast<const uint2*>(p)[i];
            words[2 * i] = v.x, words[2 * i + 1] = v.y;
        }
    } else if constexpr (ACC >= 4) {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) words[i] = reinterpret_cast<const unsigned*>(p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) {
            unsigned v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < n_bytes) v |= (unsigned)p[4 * i + b] << (8 * b);
            words[i] = v;
        }
    }
}

template <int ACC, int WORDS>
__device__ __forceinline__ void store_words(uint8_t* p, int n_bytes, const unsigned (&words)[WORDS]) {
    if constexpr (ACC == 8 && WORDS % 2 == 0) {
#pragma unroll
        for (int i = 0; i < WORDS / 2; ++i) reinterpret_cast<uint2*>(p)[i] = make_uint2(words[2 * i], words[2 * i + 1]);
    } else if constexpr (ACC >= 4) {
#pragma unroll
        for (int i = 0; i < WORDS; ++i) reinterpret_cast<unsigned*>(p)[i] = words[i];
    } else {
#pragma unroll
        for (int i = 0; i < 4 * WORDS; ++i)
            if (i < n_bytes) p[i] = (uint8_t)(words[i >> 2] >> ((i & 3) * 8));
    }
}

// The strip of this lane: false = past the last strip.  yp: luma of the upper row at the strip's first pixel; for NV12 cu points at the
// strip's first U,V pair (cv unused), for I420 cu / cv at its first U / V byte; bgr: the upper row's first BGR byte; n: pixels (2..8, even).
// (uint8_t* on both sides: each kernel only reads its source.)
template <int FMT>
__device__ __forceinline__ bool strip_of(const YuvArgs& a, uint8_t*& yp, uint8_t*& cu, uint8_t*& cv, uint8_t*& bgr, int& n) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= (a.h >> 1) * a.strips) return false;
    const int ry = idx / a.strips, x0 = (idx - ry * a.strips) * STRIP;
    n = min(STRIP, a.w - x0);
    const size_t f = blockIdx.y;
    uint8_t* yuv = a.yuv + f * a.frame_stride;
    yp = yuv + (size_t)(2 * ry) * a.pitch + x0;
    uint8_t* chroma = yuv + a.pitch * a.h;
    if (FMT == AIC_PIX_NV12) {
        cu = chroma + (size_t)ry * a.pitch + x0;
        cv = cu;
    } else {
        cu = chroma + (size_t)ry * (a.pitch >> 1) + (x0 >> 1);
        cv = cu + (a.pitch >> 1) * (size_t)(a.h >> 1);
    }
    bgr = a.bgr + ((f * a.h + 2 * ry) * a.w + x0) * 3;
    return true;
}

}  // namespace

template <int FMT, int ACC>
__global__ __launch_bounds__(256) void yuv_to_bgr_kernel(YuvArgs a) {
    uint8_t *yp, *cu, *cv, *bgr;
    int n;
    if (!strip_of<FMT>(a, yp, cu, cv, bgr, n)) return;
    constexpr int YACC = ACC == 1 ? 1 : 8, CACC = ACC == 1 ? 1 : 4;
    unsigned y0[2], y1[2], uu[1], vv[1], uv[2];
    load_words<YACC>(yp, n, y0);
    load_words<YACC>(yp + a.pitch, n, y1);
    if (FMT == AIC_PIX_NV12) load_words<YACC>(cu, n, uv);
    else load_words<CACC>(cu, n >> 1, uu), load_words<CACC>(cv, n >> 1, vv);
    const int cy = a.c.dec[0], cvr = a.c.dec[1], cvg = a.c.dec[2], cug = a.c.dec[3], cub = a.c.dec[4], yo = a.c.y_offset;
    unsigned o0[6] = {0, 0, 0, 0, 0, 0}, o1[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < STRIP / 2; ++k) {
        const int d = (int)(FMT == AIC_PIX_NV12 ? byte_of(uv, 2 * k) : byte_of(uu, k)) - 128;
        const int e = (int)(FMT == AIC_PIX_NV12 ? byte_of(uv, 2 * k + 1) : byte_of(vv, k)) - 128;
        const int tr = cvr * e + HALF, tg = cvg * e + cug * d + HALF, tb = cub * d + HALF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {                       // the block's four pixels: upper left, upper right, lower left, lower right
            const int px = 2 * k + (j & 1);
            const int c = cy * ((int)byte_of(j < 2 ? y0 : y1, px) - yo);
            const unsigned b = shift_clamp8<YUV_SHIFT>(c + tb), g = shift_clamp8<YUV_SHIFT>(c + tg), r = shift_clamp8<YUV_SHIFT>(c + tr);
            unsigned* o = j < 2 ? o0 : o1;
            o[(3 * px) >> 2] |= b << (((3 * px) & 3) * 8);
            o[(3 * px + 1) >> 2] |= g << (((3 * px + 1) & 3) * 8);
            o[(3 * px + 2) >> 2] |= r << (((3 * px + 2) & 3) * 8);
        }
    }
    store_words<ACC>(bgr, 3 * n, o0);
    store_words<ACC>(bgr + (size_t)a.w * 3, 3 * n, o1);
}

template <int FMT, int ACC>
__global__ __launch_bounds__(256) void bgr_to_yuv_kernel(YuvArgs a) {
    uint8_t *yp, *cu, *cv, *bgr;
    int n;
    if (!strip_of<FMT>(a, yp, cu, cv, bgr, n)) return;
    constexpr int YACC = ACC == 1 ? 1 : 8, CACC = ACC == 1 ? 1 : 4;
    unsigned i0[6], i1[6];
    load_words<ACC>(bgr, 3 * n, i0);
    load_words<ACC>(bgr + (size_t)a.w * 3, 3 * n, i1);
    const int yr = a.c.enc[0], yg = a.c.enc[1], yb = a.c.enc[2], ybias = (a.c.y_offset << YUV_SHIFT) + HALF;
    const int cbias = (128 << (YUV_SHIFT + 2)) + (1 << (YUV_SHIFT + 1));
    unsigned y0[2] = {0, 0}, y1[2] = {0, 0}, uu[1] = {0}, vv[1] = {0}, uv[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < STRIP / 2; ++k) {
        int rs = 0, gs = 0, bs = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int px = 2 * k + (j & 1);
            const unsigned* in = j < 2 ? i0 : i1;
            const int b = (int)byte_of(in, 3 * px), g = (int)byte_of(in, 3 * px + 1), r = (int)byte_of(in, 3 * px + 2);
            rs += r, gs += g, bs += b;
            const unsigned y = shift_clamp8<YUV_SHIFT>(yr * r + yg * g + yb * b + ybias);
            (j < 2 ? y0 : y1)[px >> 2] |= y << ((px & 3) * 8);
        }
        const unsigned u = shift_clamp8<YUV_SHIFT + 2>(a.c.enc[3] * rs + a.c.enc[4] * gs + a.c.enc[5] * bs + cbias);
        const unsigned v = shift_clamp8<YUV_SHIFT + 2>(a.c.enc[6] * rs + a.c.enc[7] * gs + a.c.enc[8] * bs + cbias);
        if (FMT == AIC_PIX_NV12) uv[k >> 1] |= (u | v << 8) << ((k & 1) * 16);
        else uu[0] |= u << (k * 8), vv[0] |= v << (k * 8);
    }
    store_words<YACC>(yp, n, y0);
    store_words<YACC>(yp + a.pitch, n, y1);
    if (FMT == AIC_PIX_NV12) store_words<YACC>(cu, n, uv);
    else store_words<CACC>(cu, n >> 1, uu), store_words<CACC>(cv, n >> 1, vv);
}

namespace {

int access_width(const void* yuv, const void* bgr, const YuvLayout& L) {
    const uintptr_t y = reinterpret_cast<uintptr_t>(yuv), b = reinterpret_cast<uintptr_t>(bgr);
    if (L.w % 8 || L.pitch % 8 || L.frame_stride % 8 || y % 8 || b % 4) return 1;
    return b % 8 ? 4 : 8;
}

template <class Launch>
void for_each_chunk(int n, Launch&& launch) {
    constexpr int MAXF = 32768;                              // frames per launch (grid.y)
    for (int f0 = 0; f0 < n; f0 += MAXF) launch(f0, std::min(MAXF, n - f0));
}

}  // namespace

#define AIC_YUV_DISPATCH(KERNEL, grid, s, a, fmt, acc)                                                         \
    do {                                                                                                       \
        if (fmt == AIC_PIX_NV12) {                                                                             \
            if (acc == 8) hipLaunchKernelGGL((KERNEL<AIC_PIX_NV12, 8>), grid, dim3(256), 0, s, a);            \
            else if (acc == 4) hipLaunchKernelGGL((KERNEL<AIC_PIX_NV12, 4>), grid, dim3(256), 0, s, a);       \
            else hipLaunchKernelGGL((KERNEL<AIC_PIX_NV12, 1>), grid, dim3(256), 0, s, a);                     \
        } else {                                                                                               \
            if (acc == 8) hipLaunchKernelGGL((KERNEL<AIC_PIX_I420, 8>), grid, dim3(256), 0, s, a);            \
            else if (acc == 4) hipLaunchKernelGGL((KERNEL<AIC_PIX_I420, 4>), grid, dim3(256), 0, s, a);       \
            else hipLaunchKernelGGL((KERNEL<AIC_PIX_I420, 1>), grid, dim3(256), 0, s, a);                     \
        }                                                                                                      \
        KCHECK();                                                                                              \
    } while (0)

void launch_yuv_to_bgr(const uint8_t* src, int n, const YuvLayout& L, const YuvCoeffs& c, uint8_t* dst_bgr, hipStream_t s) {
    const int acc = access_width(src, dst_bgr, L);
    for_each_chunk(n, [&](int f0, int k) {
        YuvArgs a{const_cast<uint8_t*>(src) + (size_t)f0 * L.frame_stride, dst_bgr + (size_t)f0 * L.h * L.w * 3, L.h, L.w, ceil_div(L.w, STRIP), L.pitch, L.frame_stride, c};
        const dim3 grid((unsigned)ceil_div((long)(L.h / 2) * a.strips, 256), (unsigned)k);
        AIC_YUV_DISPATCH(yuv_to_bgr_kernel, grid, s, a, L.format, acc);
    });
}

void launch_bgr_to_yuv(const uint8_t* src_bgr, int n, const YuvLayout& L, const YuvCoeffs& c, uint8_t* dst, hipStream_t s) {
    const int acc = access_width(dst, src_bgr, L);
    for_each_chunk(n, [&](int f0, int k) {
        YuvArgs a{dst + (size_t)f0 * L.frame_stride, const_cast<uint8_t*>(src_bgr) + (size_t)f0 * L.h * L.w * 3, L.h, L.w, ceil_div(L.w, STRIP), L.pitch, L.frame_stride, c};
        const dim3 grid((unsigned)ceil_div((long)(L.h / 2) * a.strips, 256), (unsigned)k);
        AIC_YUV_DISPATCH(bgr_to_yuv_kernel, grid, s, a, L.format, acc);
    });
}

}  // namespace aic
