// conv_common.hpp -- device helpers shared by the convolution translation units (kernels_conv*.hip): MFMA fragment
// types, the LDS swizzle, the channel permutation and the epilogues, LDS-DMA typedefs and counted waits; plus the
// launchers by which launch_conv_igemm() (kernels_conv.hip) reaches the kernels that live in the other units.
#pragma once
#include "kernels.hpp"
#include "pad_skip_map.hpp"

#include <cstdlib>
#include <type_traits>
#include <utility>

namespace aic {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float act_apply(float v, int act) {
    if (act == 1) return v / (1.0f + __expf(-v));   // SiLU
    if (act == 2) return fmaxf(v, 0.0f);             // ReLU
    return v;
}

template <typename T> struct Frag;
template <> struct Frag<half_t> {
    typedef half8 type;
    static __device__ __forceinline__ floatx4 mma(const half8& a, const half8& b, floatx4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Frag<float> {
    typedef floatx4 type;
    // Two-level summation (parity mode): the 16 products of one K-step are chained from zero and their sum joins the running
    // accumulator with one fp32 add.  A single chain over K = 576 .. 5 184 rounds K/4 times in sequence; this form rounds
    // 4 + K/16 times, which puts the fp32 engine ~4x closer to the fp64 evaluation of the same graph than a plain chain
    // (measured against oracle/nets_oracle.py in fp64: tests/test_gpu_nets.py, tests/test_gpu_configs.py).
    static __device__ __forceinline__ floatx4 partial(const floatx4& a, const floatx4& b) {
        floatx4 p = {0.f, 0.f, 0.f, 0.f};
        p = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], p, 0, 0, 0);
        p = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], p, 0, 0, 0);
        p = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], p, 0, 0, 0);
        p = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], p, 0, 0, 0);
        return p;
    }
    static __device__ __forceinline__ floatx4 mma(const floatx4& a, const floatx4& b, floatx4 c) { return c + partial(a, b); }
};

// acc[i][j] += w[j] x x[i] for one K-step of a wave's MT x NT tile grid.
// fp16: plain accumulating MFMAs.  fp32 (two-level summation): every tile's partial chain starts from zero and joins the
// accumulator with a VALU add.  Two things go wrong when that add is left to the compiler in the fully unrolled 3x3 kernels,
// whose accumulators have no use before the epilogue block: MachineSink moves the adds, link by link, down into the epilogue,
// so every partial of every K-step stays live (576 of them on the 4x4 patch kernel: 11 KB of scratch per lane, 8x slower);
// and the scheduler interleaves the independent chains.  Hence (1) an empty volatile asm on the accumulator after each add
// -- it cannot be sunk or reordered -- and (2) a pinned order: chain of tile t, then the add of tile t-1, whose MFMAs have
// retired by then; two partials live.
template <typename T, int MT, int NT>
__device__ __forceinline__ void mma_tiles(floatx4 (&acc)[MT][NT], const typename Frag<T>::type (&wf)[NT], const typename Frag<T>::type (&xf)[MT]) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = Frag<T>::mma(wf[j], xf[i], acc[i][j]);
    } else {
        floatx4 prev = Frag<T>::partial(wf[0], xf[0]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 1; t < MT * NT; ++t) {
            const floatx4 p = Frag<T>::partial(wf[t % NT], xf[t / NT]);
            acc[(t - 1) / NT][(t - 1) % NT] += prev;
            asm volatile("" : "+v"(acc[(t - 1) / NT][(t - 1) % NT]));
            prev = p;
            __builtin_amdgcn_sched_barrier(0);
        }
        acc[MT - 1][NT - 1] += prev;
        asm volatile("" : "+v"(acc[MT - 1][NT - 1]));
    }
}

// fp32, THREE-level summation (round 5; the LDS-DMA implicit GEMM, the only kernel fp32 engines run since): the partial chain of a K-step joins a
// MID-level accumulator; every MID_STEPS steps (256 products) the mid level joins the accumulator and restarts from zero.  Roundings in
// sequence for K = 5 184 (YOLOv8m's deepest 3x3): 4 + 16 (+ 21 at the top, in double: below) instead of the two-level form's 4 + 324 -- what brought YOLOv8m's
// boxes from 1.6e-3 to within 1e-3 px of the fp64 evaluation (north_star's bound).  Costs a second accumulator set.
constexpr int MID_STEPS = 16;
template <int MT, int NT>
__device__ __forceinline__ void mma_tiles_mid(floatx4 (&mid)[MT][NT], const floatx4 (&wf)[NT], const floatx4 (&xf)[MT]) {
    floatx4 prev = Frag<float>::partial(wf[0], xf[0]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 1; t < MT * NT; ++t) {
        const floatx4 p = Frag<float>::partial(wf[t % NT], xf[t / NT]);
        mid[(t - 1) / NT][(t - 1) % NT] += prev;
        asm volatile("" : "+v"(mid[(t - 1) / NT][(t - 1) % NT]));
        prev = p;
        __builtin_amdgcn_sched_barrier(0);
    }
    mid[MT - 1][NT - 1] += prev;
    asm volatile("" : "+v"(mid[MT - 1][NT - 1]));
}
// The TOP level was tried in double as well (two registers per output, tiles of at most 8 MFMA tiles): the same statistics -- YOLOv8m boxes
// against the fp64 evaluation, 33 600 coordinates: rms 5.3e-5 px, 99.9th percentile 5.2e-4, one or two coordinates above 1e-3 (max 1.05e-3 /
// 1.48e-3: which anchor it is changes with every rounding pattern) -- so what is left is the fp32 rounding of 83 layers of activations, not
// the accumulation.  fp32 it stays.
typedef float doublex4 __attribute__((ext_vector_type(4)));
template <int MT, int NT>
__device__ __forceinline__ void flush_mid(doublex4 (&accd)[MT][NT], floatx4 (&mid)[MT][NT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
#pragma unroll
            for (int e = 0; e < 4; ++e) accd[i][j][e] += mid[i][j][e];
            mid[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
}

// swz(row) = ((row>>1)&3) ^ ((row>>3)&2): conflict-free for 16 consecutive rows (pixel tiles, identity weight tiles) AND
// for the permuted weight rows {c + 8k + s} of perm_row() (brute-forced over the ds_read_b128 lane groups).
__device__ __forceinline__ int lds_swz(int row) { return ((row >> 1) & 3) ^ ((row >> 3) & 2); }
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 64 + 16 * (chunk ^ lds_swz(row)); }

// ---- shared by the v2 kernel: cheap index math and a specialised epilogue ------------------------
// m -> (m / d, m % d) with one reciprocal multiply and a +-1 fix-up (m < 2^26 here).
__device__ __forceinline__ void fast_divmod(int m, int d, float inv, int& q, int& r) {
    q = (int)(__int2float_rz(m) * inv);
    r = m - q * d;
    if (r >= d) { r -= d; ++q; }
    if (r < 0) { r += d; --q; }
}

template <int ACT> __device__ __forceinline__ float act_fast(float v) {
    if constexpr (ACT == 1) {   // SiLU = v * sigmoid(v); v_exp_f32 + v_rcp_f32 (<= 1 ulp each)
        return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
    } else if constexpr (ACT == 2) {
        return fmaxf(v, 0.0f);
    } else {
        return v;
    }
}

// fp32 engines (the parity mode: speed is irrelevant there) take SiLU with expf and an IEEE division: v_exp_f32(v * log2 e) rounds the
// product before the exponential -- |v| * 6e-8 of relative error, five ulps at |v| = 5 -- and 83 layers of it were a third of YOLOv8m's
// distance from the fp64 evaluation of the same graph (tools/v8m_err.py, round 5)
template <typename T, int ACT> __device__ __forceinline__ float act_t(float v) {
    if constexpr (sizeof(T) == 4 && ACT == 1) return v / (1.0f + expf(-v));
    else return act_fast<ACT>(v);
}

// One lane owns, per (i, j) tile, 4 consecutive output channels of one pixel.
// ACT / RES / F32OUT are compile-time so the unrolled body carries no branches.
template <typename T, int MT, int NT, int ACT, int RES, bool F32OUT>
__device__ __forceinline__ void epilogue_fast(const ConvArgs& a, floatx4 (&acc)[MT][NT], const int (&mrow)[MT], int n_base, int q) {
    const float* __restrict__ bias = a.bias;
    const T* __restrict__ rg = reinterpret_cast<const T*>(a.res);
    floatx4 b4[NT];
    bool ncol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n_base + j * 16 + 4 * q;
        ncol[j] = n < a.Cout;                       // Cout % 4 == 0 on this path: all four or none
        b4[j] = *reinterpret_cast<const floatx4*>(bias + n);   // bias is padded to cout_pad
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = mrow[i];
        if (m < 0) continue;
        const size_t ybase = (size_t)m * a.y_cs + a.y_coff;
        const size_t rbase = RES ? (size_t)m * a.r_cs + a.r_coff : 0;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            if (!ncol[j]) continue;
            const int n = n_base + j * 16 + 4 * q;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + b4[j][e];
            if constexpr (RES != 0) {
                float rv[4];
                if constexpr (sizeof(T) == 2) {
                    const half4 h = *reinterpret_cast<const half4*>(rg + rbase + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) rv[e] = (float)h[e];
                } else {
                    const floatx4 h = *reinterpret_cast<const floatx4*>(rg + rbase + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) rv[e] = h[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = RES == 1 ? act_t<T, ACT>(v[e] + rv[e]) : act_t<T, ACT>(v[e]) + rv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = act_t<T, ACT>(v[e]);
            }
            if constexpr (F32OUT || sizeof(T) == 4) {
                *reinterpret_cast<floatx4*>(reinterpret_cast<float*>(a.y) + ybase + n) = floatx4{v[0], v[1], v[2], v[3]};
            } else {
                const half4 h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                *reinterpret_cast<half4*>(reinterpret_cast<half_t*>(a.y) + ybase + n) = h;
            }
        }
    }
}

// Channel permutation of the v2+ kernels: MFMA tile j, row rho (= 4q + e on the output side) of a wave's
// NT-tile channel block carries output channel  32*(j>>1) + 8*(rho>>2) + 4*(j&1) + (rho&3)  (tiles taken in
// pairs; an odd last tile keeps the identity 16j + rho).  A lane (r, q) then owns, per tile pair, EIGHT
// consecutive channels of its pixel: one 16-byte fp16 store (two for fp32) instead of two 8-byte ones, and
// the four q-lanes of a pixel write 64 contiguous bytes per instruction.  The A-operand (weight) rows are
// fetched from LDS through the same map (perm_row), so the arithmetic per output is unchanged.
template <int NT> __device__ __forceinline__ int perm_ch(int j, int q, int e) {
    return j < (NT & ~1) ? 32 * (j >> 1) + 8 * q + 4 * (j & 1) + e : 16 * j + 4 * q + e;
}
template <int NT> __device__ __forceinline__ int perm_row(int j, int r) { return perm_ch<NT>(j, r >> 2, r & 3); }

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N-1>{})
template <typename F, int... I> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// fp16 output of whole tile pairs in PHASES, four or eight vectors at a time: their residual vectors are requested first (independent 16-byte
// loads), then the eight output vectors are formed, then all eight are stored.  Written tile by tile (load -> add -> activate -> store) the compiler reuses
// one set of data registers for every store and one for every residual and fences each reuse with s_waitcnt vmcnt(0) (stores count
// in vmcnt on gfx950): 16 exposed store round trips per wave and, with a residual, 16 exposed load round trips on top -- the
// 4.2 us (7.7 us with residual) a 512 x 128 tile spent after its last MFMA.  Same arithmetic, same roundings.
template <int MT, int NT, int ACT, int RES>
__device__ __forceinline__ void epilogue_wide_phased(const ConvArgs& a, floatx4 (&acc)[MT][NT], const int (&mrow)[MT], int n_base, int q) {
    constexpr int NP = NT / 2, ODD = NT & 1, NV = NP + ODD;                  // vectors per pixel tile: NP of 8 channels (+ one of 4 for an odd last tile)
    // vectors per pass: 4 where the accumulators alone take 128 VGPRs.  (With a residual the tile spends 9.8 us after its last MFMA instead
    // of 3.8 -- AICAM_PP_TIMES; requesting all MT * NV residual vectors at once changes nothing, 9.2 us: it is not four exposed round
    // trips but the 128 KB themselves, which a CU pulls from HBM at ~22 GB/s; from an L2-resident address the same tile takes 4.7 us.)
    constexpr int VPP = (MT * NT >= 32) ? 4 : 8;
    constexpr int MC = (MT * NV > VPP) ? (VPP / NV > 0 ? VPP / NV : 1) : MT;  // pixel tiles per pass
    static_assert(MT % MC == 0, "whole passes");
    const float* __restrict__ bias = a.bias;
    const half_t* __restrict__ rg = reinterpret_cast<const half_t*>(a.res);
    half_t* __restrict__ yg = reinterpret_cast<half_t*>(a.y);
    floatx4 b4[NT];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int n = n_base + 32 * p + 8 * q;
        b4[2 * p] = *reinterpret_cast<const floatx4*>(bias + n);          // bias is padded to cout_pad
        b4[2 * p + 1] = *reinterpret_cast<const floatx4*>(bias + n + 4);
    }
    const int n_odd = n_base + 16 * (NT - 1) + 4 * q;                       // the odd last tile keeps the identity map: 4 channels per lane
    if constexpr (ODD) b4[NT - 1] = *reinterpret_cast<const floatx4*>(bias + n_odd);
    // With a residual the passes are software-pipelined: the residual vectors of pass k + 1 are requested BEFORE the stores of pass k are
    // issued.  Requested after them (the form before), their s_waitcnt had the four stores in front of it in the in-order vmcnt queue: every
    // pass paid a store acknowledge plus a load round trip, ~2 us x 4 passes -- the 8.4 us a 512 x 128 tile spent here even with its residual
    // already in the L2 (AICAM_PP_TIMES, conv3x3_pp_patch_kernel's prefetch), against 3.9 us without a residual.
    half8 rq[2][MC][NP > 0 ? NP : 1];
    half4 rq4[2][MC];
    auto request = [&](int i0, auto setc) {                // rows past the end / channels past Cout read a valid address (row 0; the pixel's
        constexpr int S = decltype(setc)::value;           // last channels) and are never stored
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const size_t rbase = (size_t)max(mrow[i0 + i], 0) * a.r_cs + a.r_coff;
#pragma unroll
            for (int p = 0; p < NP; ++p) rq[S][i][p] = *reinterpret_cast<const half8*>(rg + rbase + min(n_base + 32 * p + 8 * q, a.Cout - 8));
            if constexpr (ODD) rq4[S][i] = *reinterpret_cast<const half4*>(rg + rbase + min(n_odd, a.Cout - 4));
        }
    };
    if constexpr (RES != 0) request(0, std::integral_constant<int, 0>{});
    static_for<MT / MC>([&](auto passc) {
        constexpr int PASS = decltype(passc)::value, i0 = PASS * MC, S = PASS & 1;
        half8 o[MC][NP > 0 ? NP : 1];
        half4 o4[MC];
        if constexpr (RES != 0) {
            if constexpr (PASS + 1 < MT / MC) {
                request(i0 + MC, std::integral_constant<int, S ^ 1>{});
                __builtin_amdgcn_sched_barrier(0);         // (the requests stay in front of this pass's arithmetic and stores)
            }
#pragma unroll
            for (int i = 0; i < MC; ++i) {
#pragma unroll
                for (int p = 0; p < NP; ++p) o[i][p] = rq[S][i][p];
                if constexpr (ODD) o4[i] = rq4[S][i];
            }
        }
#pragma unroll
        for (int i = 0; i < MC; ++i) {
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = acc[i0 + i][2 * p + (e >> 2)][e & 3] + b4[2 * p + (e >> 2)][e & 3];
                if constexpr (RES != 0) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = RES == 1 ? act_fast<ACT>(v[e] + (float)o[i][p][e]) : act_fast<ACT>(v[e]) + (float)o[i][p][e];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = act_fast<ACT>(v[e]);
                }
                o[i][p] = half8{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3], (half_t)v[4], (half_t)v[5], (half_t)v[6], (half_t)v[7]};
            }
            if constexpr (ODD) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i0 + i][NT - 1][e] + b4[NT - 1][e];
                if constexpr (RES != 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = RES == 1 ? act_fast<ACT>(v[e] + (float)o4[i][e]) : act_fast<ACT>(v[e]) + (float)o4[i][e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_fast<ACT>(v[e]);
                }
                o4[i] = half4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
            }
        }
        // every output vector of the pass exists, in registers of its own, BEFORE its first store: left to itself the compiler sinks each
        // vector's arithmetic into its store's predicated block and recycles one set of data registers, one s_waitcnt vmcnt(0) per store
#pragma unroll
        for (int i = 0; i < MC; ++i) {
#pragma unroll
            for (int p = 0; p < NP; ++p) asm volatile("" : "+v"(o[i][p]));
            if constexpr (ODD) asm volatile("" : "+v"(o4[i]));
        }
#pragma unroll
        for (int i = 0; i < MC; ++i) {
            const int m = mrow[i0 + i];
            const size_t ybase = (size_t)max(m, 0) * a.y_cs + a.y_coff;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int n = n_base + 32 * p + 8 * q;
                if (m >= 0 && n < a.Cout) *reinterpret_cast<half8*>(yg + ybase + n) = o[i][p];
            }
            if constexpr (ODD) {
                if (m >= 0 && n_odd < a.Cout) *reinterpret_cast<half4*>(yg + ybase + n_odd) = o4[i];
            }
        }
    });
}

// PHASED: only the 8-wave kernels ask for it.  They run one block per CU whatever their register count; in the 4-wave kernels the
// extra live vectors cost occupancy (256 px x 64 ch tile: 240 -> 272 registers = one wave per SIMD instead of two, and YOLOv8n's
// thin 1x1 layers ran 7 - 30 % slower: profiles/r03, first refresh).
template <typename T, int MT, int NT, int ACT, int RES, bool F32OUT, bool PHASED = false>
__device__ __forceinline__ void epilogue_wide(const ConvArgs& a, floatx4 (&acc)[MT][NT], const int (&mrow)[MT], int n_base, int q) {
    if constexpr (PHASED && sizeof(T) == 2 && !F32OUT) {
        epilogue_wide_phased<MT, NT, ACT, RES>(a, acc, mrow, n_base, q);
        return;
    }
    constexpr int NP = NT / 2;
    const float* __restrict__ bias = a.bias;
    const T* __restrict__ rg = reinterpret_cast<const T*>(a.res);
    floatx4 b4[NT];
    bool pcol[NP + 1];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int n = n_base + 32 * p + 8 * q;
        pcol[p] = n < a.Cout;                       // Cout % 8 == 0 on this path: all eight or none
        b4[2 * p] = *reinterpret_cast<const floatx4*>(bias + n);          // bias is padded to cout_pad
        b4[2 * p + 1] = *reinterpret_cast<const floatx4*>(bias + n + 4);
    }
    if constexpr (NT & 1) {
        const int n = n_base + 16 * (NT - 1) + 4 * q;
        pcol[NP] = n < a.Cout;
        b4[NT - 1] = *reinterpret_cast<const floatx4*>(bias + n);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = mrow[i];
        if (m < 0) continue;
        const size_t ybase = (size_t)m * a.y_cs + a.y_coff;
        const size_t rbase = RES ? (size_t)m * a.r_cs + a.r_coff : 0;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (!pcol[p]) continue;
            const int n = n_base + 32 * p + 8 * q;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = acc[i][2 * p + (e >> 2)][e & 3] + b4[2 * p + (e >> 2)][e & 3];
            if constexpr (RES != 0) {
                float rv[8];
                if constexpr (sizeof(T) == 2) {
                    const half8 h = *reinterpret_cast<const half8*>(rg + rbase + n);
#pragma unroll
                    for (int e = 0; e < 8; ++e) rv[e] = (float)h[e];
                } else {
                    const floatx4 h0 = *reinterpret_cast<const floatx4*>(rg + rbase + n);
                    const floatx4 h1 = *reinterpret_cast<const floatx4*>(rg + rbase + n + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { rv[e] = h0[e]; rv[4 + e] = h1[e]; }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = RES == 1 ? act_t<T, ACT>(v[e] + rv[e]) : act_t<T, ACT>(v[e]) + rv[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = act_t<T, ACT>(v[e]);
            }
            if constexpr (F32OUT || sizeof(T) == 4) {
                float* yp = reinterpret_cast<float*>(a.y) + ybase + n;
                *reinterpret_cast<floatx4*>(yp) = floatx4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<floatx4*>(yp + 4) = floatx4{v[4], v[5], v[6], v[7]};
            } else {
                const half8 h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3], (half_t)v[4], (half_t)v[5], (half_t)v[6], (half_t)v[7]};
                *reinterpret_cast<half8*>(reinterpret_cast<half_t*>(a.y) + ybase + n) = h;
            }
        }
        if constexpr (NT & 1) {
            if (pcol[NP]) {
                constexpr int j = NT - 1;
                const int n = n_base + 16 * j + 4 * q;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + b4[j][e];
                if constexpr (RES != 0) {
                    float rv[4];
                    if constexpr (sizeof(T) == 2) {
                        const half4 h = *reinterpret_cast<const half4*>(rg + rbase + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) rv[e] = (float)h[e];
                    } else {
                        const floatx4 h = *reinterpret_cast<const floatx4*>(rg + rbase + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) rv[e] = h[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = RES == 1 ? act_t<T, ACT>(v[e] + rv[e]) : act_t<T, ACT>(v[e]) + rv[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_t<T, ACT>(v[e]);
                }
                if constexpr (F32OUT || sizeof(T) == 4) {
                    *reinterpret_cast<floatx4*>(reinterpret_cast<float*>(a.y) + ybase + n) = floatx4{v[0], v[1], v[2], v[3]};
                } else {
                    const half4 h = {(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
                    *reinterpret_cast<half4*>(reinterpret_cast<half_t*>(a.y) + ybase + n) = h;
                }
            }
        }
    }
}

// Generic (any Cout, any mode) fallback: runtime branches, scalar tail.
template <typename T, int MT, int NT, bool PERM>
__device__ __forceinline__ void epilogue_generic(const ConvArgs& a, floatx4 (&acc)[MT][NT], const int (&mrow)[MT], int n_base, int q) {
    // (inlined and fully unrolled on purpose: a call would force `a` and `acc` into scratch memory)
    const float* __restrict__ bias = a.bias;
    const T* __restrict__ rg = reinterpret_cast<const T*>(a.res);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = mrow[i];
        if (m < 0) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n_base + (PERM ? perm_ch<NT>(j, q, 0) : j * 16 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (n + e >= a.Cout) continue;
                float x = acc[i][j][e] + bias[n + e];
                const float rv = a.res_mode ? (float)rg[(size_t)m * a.r_cs + a.r_coff + n + e] : 0.f;
                if (a.res_mode == 1) x += rv;
                x = act_apply(x, a.act);
                if (a.res_mode == 2) x += rv;
                const size_t yo = (size_t)m * a.y_cs + a.y_coff + n + e;
                if (a.out_f32 || sizeof(T) == 4) reinterpret_cast<float*>(a.y)[yo] = x;
                else reinterpret_cast<half_t*>(a.y)[yo] = (half_t)x;
            }
        }
    }
}

template <typename T, int MT, int NT, bool PERM = false, bool PHASED = false>
__device__ __forceinline__ void epilogue_dispatch(const ConvArgs& a, floatx4 (&acc)[MT][NT], const int (&mrow)[MT], int n_base, int q) {
    const int key = (a.Cout & (PERM ? 7 : 3)) ? -1 : (a.act | (a.res_mode << 2) | (a.out_f32 << 4));
#define AIC_EPI(ACT, RES, F32) do { if constexpr (PERM) epilogue_wide<T, MT, NT, ACT, RES, F32, PHASED>(a, acc, mrow, n_base, q); \
                                    else epilogue_fast<T, MT, NT, ACT, RES, F32>(a, acc, mrow, n_base, q); } while (0)
    switch (key) {
        case 1: AIC_EPI(1, 0, false); break;             // SiLU
        case 1 | (2 << 2): AIC_EPI(1, 2, false); break;  // SiLU then +res (C2f bottleneck)
        case 2: AIC_EPI(2, 0, false); break;             // ReLU
        case 2 | (1 << 2): AIC_EPI(2, 1, false); break;  // relu(x + res) (BasicBlock)
        case 0: AIC_EPI(0, 0, false); break;             // linear (downsample, FC)
        case 0 | (1 << 4): AIC_EPI(0, 0, true); break;   // linear fp32 (detect head)
        default: epilogue_generic<T, MT, NT, PERM>(a, acc, mrow, n_base, q); break;
    }
#undef AIC_EPI
}

// ---- a 1x1 conv in the epilogue of the conv before it (ConvArgs::w_tail; fp16) -----------------------------------------
// For a wave that owns ALL channels of its pixels (WN == 1, Cout == 16 NT) the permuted accumulator layout IS the B operand of
// the next conv: after bias + SiLU + rounding to fp16 -- exactly what the conv would have stored -- lane (r, q) holds, per tile
// pair p, channels 32 p + 8 q .. + 7 of pixel r, i.e. K elements 8 q .. 8 q + 7 of K-step p.  No LDS round trip, no HBM round
// trip.  An odd last tile (Cout = 80: channels 64 .. 79) holds 4 channels per lane; K-step NP wants 8 (64 + 8 q .. + 7) from
// lanes (r, 2 q) and (r, 2 q + 1): four ds_bpermute per pixel tile, zeros for q >= 2 (the K padding 80 .. 95).
// The 1x1's weights come straight from L2 as A fragments (row perm_row(j2, r), K elements 32 s + 8 q .. + 7), once per wave.
// Same products, same K-step order, same roundings as the two kernels run one after the other: bit-identical outputs
// (tests/test_gpu_nets.py::test_fused_head_tail).
template <int MT, int NT>
__device__ __forceinline__ void tail_1x1(const ConvArgs& a, floatx4 (&acc)[MT][NT], const int (&mrow)[MT], int lane) {
    constexpr int NP = NT / 2, KS = NP + (NT & 1);
    const int r = lane & 15, q = lane >> 4;
    // the loads below depend on nothing the K loop computes: without this fence the scheduler hoists them into the (fully
    // unrolled) loop, where they stay live to the end -- 182 -> 278 registers on the patch kernel, 2 -> 1 waves per SIMD
    __builtin_amdgcn_sched_barrier(0);
    const half_t* __restrict__ wt = reinterpret_cast<const half_t*>(a.w_tail);
    half8 wf[NT][KS];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int s = 0; s < KS; ++s) wf[j][s] = *reinterpret_cast<const half8*>(wt + (size_t)perm_row<NT>(j, r) * a.t_kp + 32 * s + 8 * q);
    floatx4 b1[NT];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        b1[2 * p] = *reinterpret_cast<const floatx4*>(a.bias + 32 * p + 8 * q);
        b1[2 * p + 1] = *reinterpret_cast<const floatx4*>(a.bias + 32 * p + 8 * q + 4);
    }
    if constexpr (NT & 1) b1[NT - 1] = *reinterpret_cast<const floatx4*>(a.bias + 16 * (NT - 1) + 4 * q);
    ConvArgs a2 = a;                       // the tail's epilogue: its own bias / activation / output, no residual
    a2.y = a.y_tail, a2.bias = a.b_tail, a2.Cout = a.t_cout, a2.y_cs = a.t_y_cs, a2.y_coff = a.t_y_coff;
    a2.act = a.t_act, a2.res_mode = 0, a2.out_f32 = a.t_out_f32;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        half8 bf[KS];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int e = 0; e < 8; ++e) bf[p][e] = (half_t)act_fast<1>(acc[i][2 * p + (e >> 2)][e & 3] + b1[2 * p + (e >> 2)][e & 3]);
        if constexpr (NT & 1) {
            half4 own;
#pragma unroll
            for (int e = 0; e < 4; ++e) own[e] = (half_t)act_fast<1>(acc[i][NT - 1][e] + b1[NT - 1][e]);
            const int2 u = *reinterpret_cast<const int2*>(&own);
            const int s0 = (((2 * q) & 3) * 16 + r) * 4, s1 = (((2 * q + 1) & 3) * 16 + r) * 4;
            int4 g;
            g.x = __builtin_amdgcn_ds_bpermute(s0, u.x), g.y = __builtin_amdgcn_ds_bpermute(s0, u.y);
            g.z = __builtin_amdgcn_ds_bpermute(s1, u.x), g.w = __builtin_amdgcn_ds_bpermute(s1, u.y);
            if (q >= 2) g = make_int4(0, 0, 0, 0);
            bf[NP] = *reinterpret_cast<const half8*>(&g);
        }
        floatx4 acc2[1][NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc2[0][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc2[0][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j][s], bf[s], acc2[0][j], 0, 0, 0);
        const int m1[1] = {mrow[i]};
        if (a.t_max) {
            // class reduction (ConvArgs::t_max): lane (r, q) holds 4 NT channels of pixel r, in ascending order when walked (j, e); the
            // four q-lanes of the pixel meet by two xor-shuffles.  Larger value wins, equal values: the lower channel (first maximum)
            // (the tail's bias is fetched HERE, per pixel tile, behind the MFMAs just issued: their ~400 cycles cover the L1 round trip,
            //  and twenty registers carried through the tile loop would cost the lead kernels a wave per SIMD)
            floatx4 bt[NT];
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                bt[2 * p] = *reinterpret_cast<const floatx4*>(a.b_tail + 32 * p + 8 * q);
                bt[2 * p + 1] = *reinterpret_cast<const floatx4*>(a.b_tail + 32 * p + 8 * q + 4);
            }
            if constexpr (NT & 1) bt[NT - 1] = *reinterpret_cast<const floatx4*>(a.b_tail + 16 * (NT - 1) + 4 * q);
            float best = -__builtin_inff();
            int arg = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int ch = perm_ch<NT>(j, q, e);
                    const float v = acc2[0][j][e] + bt[j][e];              // (linear, fp32: the value the store would have written)
                    if (ch < a.t_cout && v > best) { best = v; arg = ch; }
                }
#pragma unroll
            for (int off = 16; off <= 32; off <<= 1) {
                const float ov = __shfl_xor(best, off);
                const int oa = __shfl_xor(arg, off);
                if (ov > best || (ov == best && oa < arg)) { best = ov; arg = oa; }
            }
            const int m = mrow[i];
            if (q == 0 && m >= 0) {
                const int im = m / a.t_hw;
                const size_t o = (size_t)im * a.t_na + a.t_a0 + (m - im * a.t_hw);
                a.t_max[o] = best;
                a.t_arg[o] = arg;
            }
        } else if (NT == 4 && a.t_box) {
            // box decode (ConvArgs::t_box).  Lane (r, q) holds bins 8 (q & 1) .. + 7 of side q >> 1 (tiles 0, 1) and of side 2 + (q >> 1)
            // (tiles 2, 3); its partner q ^ 1 holds the other eight.  decode_kernel's order is kept exactly: the maximum of the sixteen
            // (exact in any order), then e_k = exp(v_k - max) (v_exp_f32 of the product with log2 e: decode_kernel's fp16 form), sum += e_k, ex += e_k * k for k = 0 .. 15 IN THAT ORDER -- the even lane
            // runs bins 0 .. 7 from zero, hands its two running sums to the odd lane, which continues with 8 .. 15 and divides.
            if constexpr (NT == 4) {
                floatx4 bt[4];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    bt[2 * p] = *reinterpret_cast<const floatx4*>(a.b_tail + 32 * p + 8 * q);
                    bt[2 * p + 1] = *reinterpret_cast<const floatx4*>(a.b_tail + 32 * p + 8 * q + 4);
                }
                const bool odd = q & 1;
                float dist[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {                            // h = 0: side q >> 1, h = 1: side 2 + (q >> 1)
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = acc2[0][2 * h + (k >> 2)][k & 3] + bt[2 * h + (k >> 2)][k & 3];
                    float mx = v[0];
#pragma unroll
                    for (int k = 1; k < 8; ++k) mx = fmaxf(mx, v[k]);
                    mx = fmaxf(mx, __shfl_xor(mx, 16));
                    float e[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) e[k] = __builtin_amdgcn_exp2f((v[k] - mx) * 1.4426950408889634f);   // (DetArgs::fast_exp: decode_kernel's form for fp16 engines -- 64 expf per lane and pixel tile were a third of the box tails' time)
                    float sum = 0.f, ex = 0.f;
                    if (!odd) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) { sum += e[k]; ex += e[k] * (float)k; }
                    }
                    const float s_in = __shfl_xor(sum, 16), x_in = __shfl_xor(ex, 16);
                    if (odd) {
                        sum = s_in, ex = x_in;
#pragma unroll
                        for (int k = 0; k < 8; ++k) { sum += e[k]; ex += e[k] * (float)(8 + k); }
                    }
                    dist[h] = ex / sum;                                  // (meaningful in odd lanes)
                }
                // lane q = 1 holds sides 0 and 2, lane q = 3 sides 1 and 3: q = 1 fetches the other two and stores the box
                const float d1 = __shfl_xor(dist[0], 32), d3 = __shfl_xor(dist[1], 32);
                const int m = mrow[i];
                if (q == 1 && m >= 0) {
                    const int im = m / a.t_hw, cell = m - im * a.t_hw;
                    const int gy = cell / a.t_w, gx = cell - gy * a.t_w;
                    const float cx = (float)gx + 0.5f, cy = (float)gy + 0.5f, st = (float)a.t_stride;
                    const size_t o = (size_t)im * a.t_na + a.t_a0 + cell;
                    *reinterpret_cast<floatx4*>(a.t_box + o * 4) = floatx4{(cx - dist[0]) * st, (cy - d1) * st, (cx + dist[1]) * st, (cy + d3) * st};
                }
            }
        } else {
            epilogue_dispatch<half_t, 1, NT, true>(a2, acc2, m1, 0, q);
        }
    }
}

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;


// Workgroups go to the 8 XCDs round-robin (block b -> XCD b % 8), each with its own L2.  Tiles that are neighbours in the
// image share halo rows and weights: this bijection gives XCD x one contiguous run of tiles, so a halo fetched by one block is an
// L2 hit for the next instead of a second HBM / Infinity-Cache read through another XCD.  (on = 0: identity)
__device__ __forceinline__ int xcd_tile(int b, int nb, int on) {
    if (!on) return b;
    const int x = b & 7, base = nb >> 3, rem = nb & 7;
    return x * base + (x < rem ? x : rem) + (b >> 3);
}
// linear block id -> (tile x, tile y) of a gridDim.x x gridDim.y tile grid
__device__ __forceinline__ void xcd_tile_xy(int on, int& bx, int& by) {
    const int nbx = (int)gridDim.x, lin = (int)blockIdx.y * nbx + (int)blockIdx.x;
    const int t = xcd_tile(lin, nbx * (int)gridDim.y, on);
    by = t / nbx, bx = t - by * nbx;
}
// The same when only the first nbx_live <= gridDim.x tile columns hold items (the grid was sized for a bound and the count is
// read on the device, ConvArgs::n_dev): the live tiles are dealt to the first nbx_live * gridDim.y blocks -- XCD-contiguous runs
// of LIVE tiles, all eight XCDs busy -- and the other blocks leave (false).  nbx_live == gridDim.x: exactly xcd_tile_xy above.
__device__ __forceinline__ bool xcd_tile_xy_live(int on, int nbx_live, int& bx, int& by) {
    const int lin = (int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x;
    const int nlive = nbx_live * (int)gridDim.y;
    if (lin >= nlive) return false;
    const int t = xcd_tile(lin, nlive, on);
    by = t / nbx_live, bx = t - by * nbx_live;
    return true;
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
    if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 9) asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
    else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if constexpr (N == 11) asm volatile("s_waitcnt vmcnt(11)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if constexpr (N == 14) asm volatile("s_waitcnt vmcnt(14)" ::: "memory");
    else if constexpr (N == 15) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
    else if constexpr (N == 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if constexpr (N == 18) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
    else if constexpr (N == 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else static_assert(N < 0, "add this vmcnt literal");
}


// ---- shared by the patch kernels of kernels_conv_pp.hip / kernels_conv_sp.hip
constexpr int ppp_ipix_pad(int th, int tw) {
    int ipix = (th + 2) * (tw + 2);
    if (tw >= 16) return ipix;
    while (ipix % 16 != tw && ipix % 16 != 16 - tw) ++ipix;
    return ipix;
}

// Patch geometry and halo skipping of the software-pipelined patch kernel's 16-pixel MFMA tiles (MT tiles per wave, WM wave rows, NI
// images per block):
//   row pieces  a tile is whole rows or a piece of ONE row of 16 / TW images (pitch TW + 2); every tap of every tile is issued
//   COL         a tile is ONE column of 16 / TH images (pad_skip_map.hpp: odd pitch); the tiles of column 0 read only the halo at the
//               taps kw = 0, those of column TW - 1 at kw = 2 -- 2 / TW of the tiles x 1 / 3 of the taps issue no MFMA, read no fragment
// A skipped (tile, tap) has an all-zero pixel fragment and finite weights: each of its MFMAs would add +-0 to an accumulator that
// started at +0 and, under round-to-nearest, can never have become -0 -- C + 0 = C bit for bit.  The implicit-GEMM kernels and v5 still
// execute those MFMAs, so the bit-equality across kernel families (tests/test_gpu_nets.py) checks exactly this.
template <int TH, int TW, int NI, int WM, int MT, bool COL> struct PatchGeom {
    static constexpr int PW = TW + 2, IPIXP = ppp_ipix_pad(TH, TW);
    static constexpr bool skip(int, int) { return false; }
};
template <int TH, int TW, int NI, int WM, int MT> struct PatchGeom<TH, TW, NI, WM, MT, true> : ColTiles<TH, TW, NI, WM, MT> {};

// X2 (ConvArgs::x2: a 1x1 / stride-s conv of a second tensor accumulated into the same outputs -- a ResNet downsample branch folded into
// the block's last conv): the second source's channel chunk e (BM pixels x one K-step) sits in a buffer of its own behind the weight ring.
// It streams in during the window's chunk e in the LDS-DMA slots that carry no patch pass (taps 6 .. 8; the 512-pixel tile needs four
// passes, two of them at tap 6, whose counted wait is one higher) and is consumed by ONE extra step right after tap (0, 0) of chunk e + 1:
// the last pass is issued in L(tap 8), waited for in L(tap 0), read in L(extra) -- the usual two segments; the buffer is refilled from
// tap 6 on, five steps after it was read.  The implicit-GEMM kernels walk the same order (set_tap / xs there).
// lane id worked out on the spot (two v_mbcnt) and opaque to the optimiser: values derived from it inside the K loop are computed where
// they are used instead of being carried through the loop in registers the 512 x 128 tile does not have
__device__ __forceinline__ int lane_here() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}


// ---- the launchers of the other conv units: each launches the instantiation a plan of its form names (plan_conv, conv_plan.hpp)
void launch_conv_wide(const ConvArgs& a, const ConvPlan& p, hipStream_t s);          // kernels_conv_wide.hip
void launch_conv_pp(const ConvArgs& a, const ConvPlan& p, hipStream_t s);            // kernels_conv_pp.hip
void launch_conv_pp_patch(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
void launch_conv_sp_patch(const ConvArgs& a, const ConvPlan& p, hipStream_t s);      // kernels_conv_sp.hip
void launch_conv_s2_patch(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
void launch_conv_patch(const ConvArgs& a, const ConvPlan& p, hipStream_t s);         // kernels_conv_direct.hip
void launch_conv_pm_patch(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
void launch_conv_c16(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
void launch_conv_c32s2_tail(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
void launch_conv_1x1_stream(const ConvArgs& a, const ConvPlan& p, hipStream_t s);
void launch_conv_c64_resident(const ConvArgs& a, const ConvPlan& p, hipStream_t s);

}  // namespace aic
