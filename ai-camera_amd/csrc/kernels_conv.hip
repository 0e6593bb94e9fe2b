// kernels_conv.hip -- implicit-GEMM convolution on the gfx950 matrix cores + the small graph ops.
//
// conv_igemm: NHWC activations, weights packed [Cout][kh][kw][cin] so both GEMM operands are
// contiguous along K.  GEMM view: D[cout][pixel] = sum_k W[cout][k] * X[pixel][k] with
// K = kh*kw*cin walked tap-major; the MFMA "A" operand is the weight tile and the "B" operand
// the gathered pixel tile, so each lane ends up with 4 CONSECUTIVE output channels of one
// pixel (row = 4*(lane>>4)+i, col = lane&15 of v_mfma_f32_16x16x*) and the epilogue stores
// them as one 8-byte (fp16) / 16-byte (fp32) NHWC vector: no transpose through LDS.
//
//   fp16 mode: v_mfma_f32_16x16x32_f16, fp32 accumulate  (throughput mode)
//   fp32 mode: v_mfma_f32_16x16x4_f32, exact fp32 fmaf chain (parity mode)
//
// Per K-step each tile row holds 64 B (32 halves / 16 floats).  LDS image: row*64 +
// 16*(chunk ^ ((row>>1)&3)) -- an XOR swizzle that is conflict-free for the ds_read_b128
// lane groups of gfx950 (checked exhaustively against the group table of
// MI355X_MICROARCH.md §LDS).
#include "conv_common.hpp"

namespace aic {

// ------------------------------------------------------------------------------------------------
// v2: the tiling and MFMA mapping above; the operand tiles travel HBM/L2 -> LDS by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPR staging and no ds_write pass) into an
// NSTAGE-deep ring, NSTAGE-1 K-steps in flight.  Per K-step: counted s_waitcnt vmcnt (never 0 in
// the loop) -> one raw s_barrier -> issue the loads of step+NSTAGE-1 -> MFMAs of the current step.
//  * the LDS image of a wave-instruction must be lane-linear, so the XOR swizzle is applied to the
//    SOURCE: the thread that fills LDS slot s of row r fetches K-chunk s ^ ((r>>1)&3)
//    (cdna_hip_programming.md §5.4 rule 21); the ds_read side uses the same involution;
//  * zero padding / image borders / K tail / rows past M or Cout: the lane's source address is a
//    64-byte page of zeros in HBM, so every wave issues exactly LPS loads per stage and the vmcnt
//    arithmetic is uniform (also in the drain iterations, which load zeros nobody reads);
//  * im2col address = per-row base pointer + one per-thread tap offset; in-bounds is a precomputed
//    bit per (row, tap).
//  * TAIL: the conv's output feeds a 1x1 conv (a.w_tail) that runs in this kernel's epilogue (tail_1x1, conv_common.hpp)
//  * LIST: GEMM row m stands for output pixel a.pix_list[m] of the full map (ConvArgs::pix_list), the first a.pix_count[0] rows are live.
//    Only the row set-up and the epilogue's pixel indices know: a row's im2col base, its tap-validity bits, its stores and its tail's
//    anchor are those of its own pixel, wherever its tile neighbours lie; K walk, zero page and MFMA sequence are the dense kernel's
template <typename T, int MT, int NT, int WM, int WN, int NSTAGE, bool TAIL = false, bool LIST = false>
__global__ __launch_bounds__(64 * WM * WN) void conv_igemm_dma_kernel(const ConvArgs a) {
    constexpr int CH = 16 / (int)sizeof(T);
    constexpr int BKE = 4 * CH;
    constexpr int NTHR = 64 * WM * WN;         // 4 or 8 waves
    constexpr int RP = NTHR / 4;               // tile rows staged per pass (one 16-byte chunk per thread)
    constexpr int BM = WM * MT * 16;
    constexpr int BN = WN * NT * 16;
    constexpr int BNP = (BN + RP - 1) / RP * RP;   // weight rows padded so every wave issues the same loads
    constexpr int A_PER = BM / RP;
    constexpr int B_PER = BNP / RP;
    constexpr int LPS = A_PER + B_PER;         // LDS-DMA instructions per stage per wave
    constexpr int STAGE = (BM + BNP) * 64;
    static_assert((WM * WN == 4 || WM * WN == 8) && BM % RP == 0 && NSTAGE >= 2, "geometry");

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int t = threadIdx.x;
    const int lane = t & 63, wv = t >> 6;
    const int slot = t & 3, r0 = t >> 2;
    const int kc = slot ^ lds_swz(r0);         // K-chunk this thread fetches (source-side swizzle)
    const int Mmap = a.n_dev ? min(a.M, min(a.n_dev[0], a.M / (a.Ho * a.Wo)) * (a.Ho * a.Wo)) : a.M;     // device-side item count: the grid was sized for a bound
    const int M = LIST ? max(0, min(a.pix_count[0], Mmap)) : Mmap;      // LIST: live rows of the list; pixels live in [0, Mmap)
    const int lim = LIST ? Mmap : M;                                    // a row's pixel index is live below this
    // LIST: the pixel of GEMM row m; a dead row -- past the live count, or an entry outside the map -- answers Mmap
    auto list_row = [&](int m) -> int {
        if (m >= M) return Mmap;
        const int p = a.pix_list[m];
        return (unsigned)p < (unsigned)Mmap ? p : Mmap;
    };
    int tbx, tby;
    if (!xcd_tile_xy_live(a.xcd_map, (M + BM - 1) / BM, tbx, tby)) return;
    const int m0 = tbx * BM;
    const int n0 = tby * BN;

    const T* __restrict__ xg = reinterpret_cast<const T*>(a.x);
    const T* __restrict__ wg = reinterpret_cast<const T*>(a.w);
    const T* zero = reinterpret_cast<const T*>(a.zero);

    const T* rowp[A_PER];
    unsigned vmask[A_PER];
    const int HoWo = a.Ho * a.Wo;
    const int ntap = a.KH * a.KW;
    const float inv_howo = 1.0f / (float)HoWo, inv_wo = 1.0f / (float)a.Wo;
#pragma unroll
    for (int i = 0; i < A_PER; ++i) {
        int m = m0 + r0 + RP * i;
        if constexpr (LIST) m = list_row(m);
        unsigned mk = 0;
        const T* rp = zero;
        if (m < lim) {
            int img, rem, oh, ow;
            fast_divmod(m, HoWo, inv_howo, img, rem);
            fast_divmod(rem, a.Wo, inv_wo, oh, ow);
            const int ih0 = oh * a.stride - a.pad, iw0 = ow * a.stride - a.pad;
            rp = xg + (((long)img * a.H + ih0) * a.W + iw0) * a.x_cs + a.x_coff;
            // in-bounds taps, loop-free: columns [lo_w, hi_w) x rows [lo_h, hi_h) of the KH x KW window
            const int lo_w = max(0, -iw0), hi_w = min(a.KW, a.W - iw0);
            const int lo_h = max(0, -ih0), hi_h = min(a.KH, a.H - ih0);
            if (hi_w > lo_w && hi_h > lo_h) {
                const unsigned vw = ((1u << hi_w) - 1u) & ~((1u << lo_w) - 1u);
                const unsigned rows = (((1u << (hi_h * a.KW)) - 1u) & ~((1u << (lo_h * a.KW)) - 1u)) & a.tap_rows;
                mk = vw * rows;                     // replicate the column bits at every valid row
            }
        }
        rowp[i] = rp;
        vmask[i] = mk;
    }
    const int nsteps = a.Kp / BKE;
    const int wm = wv / WN, wn = wv % WN;
    const int q = lane >> 4, r = lane & 15;

    floatx4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    if (a.bias_init) {                         // bias first (ConvArgs::bias_init): the epilogue's `bias` is a page of zeros
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            floatx4 b;
#pragma unroll
            for (int e = 0; e < 4; ++e) b[e] = a.bias_init[n0 + wn * NT * 16 + perm_ch<NT>(j, q, e)];
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[i][j] = b;
        }
    }

    // LDS offsets of this lane's operand chunks inside a stage (stage base added as an immediate below)
    int xoff[MT], woff[NT];
#pragma unroll
    for (int i = 0; i < MT; ++i) xoff[i] = lds_off((wm * MT + i) * 16 + r, q);
#pragma unroll
    for (int j = 0; j < NT; ++j) woff[j] = BM * 64 + lds_off(wn * NT * 16 + perm_row<NT>(j, r), q);
    typedef typename Frag<T>::type frag_t;
    floatx4 mid[sizeof(T) == 4 ? MT : 1][sizeof(T) == 4 ? NT : 1];      // fp32 only: the mid-level accumulators ...
    doublex4 accd[sizeof(T) == 4 ? MT : 1][sizeof(T) == 4 ? NT : 1];    // ... and the top level (it starts from `acc`: zero, or the bias)
    int mid_steps = 0;
    if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                mid[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) accd[i][j][e] = acc[i][j][e];
            }
    }
    auto compute = [&](int stage) {
        const char* base = smem + stage * STAGE;
        frag_t xf[MT], wf[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) xf[i] = *reinterpret_cast<const frag_t*>(base + xoff[i]);
#pragma unroll
        for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const frag_t*>(base + woff[j]);
        if constexpr (sizeof(T) == 4) {         // fp32: three-level summation (conv_common.hpp)
            static_assert(sizeof(T) == 2 || MT * NT <= 8, "fp32 tiles carry a mid-level set beside the accumulators");
            mma_tiles_mid<MT, NT>(mid, wf, xf);
            if ((++mid_steps & (MID_STEPS - 1)) == 0) flush_mid<MT, NT>(accd, mid);
        } else {
            mma_tiles<T, MT, NT>(acc, wf, xf);
        }
    };
    char* const sdst = smem + (16 * wv) * 64;   // this wave's 16 rows inside a staging pass

    if (a.Cin % BKE == 0) {
        // ---- fast path: a K-step never straddles a tap, so the tap is uniform. Source pointers are set up
        // once per tap (validity bit, tap offset) and then only incremented: ~2 VALU per LDS-DMA instead of ~12.
        const int csteps = a.Cin / BKE;
        const T* aptr[A_PER];
        int ainc[A_PER];
        const T* wptr[B_PER];
        int winc[B_PER];
#pragma unroll
        for (int j = 0; j < B_PER; ++j) {
            const bool okr = r0 + RP * j < BN;
            wptr[j] = okr ? wg + (size_t)(n0 + r0 + RP * j) * a.Kp + kc * CH : zero;   // weights carry NSTAGE K-steps of slack
            winc[j] = okr ? BKE : 0;
        }
        int tap = 0, kh = 0, kw = 0, cc = 0, ti3 = 0;
        const int kord = a.k_order;                 // != 0: K-steps in another order than memory's, source pointers rebuilt every step
        const bool cmaj = kord != 0;
        // split source (ConvArgs::xs; 1x1 / 1 / 0, memory order only): K-steps 0 .. ssteps - 1 read the half-resolution tensor
        const int ssteps = (a.xs && !cmaj) ? a.Cs / BKE : 0;
        auto xs_row = [&](int i) -> const T* {
            int m = m0 + r0 + RP * i;
            if constexpr (LIST) m = list_row(m);
            if (m >= lim) return zero;
            int img, rem, oh, ow;
            fast_divmod(m, HoWo, inv_howo, img, rem);
            fast_divmod(rem, a.Wo, inv_wo, oh, ow);
            return reinterpret_cast<const T*>(a.xs) + (((long)img * a.Hs + (oh >> 1)) * a.Ws + (ow >> 1)) * a.xs_cs + a.xs_coff + kc * CH;
        };
        // second source (ConvArgs::x2, chunk-major walks only): its channel chunk e is accumulated right after tap (0, 0) of the window's chunk
        // e + 1 -- the place conv3x3_pp_patch_kernel has for it; every kernel walks the same order.  xs: the step being set up is that chunk, e = cc - 1
        const int csteps2 = (a.x2 && kord == 1) ? a.Cin2 / BKE : 0;
        bool xs = false;
        auto set_tap = [&] {
            if (xs) {
                const int c2 = cc - 1;
#pragma unroll
                for (int i = 0; i < A_PER; ++i) {
                    int m = m0 + r0 + RP * i;
                    if constexpr (LIST) m = list_row(m);
                    const T* p = zero;
                    if (m < lim) {
                        int img, rem, oh, ow;
                        fast_divmod(m, HoWo, inv_howo, img, rem);
                        fast_divmod(rem, a.Wo, inv_wo, oh, ow);
                        p = reinterpret_cast<const T*>(a.x2) + (((long)img * a.H2 + oh * a.s2) * a.W2 + ow * a.s2) * a.x2_cs + a.x2_coff + kc * CH + c2 * BKE;
                    }
                    aptr[i] = p, ainc[i] = 0;
                }
                return;
            }
            const long toff = ((long)kh * a.W + kw) * a.x_cs + kc * CH + (cmaj ? cc * BKE : 0);
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                const bool ok = tap < ntap && cc < csteps && ((vmask[i] >> (tap & 31)) & 1u);
                aptr[i] = ok ? rowp[i] + toff : zero;
                ainc[i] = (ok && !cmaj) ? BKE : 0;
            }
        };
        set_tap();
        if (ssteps) {
#pragma unroll
            for (int i = 0; i < A_PER; ++i) { aptr[i] = xs_row(i); ainc[i] = aptr[i] == zero ? 0 : BKE; }
        }
        auto issue_fast = [&](int stage) {
            char* sbase = sdst + stage * STAGE;
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                __builtin_amdgcn_global_load_lds((gptr_t)aptr[i], (lptr_t)(sbase + i * (RP * 64)), 16, 0, 0);
                aptr[i] += ainc[i];
            }
            if (cmaj) {
                const int koff = xs ? ntap * a.Cin + (cc - 1) * BKE : tap * a.Cin + cc * BKE;
#pragma unroll
                for (int j = 0; j < B_PER; ++j) {
                    const T* src = (winc[j] && cc < csteps) ? wptr[j] + koff : zero;
                    asm volatile("" : "+v"(src));
                    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + BM * 64 + j * (RP * 64)), 16, 0, 0);
                }
                if (kord == 1) {                        // (cc, kh, kw), the second source's chunk cc - 1 behind tap (0, 0) of chunks 1 .. csteps2
                    if (!xs && kh == 0 && kw == 0 && cc >= 1 && cc <= csteps2 && cc < csteps) xs = true;
                    else {
                        xs = false;
                        if (++kw == a.KW) { kw = 0; if (++kh == a.KH) { kh = 0; ++cc; } }
                    }
                } else if (kord == 3) {                 // (cc, then the nine taps plane by plane: 0 2 6 8 | 1 7 | 3 5 | 4 -- conv3x3s2_sp_patch_kernel's order)
                    if (++ti3 == 9) { ti3 = 0; ++cc; }
                    const int tp = (int)((0x453718620ull >> (4 * ti3)) & 15);
                    kh = tp / 3, kw = tp - 3 * kh;
                } else {                                // (kw, cc, kh)
                    if (++kh == a.KH) { kh = 0; if (++cc == csteps) { cc = 0; ++kw; } }
                    if (kw == a.KW) { kw = 0; cc = csteps; }          // past the last step: zero page from here on
                }
                tap = kh * a.KW + kw;
                set_tap();
                return;
            }
#pragma unroll
            for (int j = 0; j < B_PER; ++j) {
                __builtin_amdgcn_global_load_lds((gptr_t)wptr[j], (lptr_t)(sbase + BM * 64 + j * (RP * 64)), 16, 0, 0);
                wptr[j] += winc[j];
            }
            if (++cc == csteps) {                      // uniform: next tap
                cc = 0;
                ++tap;
                if (++kw == a.KW) { kw = 0; ++kh; }
                set_tap();
            } else if (cc == ssteps && ssteps) {       // the split source's channels are through: on in the concat buffer, at channel Cs
#pragma unroll
                for (int i = 0; i < A_PER; ++i) {
                    const bool ok = (vmask[i] & 1u) != 0;
                    aptr[i] = ok ? rowp[i] + kc * CH + cc * BKE : zero;
                    ainc[i] = ok ? BKE : 0;
                }
            }
        };
#pragma unroll
        for (int st = 0; st < NSTAGE - 1; ++st) issue_fast(st);
        for (int step0 = 0; step0 < nsteps; step0 += NSTAGE) {
#pragma unroll
            for (int u = 0; u < NSTAGE; ++u) {         // stage index is a compile-time constant inside the body
                if (step0 + u < nsteps) {
                    wait_vmcnt<(NSTAGE - 2) * LPS>();
                    __builtin_amdgcn_s_barrier();
                    issue_fast((u + NSTAGE - 1) % NSTAGE);
                    compute(u);
                }
            }
        }
    } else {
        // ---- generic path (Cin < K-step or not a multiple of it: 3-channel stems, 16/48/80-channel layers)
        const T* wp[B_PER];
#pragma unroll
        for (int j = 0; j < B_PER; ++j) {
            const int row = r0 + RP * j;
            wp[j] = row < BN ? wg + (size_t)(n0 + row) * a.Kp + kc * CH : nullptr;
        }
        int c_in = kc * CH, kw_ = 0, kh_ = 0;
        while (c_in >= a.Cin) {
            c_in -= a.Cin;
            if (++kw_ == a.KW) { kw_ = 0; ++kh_; }
        }
        int issued = 0;
        auto issue = [&](int stage) {
            const int tap = kh_ * a.KW + kw_;
            const bool in_k = tap < ntap;
            const long toff = ((long)kh_ * a.W + kw_) * a.x_cs + c_in;
            char* sbase = sdst + stage * STAGE;
#pragma unroll
            for (int i = 0; i < A_PER; ++i) {
                const bool ok = in_k && ((vmask[i] >> (tap & 31)) & 1u);
                const T* src = ok ? rowp[i] + toff : zero;
                asm volatile("" : "+v"(src));   // one select, ONE LDS-DMA instruction per wave: keeps vmcnt counting uniform
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + i * (RP * 64)), 16, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < B_PER; ++j) {
                const T* src = (wp[j] != nullptr && issued < nsteps) ? wp[j] + (size_t)issued * BKE : zero;
                asm volatile("" : "+v"(src));
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + BM * 64 + j * (RP * 64)), 16, 0, 0);
            }
            ++issued;
            c_in += BKE;
            while (c_in >= a.Cin) {
                c_in -= a.Cin;
                if (++kw_ == a.KW) { kw_ = 0; ++kh_; }
            }
        };
#pragma unroll
        for (int st = 0; st < NSTAGE - 1; ++st) issue(st);
        int cur = 0;
        for (int step = 0; step < nsteps; ++step) {
            wait_vmcnt<(NSTAGE - 2) * LPS>();      // this wave's loads of `step` have landed
            __builtin_amdgcn_s_barrier();          // ... everyone's have, and everyone finished step-1
            int nxt = cur + NSTAGE - 1;
            if (nxt >= NSTAGE) nxt -= NSTAGE;
            issue(nxt);                            // refills the buffer that step-1 just released
            compute(cur);
            if (++cur == NSTAGE) cur = 0;
        }
    }
    wait_vmcnt<0>();   // drain the zero-page loads of the tail before the LDS goes away
    if constexpr (sizeof(T) == 4) {                                // the last (partial) block of mid-level steps
        flush_mid<MT, NT>(accd, mid);
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][e] = (float)accd[i][j][e];
    }

    int mrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = m0 + (wm * MT + i) * 16 + r;
        if constexpr (LIST) m = list_row(m);                       // mrow is the PIXEL: stores, residual and the tail's anchor land at its true position
        mrow[i] = m < lim ? m : -1;
    }
    if constexpr (TAIL) {
        static_assert(sizeof(T) == 2 && WN == 1, "the tail needs fp16 and a wave that owns every channel of its pixels");
        tail_1x1<MT, NT>(a, acc, mrow, lane);
    } else {
        epilogue_dispatch<T, MT, NT, true, WM * WN == 8>(a, acc, mrow, n0 + wn * NT * 16, q);
    }
}

template <typename T, int MT, int NT, int WM, int WN, int NSTAGE, bool TAIL = false, bool LIST = false>
static void launch_dma(const ConvArgs& a, hipStream_t s) {
    constexpr int RP = 16 * WM * WN;
    constexpr int BM = WM * MT * 16, BN = WN * NT * 16, BNP = (BN + RP - 1) / RP * RP;
    dim3 grid(ceil_div(a.M, BM), ceil_div(a.Cout, BN));
    const size_t lds = (size_t)NSTAGE * (BM + BNP) * 64;
    AIC_REQUIRE(LIST == (a.pix_list != nullptr) && (!LIST || a.pix_count), AIC_ERR_INVALID, "conv plan: pixel list and kernel form disagree");
    auto kfn = conv_igemm_dma_kernel<T, MT, NT, WM, WN, NSTAGE, TAIL, LIST>;
    if (lds > 64 * 1024) set_lds_limit(kfn, lds);
    hipLaunchKernelGGL(kfn, grid, dim3(64 * WM * WN), lds, s, a);
    KCHECK();
}
// (Measured in round 5 and removed for the small-tile launches: kernels_conv_sp.hip's lean K-step -- bit-identical, per-frame plugin loop
//  1 070 -> 1 030 us of conv per frame but 16- / 64-frame groups 7 100 -> 6 320 / 10 300 -> 9 900 frames/s; inline-asm MFMAs with early loop
//  exits also made the ReID layers non-deterministic -- and an 8-stage ring, 1 101 against 1 075 us: their K loop does not wait for memory.)

// The LDS-DMA tiles plan_conv hands out (conv_plan.cpp): fp32 engines run the 4-wave tiles only, the 8-wave and 144-channel ones and the
// tail forms are fp16.
static void launch_conv_dma(int dtype, const ConvArgs& a, const ConvPlan& p, hipStream_t s) {
    if (p.list) {                               // the pixel-list forms (ConvArgs::pix_list): 128 px x 64 ch, with and without the decoding tail
        AIC_REQUIRE(dtype == AIC_F16 && p.mt == 2 && p.nt == 4 && p.wm == 4 && p.wn == 1 && p.nstage == 4, AIC_ERR_INVALID, "conv plan: no pixel-list instantiation for this tile");
        if (p.tail) return launch_dma<half_t, 2, 4, 4, 1, 4, true, true>(a, s);
        return launch_dma<half_t, 2, 4, 4, 1, 4, false, true>(a, s);
    }
#define DMA(T, MT, NT, WM, WN, NS, TAIL)                                                                                        \
    if (sizeof(T) == (dtype == AIC_F16 ? 2u : 4u) && p.mt == MT && p.nt == NT && p.wm == WM && p.wn == WN && p.nstage == NS && \
        p.tail == TAIL)                                                                                                        \
        return launch_dma<T, MT, NT, WM, WN, NS, TAIL>(a, s);
    DMA(float, 2, 4, 2, 2, 4, false) DMA(float, 1, 5, 4, 1, 4, false) DMA(float, 2, 4, 4, 1, 4, false)
    DMA(float, 2, 3, 4, 1, 4, false) DMA(float, 4, 2, 4, 1, 4, false) DMA(float, 4, 1, 4, 1, 4, false)
    DMA(half_t, 8, 4, 2, 4, 4, false) DMA(half_t, 4, 4, 4, 2, 3, false) DMA(half_t, 4, 4, 2, 2, 4, false) DMA(half_t, 2, 2, 2, 2, 4, false)
    DMA(half_t, 4, 9, 4, 1, 4, false) DMA(half_t, 2, 9, 4, 1, 4, false) DMA(half_t, 4, 5, 8, 1, 3, false) DMA(half_t, 2, 5, 4, 1, 4, false)
    DMA(half_t, 4, 4, 4, 1, 4, false) DMA(half_t, 2, 4, 4, 1, 4, false) DMA(half_t, 2, 3, 4, 1, 4, false) DMA(half_t, 4, 2, 4, 1, 4, false)
    DMA(half_t, 4, 1, 4, 1, 4, false)
    DMA(half_t, 4, 4, 4, 1, 4, true) DMA(half_t, 2, 4, 4, 1, 4, true) DMA(half_t, 4, 5, 8, 1, 3, true) DMA(half_t, 2, 5, 4, 1, 4, true)
#undef DMA
    AIC_REQUIRE(false, AIC_ERR_INVALID, "conv plan: no LDS-DMA instantiation for this tile");
}

void launch_conv_igemm(int dtype, const ConvArgs& a0, hipStream_t s) {
    if (a0.M <= 0) return;
    ConvArgs a = a0;
    a.xcd_map = 1;
    const ConvPlan p = plan_conv_launch(dtype, a, conv_cu_budget());
    if (a.k_order == 2 && p.form != ConvForm::C64Resident) {
        // the order AND the bias placement of the weights-resident kernels (Cout = 64: one 256-byte zero page covers the epilogue's reads)
        a.bias_init = a.bias;
        a.bias = reinterpret_cast<const float*>(a.zero);
    }
    switch (p.form) {
        case ConvForm::Dma: launch_conv_dma(dtype, a, p, s); break;
        case ConvForm::Wide: launch_conv_wide(a, p, s); break;
        case ConvForm::Pp: launch_conv_pp(a, p, s); break;
        case ConvForm::PpPatch: launch_conv_pp_patch(a, p, s); break;
        case ConvForm::SpPatch: launch_conv_sp_patch(a, p, s); break;
        case ConvForm::S2Patch: launch_conv_s2_patch(a, p, s); break;
        case ConvForm::Patch: launch_conv_patch(a, p, s); break;
        case ConvForm::PmPatch: launch_conv_pm_patch(a, p, s); break;
        case ConvForm::C16: launch_conv_c16(a, p, s); break;
        case ConvForm::C32s2Tail: launch_conv_c32s2_tail(a, p, s); break;
        case ConvForm::Stream1x1: launch_conv_1x1_stream(a, p, s); break;
        case ConvForm::C64Resident: launch_conv_c64_resident(a, p, s); break;
    }
}


}  // namespace aic
