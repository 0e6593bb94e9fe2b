// conv_plan.cpp -- the conv dispatch as one decision tree (conv_plan.hpp).  Every threshold here was measured on MI355X with the kernel
// it selects; the notes on why a form wins where it does sit with the kernels (kernels_conv*.hip).  Plain C++: no HIP header.
#include "conv_plan.hpp"

#include <algorithm>
#include <cstdlib>

namespace aic {

static int g_conv_cus = 256;
int conv_cu_budget() { return g_conv_cus; }
void set_conv_cu_budget(int cus) { g_conv_cus = std::max(1, cus); }

static long cdiv(long a, long b) { return (a + b - 1) / b; }
static const long B31 = 1l << 31;

// Runs of tiles per block for the one-block-per-CU patch kernels: the longest run of at most max_run tiles that does not add a round
// of tiles (256 CUs, one block each) and leaves >= 4 rounds of blocks.  (Same box, 15 360 crops: ReID layer2 conv1 1 993 us at one
// tile per block -> 1 975 / 1 945 / 1 912 us at runs of 1 / 4 / 6; with a residual 2 257 -> 2 256; layer3 / 4 -2 % / 0.)
static int tile_run(long ntiles, int max_run) {
    int run = 1;
    long best = -1;
    for (int r = 1; r <= max_run; ++r) {
        const long blocks = (ntiles + r - 1) / r, rounds = (blocks + 255) / 256;
        if (r > 1 && rounds < 4) break;
        const long cost = rounds * r;                 // tile times until the last block ends
        if (best < 0 || cost <= best) best = cost, run = r;
    }
    return run;
}

static ConvPlan only(ConvForm f) { ConvPlan p; p.form = f; return p; }
static ConvPlan tile(ConvForm f, int mt, int nt, int wm, int wn, int nstage) {
    ConvPlan p = only(f);
    p.mt = mt, p.nt = nt, p.wm = wm, p.wn = wn, p.nstage = nstage;
    return p;
}

// ---- layer shapes (properties of the graph, not of the batch)

// The ping-pong patch kernel's shapes: 3x3 / 1 / 1 layers whose map tiles exactly -- 2 = Cout 128 (32 x 16 tiles), 3 = Cout % 256 on
// 16 x 8 tiles, 4 = on 8 x 4 tiles; 0 = none.  Such a layer is walked chunk-major by EVERY conv kernel (k_order 1).
static int pp_patch_shape(int dtype, const ConvArgs& a) {
    const int bke = dtype == AIC_F16 ? 32 : 16;
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || a.Cin % (2 * bke) || a.Ho != a.H || a.Wo != a.W) return 0;
    const int c = a.Cout;
    if (c == 128) return (a.H % 32 == 0 && a.W % 16 == 0) ? 2 : 0;
    if (c % 256 == 0) return (a.H % 16 == 0 && a.W % 8 == 0) ? 3 : ((a.H % 8 == 0 && a.W % 4 == 0) ? 4 : 0);
    return 0;
}

// The stride-2 shapes (walked in k_order 3 by EVERY kernel): 3x3 / 2 / 1 convs whose OUTPUT is one of the patch kernels' maps -- 1: Cout
// 128 on 32 x 16, 2: Cout % 256 on 16 x 8 -- with Cin a multiple of 64.  (8 x 4 output maps, ReID layer4.0.conv1: built and measured --
// 1 135 against v4's 1 008 us per 15 360 crops; the map is small enough for the im2col gather to stay in the L2.  Not kept.)
static int s2_patch_shape(const ConvArgs& a) {
    if (a.KH != 3 || a.KW != 3 || a.stride != 2 || a.pad != 1 || a.Cin % 64 || a.Kp != 9 * a.Cin || a.x2 || a.xs || a.w_tail) return 0;
    if (a.H != 2 * a.Ho || a.W != 2 * a.Wo) return 0;
    if (a.Cout == 128 && a.Ho == 32 && a.Wo == 16) return 1;
    if (a.Cout % 256 == 0 && a.Ho == 16 && a.Wo == 8) return 2;
    return 0;
}

int conv_k_order(int dtype, const ConvArgs& a) {
    // the 64-channel weights-resident kernels (fp16): any 3x3 / 1 / 1 layer with Cin = Cout = 64 whose map they tile
    // (ReLU, with or without the BasicBlock's residual: the only forms those kernels have)
    const bool c64 = dtype == AIC_F16 && a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.Cin == 64 && a.Cout == 64 && a.Kp == 576 &&
                     a.act == 2 && a.res_mode <= 1 && !a.out_f32 && !a.w_tail &&
                     a.Ho == a.H && a.Wo == a.W && ((a.W % 32 == 0 && a.H % 8 == 0) || (a.W == 32 && a.H % 4 == 0));
    return pp_patch_shape(dtype, a) ? 1 : (c64 ? 2 : (s2_patch_shape(a) ? 3 : 0));
}

// ---- the fp16 forms, each with every eligibility test of its kernel

static bool c16_ok(const ConvArgs& a) {
    if (a.KH != 3 || a.KW != 3 || a.pad != 1 || a.Cin != 16 || a.act != 1 || a.out_f32 || (a.res_mode != 0 && a.res_mode != 2)) return false;
    if (a.Wo % 32 || a.Ho % 8 || a.Kp != 160 || (a.x_cs | a.x_coff | a.y_cs | a.y_coff | a.r_cs | a.r_coff) % 8) return false;
    if (a.stride == 1 && (a.Ho != a.H || a.Wo != a.W)) return false;
    if (a.stride == 2 && (a.Ho != (a.H + 1) / 2 || a.Wo != (a.W + 1) / 2)) return false;
    return (a.Cout == 16 || a.Cout == 32) && (a.stride == 1 || a.stride == 2);
}

static bool stream1x1_ok(const ConvArgs& a) {
    static const bool off = getenv("AICAM_NO_1X1_STREAM") != nullptr;
    if (off || a.KH != 1 || a.KW != 1 || a.stride != 1 || a.pad != 0 || a.Cout != 64 || a.Cin % 32 || a.Cin > 128 || a.Cin < 64 || a.Kp != a.Cin) return false;
    if (a.res_mode != 0 || a.out_f32 || a.k_order != 0 || a.xs || a.x2 || a.w_tail || a.n_dev || a.bias_init || a.cout_pad < 64) return false;
    return a.M >= 150000 && (a.x_cs | a.x_coff | a.y_cs | a.y_coff) % 8 == 0 && (long)a.M * std::max(a.x_cs, a.y_cs) < B31;
}

// with or without the residual: 612 -> 774 TFLOP/s against the 4-wave patch kernel
static bool c64_resident_ok(const ConvArgs& a) {
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || a.Cin != 64 || a.Cout != 64 || a.out_f32 || a.Kp != 576) return false;
    if (a.W % 32 || a.H % 8 || a.Ho != a.H || a.Wo != a.W || a.M < 1500000 || (long)a.M * a.x_cs >= B31 ||
        (long)a.M * a.y_cs >= B31 || (a.res_mode != 0 && (long)a.M * a.r_cs >= B31)) return false;
    if ((a.x_cs | a.x_coff | a.y_cs | a.y_coff | a.r_cs | a.r_coff) % 8) return false;
    return a.act == 2 && (a.res_mode == 0 || a.res_mode == 1);
}

static bool c32s2_tail_ok(const ConvArgs& a) {
    static const bool off = getenv("AICAM_NO_C32S2") != nullptr;
    if (off || !a.w_tail || a.KH != 3 || a.KW != 3 || a.stride != 2 || a.pad != 1 || a.Cin != 32 || a.Cout != 64 || a.Kp != 288) return false;
    if (a.act != 1 || a.res_mode != 0 || a.out_f32 || a.k_order != 0 || a.xs || a.x2 || a.n_dev || a.t_max || a.t_box) return false;
    if (a.t_cout > 64 || a.t_cout % 8 || a.t_kp != 64 || a.cout_pad < 64) return false;
    if (a.Ho % 16 || a.Wo % 16 || a.Ho != (a.H + 1) / 2 || a.Wo != (a.W + 1) / 2 || (a.x_cs | a.x_coff | a.t_y_cs | a.t_y_coff) % 8) return false;
    const long blocks = (long)(a.M / (a.Ho * a.Wo)) * (a.Wo / 16) * (a.Ho / 16);
    return blocks >= 512 && (long)a.M * std::max(a.t_y_cs, 1) < B31;     // a few tiles: the wide-step kernel (one block per CU there)
}

// The 4-wave patch kernel (Cout 64 / 80 / 32; its Cin is fixed per instantiation: 64, or 32 for Cout 32).  Measured (profiles/): the
// patch form wins where Cout is small and M is large (ReID layer1); for Cout >= 128 the 8-wave im2col tile is faster, and small maps are
// launch-bound either way.
static bool patch(ConvPlan& p, const ConvArgs& a, bool tail) {
    static const bool c32 = getenv("AICAM_NO_PATCH_C32") == nullptr;   // Cin = Cout = 32 (YOLOv8n P3 bottlenecks): 244 -> 460 TFLOP/s
    static const bool c80 = getenv("AICAM_NO_PATCH_C80") == nullptr;   // YOLOv8n's 22.cls0.0 (64 -> 80 at 80 x 80): 461 TFLOP/s on the 512 x 80 implicit-GEMM tile
    if (a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || a.Wo < 16 || a.Ho < 8 || a.M < 200000) return false;
    if (a.k_order == 1 || (tail && a.k_order != 0)) return false;          // (cc, kh, kw): only the implicit-GEMM kernels walk K that way
    if (a.k_order == 2 && a.Cout != 64) return false;                        // (fp16, Cin = Cout = 64: the resident kernels' order)
    if (tail ? a.Cout != 64 : !(a.Cout == 64 || (a.Cout == 80 && c80) || (a.Cout == 32 && c32))) return false;
    const bool wide = a.Wo % 32 == 0 || (a.Wo % 16 != 0 && a.Wo >= 32);   // 8 x 32 tiles unless 16 x 16 tiles cover the map exactly
    if (a.k_order == 2 && !wide) return false;
    const int cpp = a.Cout == 32 ? 4 : 8;
    if (a.Cin != 8 * cpp) return false;
    p = tile(ConvForm::Patch, 4, a.Cout / 16, 4, 1, 3);
    p.th = wide ? 8 : 16, p.tw = wide ? 32 : 16, p.cpp = cpp, p.kord = a.k_order, p.tail = tail;
    return true;
}

// The pixel-major patch kernel on 3x3 / 1 / 1 whole maps in memory K order, launches of 50 000 pixels and more: with a 1x1 tail 80 -> 80
// or 64 -> 64, without one 64 -> 64 and 128 -> 144 in 40 x 8 strips of 40-row maps; 16 x 16 tiles where they cover the map with at most
// half as many pixels again hanging over the edge.
static bool pm_patch(ConvPlan& p, const ConvArgs& a) {
    static const bool off = getenv("AICAM_NO_PATCH_C80") != nullptr;
    if (off || a.KH != 3 || a.KW != 3 || a.stride != 1 || a.pad != 1 || a.k_order != 0 || a.xs || a.x2 || a.n_dev || a.out_f32 || a.bias_init) return false;
    if (a.Ho != a.H || a.Wo != a.W || a.M < 50000 || (a.x_cs | a.x_coff | a.y_cs | a.y_coff | a.r_cs | a.r_coff) % 8) return false;
    const bool tail = a.w_tail != nullptr;
    if (a.act != 1 || (tail ? a.res_mode != 0 : a.res_mode != 0 && a.res_mode != 2)) return false;
    const bool cover16 = 2 * (cdiv(a.Wo, 16) * 16 * cdiv(a.Ho, 16) * 16) <= 3 * (long)a.Wo * a.Ho;
    const bool strips = a.Ho == 40 && a.Wo % 8 == 0;
    auto form = [&](int cpp, int pitch, int nt, int mt, int th, int tw) {
        p = only(ConvForm::PmPatch);
        p.cpp = cpp, p.pitch = pitch, p.nt = nt, p.mt = mt, p.th = th, p.tw = tw, p.tail = tail;
        return true;
    };
    const bool c64 = a.Cin == 64 && a.Cout == 64 && a.Kp == 576 && a.cout_pad >= 64;
    if (tail) {
        if (a.Cin == 80 && a.Cout == 80 && a.Kp == 736 && a.cout_pad >= 128 && cover16) return form(10, 10, 5, 4, 16, 16);
        if (c64 && strips) return form(8, 9, 4, 5, 40, 8);
        if (c64 && cover16) return form(8, 9, 4, 4, 16, 16);
        return false;
    }
    if (c64 && strips) return form(8, 9, 4, 5, 40, 8);
    if (a.res_mode == 0 && a.Cin == 128 && a.Cout == 144 && a.Kp == 1152 && a.cout_pad >= 144 && strips) return form(16, 17, 9, 5, 40, 8);
    return false;
}

// The wide-step kernel (a few tiles: the grid v2 would launch for the same tile is at most 256 blocks).  `bias_init`: whether the kernel
// is handed a bias to start from (k_order 2).
static bool wide(ConvPlan& p, const ConvArgs& a, bool bias_init, int mt, int nt, int wm, int wn, bool tail) {
    const int bm = wm * mt * 16, bn = wn * nt * 16, bnp = (bn + 63) / 64 * 64;
    if (cdiv(a.M, bm) * cdiv(a.Cout, bn) > 256) return false;
    if (a.xs || a.n_dev || (a.w_tail != nullptr) != tail) return false;
    if (a.k_order < 0 || a.k_order > 3) return false;
    if ((a.k_order == 2) != bias_init || (a.k_order == 2 && (a.KH != 3 || a.x2 || tail))) return false;      // order 2 comes with the bias in front
    if (a.x2 && (a.k_order != 1 || tail || a.Cin2 <= 0 || a.Cin2 % 32 || a.Cin2 / 32 >= a.Cin / 32)) return false;
    if (a.KH != a.KW || (a.KH != 1 && a.KH != 3) || a.pad != a.KH / 2 || a.Cin % 32 || a.Kp != a.KH * a.KW * a.Cin + (a.x2 ? a.Cin2 : 0)) return false;
    if (a.KH == 3 && a.tap_rows != 0x49u) return false;
    if ((long)(2 * a.W + 2) * a.x_cs * 2 + a.Cin * 2 >= B31 || (long)a.Kp * 2 >= B31) return false;      // the K table's 32-bit byte offsets
    if (a.Kp / 32 < 8) return false;                             // a K loop of a few steps has nothing to group
    if (a.x2 && (tail || (bn != 64 && bn != 128) || wn != 2)) return false;   // (the tiles the ReID trunk's second-source layers take at these sizes)
    p = tile(ConvForm::Wide, mt, nt, wm, wn, 3);
    // Ring shape (tools/conv_bench.py, ReID layer4 at 28 crops, 60.7 us on v2): G = 4 with 3 or 5 groups in the ring 32.3 / 32.8 us, G = 2 with 10
    // groups 34.3 us -- the depth does not matter.  At most 96 .. 120 KB of LDS, so that a block of another stream's kernel still fits beside it.
    p.g = (bm + bnp) * 64 <= 8 * 1024 ? 4 : 2;
    p.tail = tail, p.x2 = a.x2 != nullptr;
    return true;
}

// v5 ping-pong patch / v6 software-pipelined patch, on the layers of a pp_patch_shape and a batch that fills one block per CU
static bool pp_patch(ConvPlan& p, const ConvArgs& a) {
    static const int pp_min = [] { const char* e = getenv("AICAM_PP_MIN"); return e ? atoi(e) : 200; }();
    const int shape = pp_patch_shape(AIC_F16, a), c = a.Cout;
    if (!shape || (long)a.M * a.x_cs >= B31) return false;                    // 32-bit element offsets inside the kernel
    if (!(shape == 2 ? a.M / 512 >= pp_min : (long)(a.M / 256) * (c / 256) >= pp_min)) return false;
    const int wm = shape == 2 ? 4 : 2, wn = shape == 2 ? 2 : 4, th = shape == 2 ? 32 : (shape == 3 ? 16 : 8), tw = th / 2;
    const int n_img = a.M / (a.Ho * a.Wo), ni = wm * 8 * 16 / (th * tw);
    // v6 (fp16, no second source; same K order, same bits): whole-image tiles, whole channel tiles, 32-bit byte strides inside the kernel
    if (!a.x2 && a.Cin % 128 == 0 && a.H == th && a.W == tw && c % (wn * 64) == 0 && (long)a.M * a.x_cs * 2 < (1l << 32) &&
        (long)c * a.Kp * 2 < (1l << 32)) {
        p = tile(ConvForm::SpPatch, 8, 4, wm, wn, 4);
        p.th = th, p.tw = tw;
        const long ntiles = cdiv(n_img, ni) * (c / (wn * 64));
        p.run = tile_run(ntiles, 6), p.blocks = cdiv(ntiles, p.run);
        return true;
    }
    if (a.H % th || a.W % tw) return false;
    if (a.M >= (1 << 23) || a.x_cs >= (1 << 23)) return false;               // issue_patch's 24-bit address arithmetic
    if (a.x2 && ((long)n_img * a.H2 >= (1 << 23) || (long)a.W2 * a.x2_cs >= (1 << 23) || (long)n_img * a.H2 * a.W2 * a.x2_cs >= B31))
        return false;                                                          // issue_e's
    p = tile(ConvForm::PpPatch, 8, 4, wm, wn, 4);
    p.th = th, p.tw = tw, p.x2 = a.x2 != nullptr;
    const long ntiles = cdiv(n_img, ni) * (a.H / th) * (a.W / tw) * cdiv(c, wn * 64);
    p.run = tile_run(ntiles, p.x2 ? 1 : 6), p.blocks = cdiv(ntiles, p.run);   // (second source: one tile per block)
    return true;
}

// Ping-pong kernels (one block per CU) where the K loop is long enough to amortise the tile's prologue / epilogue: measured on MI355X
// (tools/conv_bench.py, profiles/): +17..19 % on ReID layer3/4, +14 % on layer2, a loss at K < 512.  18 K-steps: ReID layer2.0.conv1
// (3x3 / 2, 64 -> 128, K = 576) takes the 512 x 128 tile: 1 058 -> 948 us per 7 680 crops against the 8-wave 256 x 128 LDS-DMA tile;
// below that the short loop loses.  The stride-2 layers of the patch kernels' maps go to the space-to-depth patch form first.
static bool pp(ConvPlan& p, const ConvArgs& a) {
    static const int pp_min = [] { const char* e = getenv("AICAM_PP_MIN"); return e ? atoi(e) : 200; }();
    const int c = a.Cout;
    if (a.Cin % 32 != 0 || !(a.Kp >= 16 * 32 || pp_min == 0)) return false;
    const bool c256 = c % 256 == 0 && cdiv(a.M, 256) * (c / 256) >= pp_min, c128 = c == 128 && cdiv(a.M, 512) >= pp_min;
    const int s2 = a.k_order == 3 ? s2_patch_shape(a) : 0;
    if (s2 && (c256 || c128) && a.Cout % (s2 == 1 ? 128 : 256) == 0 && a.Cin % 64 == 0 && (long)a.M * 4 * a.x_cs * 2 < (1l << 32) &&
        (long)a.Cout * a.Kp * 2 < (1l << 32)) {
        const int wm = s2 == 1 ? 4 : 2, wn = s2 == 1 ? 2 : 4, th = s2 == 1 ? 32 : 16, tw = th / 2;
        p = only(ConvForm::S2Patch);
        p.wm = wm, p.wn = wn, p.th = th, p.tw = tw;
        const long ntiles = cdiv(a.M / (a.Ho * a.Wo), wm * 128 / (th * tw)) * (a.Cout / (wn * 64));
        p.run = tile_run(ntiles, 6), p.blocks = cdiv(ntiles, p.run);
        return true;
    }
    if (c256) { p = tile(ConvForm::Pp, 8, 4, 2, 4, 4); return true; }                               // 256 px x 256 ch
    if (c == 128 && (a.Kp >= 18 * 32 || pp_min == 0) && c128) { p = tile(ConvForm::Pp, 8, 4, 4, 2, 4); return true; }   // 512 px x 128 ch
    return false;
}

// ---- the tree

// fp32 engines (the parity mode) run ONE kernel family since round 5: the LDS-DMA implicit GEMM on tiles of at most 8 MFMA tiles per
// wave, whose three-level summation carries a mid-level accumulator set (conv_common.hpp).  The patch, ping-pong, wide-step and 8-wave
// forms are fp16 only.  (--dtype fp32 throughput: 1 167 frames/s with the two-level kernels of rounds 2-4.)
static ConvPlan plan_f32(const ConvArgs& a) {
    const int c = a.Cout;
    if (c % 128 == 0 || c > 160) return tile(ConvForm::Dma, 2, 4, 2, 2, 4);       // 64 px x 128 ch
    if (c % 80 == 0) return tile(ConvForm::Dma, 1, 5, 4, 1, 4);                    // 64 px x 80 ch
    if (c % 64 == 0) return tile(ConvForm::Dma, 2, 4, 4, 1, 4);                    // 128 px x 64 ch
    if (c % 48 == 0) return tile(ConvForm::Dma, 2, 3, 4, 1, 4);                    // 128 px x 48 ch
    if (c % 32 == 0 || c > 16) return tile(ConvForm::Dma, 4, 2, 4, 1, 4);          // 256 px x 32 ch
    return tile(ConvForm::Dma, 4, 1, 4, 1, 4);                                     // 256 px x 16 ch
}

// Lead conv of a (conv, 1x1) pair with the 1x1 in its epilogue: only the kernels whose waves own all channels of their pixels.
static ConvPlan plan_tail(const ConvArgs& a) {
    ConvPlan p;
    if (a.Cout == 64) {
        if (c32s2_tail_ok(a)) p = only(ConvForm::C32s2Tail);
        else if (pm_patch(p, a) || patch(p, a, true)) return p;
        else if (cdiv(a.M, 128) >= 512) p = tile(ConvForm::Dma, 4, 4, 4, 1, 4);        // 256 px x 64 ch
        else if (!wide(p, a, a.bias_init != nullptr, 2, 4, 4, 1, true)) p = tile(ConvForm::Dma, 2, 4, 4, 1, 4);   // 128 px x 64 ch
    } else {                                                                     // 80
        if (pm_patch(p, a)) return p;
        if (cdiv(a.M, 512) >= 256) p = tile(ConvForm::Dma, 4, 5, 8, 1, 3);        // 512 px x 80 ch
        else if (!wide(p, a, a.bias_init != nullptr, 2, 5, 4, 1, true)) p = tile(ConvForm::Dma, 2, 5, 4, 1, 4);   // 128 px x 80 ch
    }
    p.tail = true;
    return p;
}

// A launch with a pixel list (ConvArgs::pix_list) takes the LDS-DMA implicit GEMM and nothing else: its rows are gathered one by one,
// the patch forms need whole tiles of neighbours.  One tile, 128 px x 64 ch on four waves that each own every channel of their pixels --
// with a tail that is the NT == 4 form tail_1x1 decodes boxes in.  The K order is not touched here: it is the layer's (conv_k_order),
// which is what makes a listed pixel's output the bits of whatever dense form its batch would have selected.
static ConvPlan plan_list(int dtype, const ConvArgs& a) {
    AIC_REQUIRE(dtype == AIC_F16 && a.pix_count && a.Cout == 64 && a.Cin % 32 == 0 && !a.xs && !a.x2 && !a.win_rows && !a.out_f32 &&
                    a.M < (1 << 26),                            // (fast_divmod's range, as for the dense launch)
                AIC_ERR_INVALID, "conv with a pixel list: unsupported shape");
    if (a.w_tail) AIC_REQUIRE(a.act == 1 && a.res_mode == 0, AIC_ERR_INVALID, "conv with a pixel list and a 1x1 tail: unsupported lead");
    ConvPlan p = tile(ConvForm::Dma, 2, 4, 4, 1, 4);
    p.tail = a.w_tail != nullptr, p.list = true;
    return p;
}

ConvPlan plan_conv(int dtype, const ConvArgs& a, int cu_budget) {
    if (a.pix_list) return plan_list(dtype, a);
    if (a.x2) AIC_REQUIRE(a.k_order == 1 && a.Cout % 128 == 0 && !a.w_tail, AIC_ERR_INVALID, "conv with a second source: unsupported shape (check conv_x2_supported)");
    if (a.xs) AIC_REQUIRE(a.k_order == 0 && a.KH == 1 && a.KW == 1 && !a.w_tail && a.Kp < 16 * (dtype == AIC_F16 ? 32 : 16), AIC_ERR_INVALID,
                          "conv with a split source: unsupported shape (check conv_xs_supported)");
    if (a.w_tail) {
        AIC_REQUIRE(dtype == AIC_F16 && (a.Cout == 64 || a.Cout == 80) && a.act == 1 && a.res_mode == 0, AIC_ERR_INVALID,
                    "conv with a 1x1 tail: unsupported lead (check conv_tail_supported before setting w_tail)");
        return plan_tail(a);
    }
    if (dtype != AIC_F16) return plan_f32(a);
    if (c16_ok(a)) return only(ConvForm::C16);
    if (stream1x1_ok(a)) return only(ConvForm::Stream1x1);
    if (c64_resident_ok(a)) {
        ConvPlan p = only(ConvForm::C64Resident);
        p.blocks = cu_budget;
        return p;
    }
    // from here on a k_order-2 layer is launched with its bias as the accumulators' start (launch_conv_igemm)
    const bool bias_init = a.k_order == 2 ? a.bias != nullptr : a.bias_init != nullptr;
    ConvPlan p;
    // the 4-wave tiles: the wide-step kernel for launches of a few tiles (bit-identical), else the LDS-DMA ring
    auto variant = [&](int mt, int nt, int wm, int wn) { return wm * wn == 4 && wide(p, a, bias_init, mt, nt, wm, wn, false) ? p : tile(ConvForm::Dma, mt, nt, wm, wn, 4); };
    const int c = a.Cout;
    const long blocks128 = cdiv(a.M, 128);
    if (pp_patch(p, a)) return p;
    if (!a.x2 && (pm_patch(p, a) || patch(p, a, false))) return p;      // (a second source: the ping-pong patch kernel above or the implicit GEMMs below)
    if (c % 128 == 0 || c > 160) {
        if (pp(p, a)) return p;
        if (c % 256 == 0 && cdiv(a.M, 256) * (c / 256) >= 200) return tile(ConvForm::Dma, 8, 4, 2, 4, 4);   // 8 waves: 256 px x 256 ch (+12 % on ReID layer3/4 over 256x128)
        if ((blocks128 / 2) * cdiv(c, 128) >= 384) return tile(ConvForm::Dma, 4, 4, 4, 2, 3);           // 8 waves: 256 px x 128 ch
        if (blocks128 * cdiv(c, 128) >= 128) return variant(4, 4, 2, 2);                                 // 128 px x 128 ch
        // too many 64 x 64 tiles for the wide-step kernel, few enough 128 x 128 ones
        if (cdiv(a.M, 64) * cdiv(c, 64) > 256 && wide(p, a, bias_init, 4, 4, 2, 2, false)) return p;
        return variant(2, 2, 2, 2);                                                                      // 64 px x 64 ch (small maps)
    }
    if (c == 144) {
        // the merged first convs of a YOLOv8 detect level (64 box + 80 class channels, Model::Model): one 144-wide tile, the map is read
        // once.  4 waves, one per SIMD: 36 accumulator tiles per wave on the 256-pixel tile need the whole register file
        if (cdiv(a.M, 256) >= 512) return tile(ConvForm::Dma, 4, 9, 4, 1, 4);                            // 256 px x 144 ch
        if (wide(p, a, bias_init, 2, 9, 4, 1, false)) return p;
        return tile(ConvForm::Dma, 2, 9, 4, 1, 4);                                                       // 128 px x 144 ch
    }
    if (c % 80 == 0) {
        // YOLOv8's class branches (Cout = nc = 80).  512 px x 80 ch on 8 waves once there are tiles for every CU:
        // 428 -> 499 TFLOP/s on cls0.1 (80 -> 80, 3x3 at 80 x 80), +7..16 % on the others (tools/conv_bench.py)
        if (cdiv(a.M, 512) >= 256) return tile(ConvForm::Dma, 4, 5, 8, 1, 3);
        return variant(2, 5, 4, 1);                                                                      // 128 px x 80 ch
    }
    if (c % 64 == 0) {
        if (blocks128 >= 512) return variant(4, 4, 4, 1);                                                // 256 px x 64 ch
        // (as above: 256 px tiles where the 128 px grid is too large for the wide-step kernel)
        if (blocks128 * cdiv(c, 64) > 256 && wide(p, a, bias_init, 4, 4, 4, 1, false)) return p;
        return variant(2, 4, 4, 1);                                                                      // 128 px x 64 ch
    }
    if (c % 48 == 0) return variant(2, 3, 4, 1);                                                         // 128 px x 48 ch
    if (c % 32 == 0 || c > 16) return variant(4, 2, 4, 1);                                               // 256 px x 32 ch
    return variant(4, 1, 4, 1);                                                                          // 256 px x 16 ch
}

ConvPlan plan_conv_launch(int dtype, ConvArgs& a, int cu_budget) {
    a.k_order = conv_k_order(dtype, a);      // 3: the stride-2 patch kernel's order (kernels_conv_sp.hip)
    return plan_conv(dtype, a, cu_budget);
}

// ---- the predicates the engine asks at load time

bool conv_tail_supported(int dtype, const ConvArgs& lead, const ConvArgs& tail) {
    static const bool off = getenv("AICAM_NO_TAIL") != nullptr;
    if (off || dtype != AIC_F16) return false;
    if ((lead.Cout != 64 && lead.Cout != 80) || lead.act != 1 || lead.res_mode != 0 || lead.out_f32) return false;
    if (lead.xs || lead.x2) return false;                          // split / second sources are walked by the plain kernels only
    if (tail.KH != 1 || tail.KW != 1 || tail.stride != 1 || tail.pad != 0 || tail.res_mode != 0) return false;
    if (tail.x != lead.y || tail.x_cs != lead.y_cs || tail.x_coff != lead.y_coff || tail.M != lead.M || tail.Cin != lead.Cout) return false;
    if (tail.Cout > lead.Cout || tail.Kp != 32 * ((lead.Cout + 31) / 32) || tail.cout_pad < lead.Cout) return false;
    if (lead.cout_pad < lead.Cout || (tail.y_cs | tail.y_coff) % 8) return false;
    return true;
}

// A split source is walked by the memory-order fast path of the LDS-DMA implicit GEMM only: a 1x1 / 1 / 0 conv without tail whose Cout
// keeps it away from the ping-pong kernels (K of these layers is short anyway) and from the direct kernels.
bool conv_xs_supported(int dtype, const ConvArgs& a, int cs) {
    const int bke = dtype == AIC_F16 ? 32 : 16;
    if (a.KH != 1 || a.KW != 1 || a.stride != 1 || a.pad != 0 || a.w_tail || a.x2 || a.Cin % bke || cs <= 0 || cs % bke || cs >= a.Cin) return false;
    if (a.H % 2 || a.W % 2) return false;
    return a.Kp < 16 * bke;                                       // (pp() takes K >= 16 steps: it has no split-source walk)
}

// A second source rides on the chunk-major walk of the LDS-DMA implicit GEMM / ping-pong kernels: the layer must be one that every batch
// size sends there in that order -- a ping-pong-patch SHAPE (k_order 1) whose Cout takes the 128-multiple branch of plan_conv.
bool conv_x2_supported(int dtype, const ConvArgs& a, int cin2) {
    const int bke = dtype == AIC_F16 ? 32 : 16;
    const int shape = pp_patch_shape(dtype, a);                  // 2: 512 x 128 tile, 3 / 4: 256 x 256 on 16 x 8 / 8 x 4 maps
    if (shape < 2 || a.Cout % 128 || a.w_tail || a.out_f32 || cin2 <= 0 || cin2 % bke) return false;
    return cin2 / bke < a.Cin / bke;                             // its chunk e rides behind the window's chunk e + 1
}

int plan_c64_block(const ConvArgs& c1, const ConvArgs& c2, int cu_budget) {
    static const bool on = [] { const char* e = getenv("AICAM_C64_BLOCK"); return !e || atoi(e) != 0; }();
    auto conv64 = [](const ConvArgs& a) {
        return a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && a.Cin == 64 && a.Cout == 64 && !a.out_f32 && a.Kp == 576 && a.act == 2 &&
               a.Ho == a.H && a.Wo == a.W && (a.x_cs | a.x_coff | a.y_cs | a.y_coff) % 8 == 0;
    };
    if (!on || !conv64(c1) || !conv64(c2) || c1.res_mode != 0 || c2.res_mode != 1) return 0;
    if (c1.W != 32 || c1.H % 4 || c1.H != c2.H || c2.W != 32 || c1.M != c2.M || c1.M < 1500000) return 0;
    if (c2.x != c1.y || c2.x_cs != c1.y_cs || c2.x_coff != c1.y_coff) return 0;            // conv2 reads what conv1 writes
    if (c2.res != c1.x || c2.r_cs != c1.x_cs || c2.r_coff != c1.x_coff) return 0;        // and adds the block input
    if ((long)c1.M * c1.x_cs >= B31 || (long)c2.M * c2.y_cs >= B31) return 0;
    // images per block: shorter-lived blocks than one persistent block per CU flow around the side stream's NMS blocks (round 3: 9 490 ->
    // 9 553 frames/s at 16).  12 .. 16 images per block, whichever wastes least of the last round of blocks over the CU budget (round 5,
    // 15 360 crops: 12 -> 1 280 blocks = 5 rounds; the layer alone 2 065 -> 2 000 us per conv).
    const int n_img = c1.M / (c1.H * c1.W), cus = (cu_budget + 7) / 8 * 8;
    long best = -1;
    int ipb = 0;
    for (int i = 12; i <= 16; ++i) {
        const long blocks = (n_img + i - 1) / i, rounds = (blocks + cus - 1) / cus;
        const long waste = (rounds * cus - blocks) * 1000 / (rounds * cus);           // idle share of the CUs' block slots, per mille
        if (best < 0 || waste < best) best = waste, ipb = i;
    }
    return ipb;
}

bool plan_c2f16(const ConvArgs& c1, const ConvArgs& m1, const ConvArgs& m2, const ConvArgs& c2) {
    static const bool off = getenv("AICAM_NO_C2F") != nullptr;
    if (off) return false;
    auto one = [](const ConvArgs& c, int cin, int cout, int kp) {
        return c.KH == 1 && c.KW == 1 && c.stride == 1 && c.pad == 0 && c.Cin == cin && c.Cout == cout && c.Kp == kp && c.act == 1 &&
               c.res_mode == 0 && !c.out_f32;
    };
    auto three = [](const ConvArgs& c) {
        return c.KH == 3 && c.KW == 3 && c.stride == 1 && c.pad == 1 && c.Cin == 16 && c.Cout == 16 && c.Kp == 160 && c.act == 1 && !c.out_f32;
    };
    if (!one(c1, 32, 32, 32) || !one(c2, 48, 32, 64) || !three(m1) || !three(m2) || m1.res_mode != 0 || m2.res_mode != 2) return false;
    const int H = c1.H, W = c1.W;
    for (const ConvArgs* c : {&c1, &m1, &m2, &c2})
        if (c->H != H || c->W != W || c->Ho != H || c->Wo != W || c->M != c1.M) return false;
    if (H % 8 || W % 32) return false;                              // the kernel's 8 x 32 output tiles
    // wiring: cv1 writes cat[0:32]; m.cv1 reads cat[16:32] -> tmp; m.cv2 reads tmp, adds cat[16:32], writes cat[32:48]; cv2 reads cat[0:48]
    const void* cat = c1.y;
    if (c1.y_coff != 0 || m1.x != cat || m1.x_coff != 16 || m1.x_cs != c1.y_cs || m2.x != m1.y || m2.x_coff != m1.y_coff || m2.x_cs != m1.y_cs ||
        m2.y != cat || m2.y_coff != 32 || m2.res != cat || m2.r_coff != 16 || m2.r_cs != c1.y_cs || c2.x != cat || c2.x_coff != 0 ||
        c2.x_cs != c1.y_cs || c1.y_cs < 48)
        return false;
    return (c1.x_cs | c1.x_coff | c2.y_cs | c2.y_coff) % 8 == 0;
}

}  // namespace aic
