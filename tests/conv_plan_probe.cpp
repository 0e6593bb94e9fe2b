// conv_plan_probe.cpp -- test-only entry point into the conv planner (ai-camera_amd/csrc/conv_plan.cpp), built with the system g++ by
// tests/test_conv_plan.py.  Not part of libaicam.so.
#include "../ai-camera_amd/csrc/conv_plan.hpp"

using namespace aic;

// L: H, W, Cin, Ho, Wo, Cout, K (square window), stride, act, res_mode, n (images), tail Cout (0: none), Cin2 (0: none), Cs (0: none),
// out_f32, n_dev (1: a device-side item count is in force, ConvArgs::n_dev).  Laid out as the engine lays out a dense layer.  out: k_order, form, mt, nt, wm, wn, nstage, th, tw, cpp, pitch, kord, g, tail,
// x2, run, blocks, then conv_tail_supported, conv_x2_supported, conv_xs_supported.  Returns 0, or -1 when plan_conv refuses the layer.
extern "C" int probe_plan(int dtype, const int* L, int cu_budget, long* out) {
    static const char page[256] = {0};
    const int bke = dtype == AIC_F16 ? 32 : 16, k = L[6];
    ConvArgs a{};
    a.H = L[0], a.W = L[1], a.Cin = L[2], a.Ho = L[3], a.Wo = L[4], a.Cout = L[5], a.KH = a.KW = k, a.stride = L[7], a.pad = k / 2;
    a.act = L[8], a.res_mode = L[9], a.M = L[10] * a.Ho * a.Wo, a.out_f32 = L[14];
    a.x_cs = a.Cin, a.y_cs = a.Cout, a.r_cs = a.res_mode ? a.Cout : 0;
    a.Kp = (k * k * a.Cin + bke - 1) / bke * bke, a.cout_pad = (a.Cout + 127) / 128 * 128;
    for (int kh = 0; kh < k; ++kh) a.tap_rows |= 1u << (kh * k);
    a.x = a.w = a.zero = page, a.y = (void*)page, a.bias = reinterpret_cast<const float*>(page);
    if (a.res_mode) a.res = page;
    if (L[15]) a.n_dev = reinterpret_cast<const int*>(page);
    ConvArgs t{};
    if (L[11]) {
        t.x = a.y, t.x_cs = a.y_cs, t.M = a.M, t.Cin = a.Cout, t.Cout = L[11], t.KH = t.KW = 1, t.stride = 1, t.Kp = 32 * ((a.Cout + 31) / 32);
        t.cout_pad = (t.Cout + 127) / 128 * 128, t.y_cs = t.Cout;
    }
    out[17] = conv_tail_supported(dtype, a, t);
    out[18] = conv_x2_supported(dtype, a, L[12]);
    out[19] = conv_xs_supported(dtype, a, L[13]);
    if (L[11]) a.w_tail = page, a.t_cout = t.Cout, a.t_kp = t.Kp, a.t_y_cs = t.y_cs;
    if (L[12]) a.x2 = page, a.Cin2 = L[12], a.x2_cs = L[12], a.H2 = a.H * 2, a.W2 = a.W * 2, a.s2 = 2, a.Kp += L[12];
    if (L[13]) a.xs = page, a.Cs = L[13], a.xs_cs = L[13], a.Hs = a.H / 2, a.Ws = a.W / 2;
    a.k_order = conv_k_order(dtype, a);
    out[0] = a.k_order;
    try {
        const ConvPlan p = plan_conv(dtype, a, cu_budget);
        const long v[] = {(long)p.form, p.mt, p.nt, p.wm, p.wn, p.nstage, p.th, p.tw, p.cpp, p.pitch, p.kord, p.g, p.tail, p.x2, p.run, p.blocks};
        for (int i = 0; i < 16; ++i) out[1 + i] = v[i];
    } catch (const Error&) {
        return -1;
    }
    return 0;
}

// The 64-channel BasicBlock pair on an H x 32 map at n images, as the engine lays it out: plan_c64_block's images per block (0: not fused).
extern "C" int probe_c64_block(int H, int n, int cu_budget) {
    static const char px[256] = {0}, pm[256] = {0}, py[256] = {0};
    ConvArgs c1{}, c2{};
    for (ConvArgs* c : {&c1, &c2}) {
        c->H = c->Ho = H, c->W = c->Wo = 32, c->Cin = c->Cout = 64, c->KH = c->KW = 3, c->stride = 1, c->pad = 1, c->act = 2, c->Kp = 576;
        c->M = n * H * 32, c->x_cs = c->y_cs = 64, c->cout_pad = 128;
    }
    c1.x = px, c1.y = (void*)pm, c2.x = pm, c2.y = (void*)py, c2.res = px, c2.r_cs = 64, c2.res_mode = 1;
    return plan_c64_block(c1, c2, cu_budget);
}
