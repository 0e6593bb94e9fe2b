// sparse_box_probe.cpp -- test-only entry point into the conv planner (ai-camera_amd/csrc/conv_plan.cpp) for launches with a pixel list
// (ConvArgs::pix_list), built with the system g++ by tests/test_sparse_box_plan.py.  Not part of libaicam.so.
#include "../ai-camera_amd/csrc/conv_plan.hpp"

using namespace aic;

// L: H, W (3x3 / 1 / 1, 64 -> 64 channels, SiLU, fp16 as the engine lays a detect level's box convs out), n images, tail (1: the 64 -> 64
// 1x1 in the epilogue, decoding boxes), listed (1: with a pixel list), dtype.  out: k_order, form, mt, nt, wm, wn, nstage, tail, list.
// Returns 0, or -1 when the planner refuses the launch.
extern "C" int probe_list_plan(const int* L, int cu_budget, long* out) {
    static const char page[256] = {0};
    static float box[4];
    const int dtype = L[5];
    ConvArgs a{};
    a.H = a.Ho = L[0], a.W = a.Wo = L[1], a.Cin = a.Cout = 64, a.KH = a.KW = 3, a.stride = 1, a.pad = 1, a.act = 1;
    a.M = L[2] * a.Ho * a.Wo, a.x_cs = a.y_cs = 64, a.Kp = 576, a.cout_pad = 128, a.tap_rows = 0x49u;
    a.x = a.w = a.zero = page, a.y = (void*)page, a.bias = reinterpret_cast<const float*>(page);
    if (L[3]) {
        a.w_tail = page, a.b_tail = reinterpret_cast<const float*>(page), a.t_cout = 64, a.t_kp = 64, a.t_y_cs = 64, a.t_out_f32 = 1;
        a.t_box = box, a.t_hw = a.Ho * a.Wo, a.t_na = a.t_hw, a.t_w = a.Wo, a.t_stride = 8;
    }
    if (L[4]) a.pix_list = a.pix_count = reinterpret_cast<const int*>(page);
    try {
        const ConvPlan p = plan_conv_launch(dtype, a, cu_budget);
        const long v[] = {a.k_order, (long)p.form, p.mt, p.nt, p.wm, p.wn, p.nstage, p.tail, p.list};
        for (int i = 0; i < 9; ++i) out[i] = v[i];
    } catch (const Error&) {
        return -1;
    }
    return 0;
}
