// row_band_probe.cpp -- test-only entry points into the row-band planner (ai-camera_amd/csrc/row_band.cpp), built with the system g++
// by tests/test_row_band.py.  Not part of libaicam.so.
#include "../ai-camera_amd/csrc/row_band.hpp"

using namespace aic;

// ops: 12 ints per op -- conv, src, src_c0, src_cn, dst, dst_c0, dst_cn, k, stride, pad, res (-1: none), res_c0.
// out: 3 ints per op -- full, lo, hi.
extern "C" void probe_row_bands(int n_ops, const int* ops, int n_bufs, const int* buf_h, int top, int unpad_h, int side_pad, int* out) {
    std::vector<RbOp> ro(n_ops);
    for (int i = 0; i < n_ops; ++i) {
        const int* v = ops + 12 * i;
        RbOp& r = ro[i];
        r.conv = v[0], r.src = v[1], r.src_c0 = v[2], r.src_cn = v[3], r.dst = v[4], r.dst_c0 = v[5], r.dst_cn = v[6];
        r.k = v[7], r.stride = v[8], r.pad = v[9], r.res = v[10], r.res_c0 = v[11];
    }
    const std::vector<RowBand> b = plan_row_bands(ro, std::vector<int>(buf_h, buf_h + n_bufs), top, unpad_h, side_pad != 0);
    for (int i = 0; i < n_ops; ++i) out[3 * i] = b[i].full, out[3 * i + 1] = b[i].lo, out[3 * i + 2] = b[i].hi;
}

extern "C" void probe_tile_window(int y0, int rows, int th, int Ho, int* out) {
    const TileWindow t = tile_window(y0, rows, th, Ho);
    out[0] = t.origin, out[1] = t.tiles;
}

// steps: 8 ints per step -- op, dst, dst_c0, dst_cn, Ho, th, exact, number of reads; reads (all steps' in order): 7 ints each -- buf, c0,
// cn, all, stride, halo_lo, halo_hi.  bands: 3 ints per op (full, lo, hi).  out: 2 ints per step -- y0, rows (0: the full map).
extern "C" void probe_row_windows(int n_steps, const int* steps, const int* reads, int n_ops, const int* bands, int* out) {
    std::vector<RbStep> st(n_steps);
    const int* r = reads;
    for (int i = 0; i < n_steps; ++i) {
        const int* v = steps + 8 * i;
        RbStep& s = st[i];
        s.op = v[0], s.dst = v[1], s.dst_c0 = v[2], s.dst_cn = v[3], s.Ho = v[4], s.th = v[5], s.exact = v[6] != 0;
        for (int k = 0; k < v[7]; ++k, r += 7) {
            RbRead rr;
            rr.buf = r[0], rr.c0 = r[1], rr.cn = r[2], rr.all = r[3] != 0, rr.stride = r[4], rr.halo_lo = r[5], rr.halo_hi = r[6];
            s.reads.push_back(rr);
        }
    }
    std::vector<RowBand> b(n_ops);
    for (int i = 0; i < n_ops; ++i) b[i].full = bands[3 * i] != 0, b[i].lo = bands[3 * i + 1], b[i].hi = bands[3 * i + 2];
    const std::vector<RowWindow> w = plan_row_windows(st, b);
    for (int i = 0; i < n_steps; ++i) out[2 * i] = w[i].y0, out[2 * i + 1] = w[i].rows;
}
