// row_band.hpp -- which output rows of every op can depend on the frame when the input is a letterboxed picture with flat borders
// above and below it, and the row windows the launches take from that.  Plain C++ (no HIP header): the CPU test
// (tests/test_row_band.py) builds row_band.cpp with the system compiler.
//
// A letterboxed 16:9 frame carries the picture in rows [top, top + unpad_h) of the engine's input; the rows around it are the same
// grey for every frame.  Through convs with small windows a share of every early activation map therefore depends on the weights and
// the grey value only.  Activation buffers are never aliased between tensors, so those rows can be written once (a full run) and left
// where they are: later runs of the same geometry launch only the tile rows that cover the band.
#pragma once
#include <vector>

namespace aic {

// closed interval [lo, hi] of rows of an op's output map that can depend on the frame; full: every row (lo = 0, hi = H - 1)
struct RowBand { int lo = 0, hi = -1; bool full = true; };

// one op of the engine's list as the planner sees it
struct RbOp {
    int conv = 0;                      // 1: a conv the planner models (activation dtype in and out, one source); 0: anything else -> "all rows"
    int src = 0, src_c0 = 0, src_cn = 0;
    int dst = 0, dst_c0 = 0, dst_cn = 0;
    int k = 1, stride = 1, pad = 0;
    int res = -1, res_c0 = 0;          // residual slice (dst_cn channels of buffer res), -1: none
};

// Bands of every op for a picture in rows [top, top + unpad_h) of buffer 0.  buf_h: rows of every buffer.  side_pad: the picture has
// borders left / right (portrait sources): out of scope, every op gets all rows.
//  * a conv (k, stride s, pad p) maps input rows [a, b] to the output rows whose windows touch them:
//    [ceil((a + p - k + 1) / s), floor((b + p) / s)], clipped to the map;
//  * bands are tracked per (buffer, channel slice): a reader takes the hull over the slices it reads (a 1x1 over a concat buffer, a
//    residual add); a slice nobody has written is unknown -> all rows;
//  * what the planner does not model, and everything downstream of it, gets all rows;
//  * a band that leaves fewer than `min_saved` rows of the map out counts as all rows.
constexpr int kRowBandMinSaved = 8;
std::vector<RowBand> plan_row_bands(const std::vector<RbOp>& ops, const std::vector<int>& buf_h, int top, int unpad_h, bool side_pad);

// ---- windows: what one LAUNCH (a conv, a conv with its tail, a fused block) computes of its output map
struct RbRead {
    int buf = 0, c0 = 0, cn = 0;
    bool all = false;                  // reads the whole map whatever it computes
    int stride = 1, halo_lo = 0, halo_hi = 0;   // output rows [a, b] read input rows [a * stride - halo_lo, b * stride + halo_hi]
};
struct RbStep {
    int op = 0;                        // the op whose output the launch writes (the last op it covers): its band is the launch's
    int dst = 0, dst_c0 = 0, dst_cn = 0, Ho = 0;
    int th = 0;                        // tile rows of the kernel's window form; 0: the launch has none and always computes the full map
    bool exact = false;                // the kernel stores exactly the window's rows; otherwise whole tiles (tile_window)
    std::vector<RbRead> reads;
};
struct RowWindow { int y0 = 0, rows = 0; };     // rows == 0: the full map

// The launch grid of a window on tiles of th rows: `tiles` tile rows from output row `origin`.  The origin need not be a multiple of
// th; it is clamped so that the last tile ends inside the map (the rows recomputed in front of the window get the bits they had).
// rows == 0: the full map, ceil(Ho / th) tile rows from row 0.
struct TileWindow { int origin, tiles; };
TileWindow tile_window(int y0, int rows, int th, int Ho);

// One window per step.  A step's window is its band, except:
//  * a slice with MORE THAN ONE writer in the list (the bottleneck scratch of a C2f with n = 2: m0.cv1 and m1.cv1 share a buffer) has
//    no persistent rows -- what lies outside a writer's band is the other writer's output.  Each writer computes the hull of its own
//    band and of every row its readers (the steps that read the slice before the next writer, in list order, cyclically) read for
//    what THEY compute -- their whole tiles, not only their bands;
//  * a step whose tiles would cover the map anyway, a step without a window form and a step without a band run full.
std::vector<RowWindow> plan_row_windows(const std::vector<RbStep>& steps, const std::vector<RowBand>& bands);

}  // namespace aic
