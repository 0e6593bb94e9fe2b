// heat_math.hpp -- the arithmetic of the heat-map stage (heat.hpp, kernels_heat.hip), once for host and device: the
// anchor and its cell, the octant of a step, the Q8 logarithm and the level of a cell, the bilinear weights of a pixel, the blend and the
// default colour ramp.  Integer arithmetic only; nothing but the standard library, so a stand-alone program builds it with the system
// compiler (tests/heat_probe.cpp).  tests/heat_oracle.py is the specification.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HEAT_HD __host__ __device__ inline
#else
#define HEAT_HD inline
#endif

namespace aic {

constexpr int HEAT_LAYERS = 12;
enum { HEAT_VISITS = 0, HEAT_DWELL, HEAT_STARTS, HEAT_ENDS, HEAT_DIR0 };
constexpr int HEAT_SAT = 1 << 30;          // where every layer cell and every slot counter stops
constexpr int HEAT_Q_MAX = 65280;          // the level of the stream's hottest cell (255 * 256)
enum { HEAT_FOOT = 0, HEAT_CENTRE = 1 };
enum { HEAT_LINEAR = 0, HEAT_LOG = 1 };

HEAT_HD int heat_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
HEAT_HD int heat_sat_add(int a, int b) { return a + b > HEAT_SAT ? HEAT_SAT : a + b; }      // a <= 2^30, 0 <= b < 2^30

// the anchor of a row in doubled pixels, clamped into the frame (|coord| <= 2^20, so the sums stay inside int32)
HEAT_HD int heat_fx(int x1, int x2, int w) { return heat_clamp(x1 + x2, 0, 2 * w - 1); }
HEAT_HD int heat_fy(int y1, int y2, int h, int anchor) { return heat_clamp(anchor == HEAT_CENTRE ? y1 + y2 : 2 * y2, 0, 2 * h - 1); }

// the octant of a step (dx, dy) != (0, 0), image coordinates, clockwise from east: 5 / 12 stands for tan 22.5 degrees
HEAT_HD int heat_octant(int dx, int dy) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;                 // <= 2^15: 12 a stays inside int32
    if (12 * ay < 5 * ax) return dx > 0 ? 0 : 4;
    if (12 * ax < 5 * ay) return dy > 0 ? 2 : 6;
    return dy > 0 ? (dx > 0 ? 1 : 3) : (dx > 0 ? 7 : 5);
}

// u(v): the Q8 base-2 logarithm of v + 1 for 0 <= v <= 2^30: floor(log2) << 8 | the next 8 bits below the leading one
HEAT_HD int heat_log_q8(int v) {
    const unsigned n = (unsigned)v + 1u;
    int b = 0;
    while ((n >> b) > 1u) ++b;
    const unsigned m = b >= 8 ? n >> (b - 8) : n << (8 - b);
    return (b << 8) | (int)(m & 255u);
}

// the level 0..65280 of a cell holding v when the stream's maximum is M >= 1
HEAT_HD int heat_level(int v, int M, int scale) {
    if (scale == HEAT_LINEAR) return (int)(((long long)v * HEAT_Q_MAX) / M);
    return (int)(((unsigned)heat_log_q8(v) * (unsigned)HEAT_Q_MAX) / (unsigned)heat_log_q8(M));      // u <= 7935: below 2^31
}

// the two neighbours and the weight of pixel x along one axis: cells of 1 << lc pixels, n of them.  w in 0 .. 2 cell - 1 belongs to i1.
HEAT_HD void heat_axis(int x, int lc, int n, int* i0, int* i1, int* w) {
    const int d = 2 * x + 1 - (1 << lc);                                      // doubled pixels from the centre of cell 0
    const int i = d >> (lc + 1);                                              // floor: -1 in the first half cell
    *w = d & ((2 << lc) - 1);                                                 // d - 2 cell i
    *i0 = heat_clamp(i, 0, n - 1), *i1 = heat_clamp(i + 1, 0, n - 1);
}

// L in 0..255 from the four levels
HEAT_HD int heat_bilinear(int q00, int q01, int q10, int q11, int wx, int wy, int lc) {
    const int c2 = 2 << lc;
    const int top = q00 * (c2 - wx) + q01 * wx, bot = q10 * (c2 - wx) + q11 * wx;         // <= 65280 * 64
    return (int)(((unsigned)top * (unsigned)(c2 - wy) + (unsigned)bot * (unsigned)wy + (128u << (2 * lc + 2))) >> (2 * lc + 2 + 8));
}

HEAT_HD int heat_blend(int in, int lut, int a) { return (in * (256 - a) + lut * a + 128) >> 8; }

// the default colour ramp at L, channel c of R G B
HEAT_HD int heat_ramp(int L, int c) {
    const int at[5] = {0, 64, 128, 192, 255};
    const int rgb[5][3] = {{0, 0, 160}, {0, 160, 255}, {0, 255, 0}, {255, 255, 0}, {255, 0, 0}};
    int k = 0;
    while (k < 3 && L >= at[k + 1]) ++k;
    const int n = at[k + 1] - at[k], j = L - at[k];
    return (rgb[k][c] * (n - j) + rgb[k + 1][c] * j + n / 2) / n;
}

}  // namespace aic
