// prox_math.hpp -- the arithmetic of the proximity stage (prox.hpp, kernels_prox.hip), once for host and device: the
// integer square root, the floor division, the ground map of an anchor, the near rule and the reported distance of both metrics, the step
// of a slot's speed and its gait, and the packed pair entry.  Integer arithmetic only; nothing but the standard library, so a stand-alone
// program builds it with the system compiler (tests/prox_probe.cpp).  tests/prox_oracle.py is the specification.
//
// Ranges.  fx, fy < 2^15 (doubled pixels of a frame of at most 16384); |H[k]| <= 2^30, so |nx|, |ny|, |den| <= 2^30 (2^15 + 2^15 + 2) <
// 2^47 and, shifted by at most 14, < 2^61: every intermediate of the ground map fits int64.  |gx|, |gy| <= 2^24, so a squared distance
// is at most 2^51 (metric 0); metric 1: D2 < 2^31, 1 000 000 D2 < 2^51 and near^2 (hc_i + hc_j)^2 <= 2^24 2^32 = 2^56 < 2^57.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROX_HD __host__ __device__ inline
#else
#define PROX_HD inline
#endif

namespace aic {

enum { PROX_GROUND = 0, PROX_BODY = 1 };
enum { PROX_LINK = 1, PROX_UNLINK = 2 };
enum { PROX_F_PLACED = 8, PROX_F_NEW = 16 };                                  // behind SLOT_F_VALID 1, FIRST 2, NONEMPTY 4
constexpr int PROX_SAT = 1 << 30;          // where dist, max_v_q8 and every slot counter stop
constexpr int PROX_G_MAX = 1 << 24;        // |gx|, |gy| of a placed row
constexpr int PROX_ON_MAX = 32767;         // where `on` and `off` of a pair stop
constexpr int PROX_SPEED_MAX = 1 << 22;    // speed << 8 stays at or below 2^30

// what the kernel needs of aic_prox_config's rules (option changes them between calls)
struct ProxRules {
    int metric, near, height_ratio_q8, link_ticks, unlink_ticks, speed_shift, still_speed, run_speed;
};
// a stream's ground map: gx = floor(((H0 fx + H1 fy + 2 H2) << shift) / (H6 fx + H7 fy + 2 H8)), gy from H3..H5
struct ProxGround {
    int h[9], shift;
};

PROX_HD int prox_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
PROX_HD int prox_sat_add(int a, int b) { return a + b > PROX_SAT ? PROX_SAT : a + b; }      // a <= 2^30, 0 <= b < 2^30

// the largest r with r * r <= v, 0 <= v < 2^62, bit by bit
PROX_HD long long prox_isqrt(long long v) {
    long long r = 0, bit = 1ll << 60;
    while (bit > v) bit >>= 2;
    while (bit) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
        bit >>= 2;
    }
    return r;
}

// floor(a / b) for b > 0
PROX_HD long long prox_floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// the anchor's place on the ground (metric 0); false: den <= 0, or beyond 2^24
PROX_HD bool prox_place(const ProxGround& m, int fx, int fy, int* gx, int* gy) {
    const long long nx = (long long)m.h[0] * fx + (long long)m.h[1] * fy + 2ll * m.h[2];
    const long long ny = (long long)m.h[3] * fx + (long long)m.h[4] * fy + 2ll * m.h[5];
    const long long den = (long long)m.h[6] * fx + (long long)m.h[7] * fy + 2ll * m.h[8];
    *gx = 0, *gy = 0;
    if (den <= 0) return false;
    const long long x = prox_floor_div(nx * (1ll << m.shift), den), y = prox_floor_div(ny * (1ll << m.shift), den);
    if (x > PROX_G_MAX || x < -PROX_G_MAX || y > PROX_G_MAX || y < -PROX_G_MAX) return false;
    *gx = (int)x, *gy = (int)y;
    return true;
}

PROX_HD long long prox_d2(int ax, int ay, int bx, int by) {
    const long long dx = (long long)ax - bx, dy = (long long)ay - by;
    return dx * dx + dy * dy;
}

PROX_HD bool prox_near(const ProxRules& r, int ax, int ay, int ah, int bx, int by, int bh) {
    const long long d2 = prox_d2(ax, ay, bx, by), nn = (long long)r.near * r.near;
    if (r.metric == PROX_GROUND) return d2 <= nn;
    const int lo = ah < bh ? ah : bh, hi = ah < bh ? bh : ah;
    const long long hs = (long long)ah + bh;
    return 256ll * hi <= (long long)r.height_ratio_q8 * lo && 1000000ll * d2 <= nn * hs * hs;
}

PROX_HD int prox_distance(int metric, int ax, int ay, int ah, int bx, int by, int bh) {
    const long long d2 = prox_d2(ax, ay, bx, by);
    return (int)(metric == PROX_GROUND ? prox_isqrt(d2) : prox_isqrt(1000000ll * d2) / (ah + bh));
}

// how far a slot moved since it was last seen: ground units, or per mille of the row's height
PROX_HD int prox_moved(int metric, int dx, int dy, int hc) {
    const long long s = prox_isqrt((long long)dx * dx + (long long)dy * dy);
    return (int)(metric == PROX_GROUND ? s : 1000 * s / (2 * hc));
}

PROX_HD int prox_speed(int moved, int dt) {
    const int v = moved / dt;
    return v > PROX_SPEED_MAX ? PROX_SPEED_MAX : v;
}

// the smoothed speed behind one measurement; gait 0: the first one
PROX_HD int prox_v_q8(int v_q8, int gait, int speed, int speed_shift) { return gait == 0 ? speed << 8 : v_q8 + (((speed << 8) - v_q8) >> speed_shift); }

PROX_HD int prox_gait(int v_q8, int still_speed, int run_speed) {
    const int v = v_q8 >> 8;
    return v <= still_speed ? 1 : v >= run_speed ? 3 : 2;
}

// a pair entry, 8 bytes: x = linked | on << 1 | off << 16, y = since
PROX_HD int prox_pack(int linked, int on, int off) { return linked | on << 1 | off << 16; }
PROX_HD int prox_linked(int x) { return x & 1; }
PROX_HD int prox_on(int x) { return (x >> 1) & 32767; }
PROX_HD int prox_off(int x) { return (x >> 16) & 32767; }
// the entry of slots a < b in a stream's triangle of max_tracks (max_tracks - 1) / 2 entries
PROX_HD int prox_pair_index(int a, int b) { return b * (b - 1) / 2 + a; }

// One judgement of a pair.  Returns the kind of the event it raises (0: none); *x, *since are the entry.
PROX_HD int prox_judge(bool near, int link_ticks, int unlink_ticks, int frame, int* x, int* since) {
    int linked = prox_linked(*x), on = prox_on(*x), off = prox_off(*x), kind = 0;
    if (near) {
        on = on < PROX_ON_MAX ? on + 1 : PROX_ON_MAX, off = 0;
        if (!linked && on >= link_ticks) linked = 1, *since = frame, kind = PROX_LINK;
    } else {
        off = off < PROX_ON_MAX ? off + 1 : PROX_ON_MAX, on = 0;
        if (linked && off >= unlink_ticks) linked = 0, kind = PROX_UNLINK;
    }
    *x = prox_pack(linked, on, off);
    return kind;
}

}  // namespace aic
