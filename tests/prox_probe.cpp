// prox_probe.cpp -- csrc/prox_math.hpp on the CPU, stand-alone: tests/test_prox_host.py builds this with the system compiler and
// -fsanitize=address,undefined, runs it, and compares every printed value with tests/prox_oracle.py.  One line per table, a key first.
#include <cstdio>
#include <string>
#include <vector>

#include "../ai-camera_amd/csrc/prox_math.hpp"

using namespace aic;

int main() {
    // isq: v:r at 0, 1 and around every square and power of two up to 2^61
    std::printf("isq");
    std::vector<long long> vs = {0, 1, 2, 3};
    for (int b = 1; b <= 30; ++b)
        for (long long k : {(1ll << b) - 1, 1ll << b, (1ll << b) + 1, 3ll << (b - 1)}) {
            vs.push_back(k * k - 1), vs.push_back(k * k), vs.push_back(k * k + 1);
        }
    for (int b = 2; b <= 61; ++b) vs.push_back((1ll << b) - 1), vs.push_back(1ll << b), vs.push_back((1ll << b) + 1);
    for (long long v : vs)
        if (v >= 0 && v <= (1ll << 61) + 1) std::printf(" %lld:%lld", v, prox_isqrt(v));
    std::printf("\n");
    // fdiv: a:b:floor(a / b), negative numerators among them
    std::printf("fdiv");
    for (long long a : {-(1ll << 60), -1000001ll, -7ll, -6ll, -1ll, 0ll, 1ll, 6ll, 7ll, 1000001ll, 1ll << 60})
        for (long long b : {1ll, 2ll, 3ll, 7ll, 1000ll, (1ll << 46) + 1}) std::printf(" %lld:%lld:%lld", a, b, prox_floor_div(a, b));
    std::printf("\n");
    // plc: the ground map of tests/prox_cases.py and two others on a grid of anchors: fx fy placed gx gy
    const ProxGround maps[3] = {{{1024, 0, 0, 0, 1024, 0, 0, -1, 40}, 14}, {{2, 0, 0, 0, 2, 0, 0, 0, 1}, 0}, {{-(1 << 30), 1 << 30, 12345, 7, -9, 1 << 30, 3, 5, -100}, 3}};
    for (int m = 0; m < 3; ++m) {
        std::printf("plc %d", m);
        for (int fy = 0; fy < 96; fy += 5)
            for (int fx = 0; fx < 128; fx += 9) {
                int gx, gy;
                const bool ok = prox_place(maps[m], fx, fy, &gx, &gy);
                std::printf(" %d:%d:%d:%d:%d", fx, fy, (int)ok, gx, gy);
            }
        std::printf("\n");
    }
    // near / dst: both metrics on a lattice around the boundary: (0, 0, ha) against (dx, dy, hb)
    for (int metric = 0; metric < 2; ++metric) {
        const ProxRules r{metric, metric == PROX_GROUND ? 13 : 700, 384, 3, 2, 1, 5, 70};
        std::printf("near %d", metric);
        for (int ha : {10, 20, 30, 31})
            for (int hb : {20, 30})
                for (int dx = -30; dx <= 30; ++dx)
                    for (int dy : {0, 5, 12, 13, 14}) std::printf(" %d", (int)prox_near(r, 0, 0, ha, dx, dy, hb));
        std::printf("\n");
        std::printf("dst %d", metric);
        for (int ha : {1, 20, 32767})
            for (int dx : {0, 1, 7, 127, 1 << 15, 1 << 25})
                for (int dy : {0, 3, -(1 << 25)})
                    if (metric == PROX_GROUND || (dx <= (1 << 15) && dy > -(1 << 15)))
                        std::printf(" %d:%d:%d:%d", ha, dx, dy, prox_distance(metric, 0, 0, ha, dx, dy, 20));
        std::printf("\n");
        std::printf("mov %d", metric);
        for (int hc : {1, 20, 32767})
            for (int dx : {0, 1, -7, 127, -(1 << 15)})
                for (int dy : {0, 3, 1 << 15}) std::printf(" %d:%d:%d:%d", hc, dx, dy, prox_moved(metric, dx, dy, hc));
        std::printf("\n");
    }
    // spd: a slot's smoothed speed and gait along a sequence of measurements (moved:dt), speed_shift 0..12
    for (int shift : {0, 1, 2, 12}) {
        std::printf("spd %d", shift);
        int v = 0, gait = 0;
        const int seq[][2] = {{100, 1}, {0, 1}, {7, 2}, {1 << 25, 1}, {1 << 30, 1}, {0, 1}, {0, 3}, {5, 1}, {1000, 7}, {0, 1}, {0, 1}, {0, 1}};
        for (const auto& q : seq) {
            v = prox_v_q8(v, gait, prox_speed(q[0], q[1]), shift);
            gait = prox_gait(v, 5, 70);
            std::printf(" %d:%d", v, gait);
        }
        std::printf("\n");
    }
    // jdg: a pair's entry along a sequence of judgements (1 near, 0 far), link_ticks 3, unlink_ticks 2, then saturation of on and off
    std::printf("jdg");
    int x = 0, since = 0, frame = 0;
    for (char c : std::string("1101110100111001")) {
        const int kind = prox_judge(c == '1', 3, 2, frame, &x, &since);
        std::printf(" %d:%d:%d:%d:%d", kind, prox_linked(x), prox_on(x), prox_off(x), since);
        ++frame;
    }
    x = prox_pack(1, 32766, 0);
    for (int k = 0; k < 3; ++k) prox_judge(true, 3, 2, frame++, &x, &since), std::printf(" 0:%d:%d:%d:%d", prox_linked(x), prox_on(x), prox_off(x), since);
    x = prox_pack(0, 0, 32766);
    for (int k = 0; k < 3; ++k) prox_judge(false, 3, 2, frame++, &x, &since), std::printf(" 0:%d:%d:%d:%d", prox_linked(x), prox_on(x), prox_off(x), since);
    std::printf("\n");
    // idx: the triangle's index is a bijection onto 0 .. n (n - 1) / 2 - 1
    std::printf("idx");
    for (int n : {2, 3, 128, 512}) {
        std::vector<char> seen((size_t)n * (n - 1) / 2, 0);
        bool ok = true;
        for (int b = 1; b < n; ++b)
            for (int a = 0; a < b; ++a) {
                const int i = prox_pair_index(a, b);
                ok = ok && i >= 0 && i < (int)seen.size() && !seen[i];
                if (i >= 0 && i < (int)seen.size()) seen[i] = 1;
            }
        std::printf(" %d:%d", n, (int)ok);
    }
    std::printf("\n");
    return 0;
}
