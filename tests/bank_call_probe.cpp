// bank_call_probe.cpp -- prints what ai-camera_amd/csrc/bank_call.hpp computes: the staging and output offsets of the four frame-bank
// stages over a cross product of calls, the launch planner's cuts, and what fill() writes into buffers of exactly the size the layout
// names.  tests/test_bank_call_host.py builds it with the system compiler under the address and undefined-behaviour sanitizers, runs it
// as a child process and compares every line with the call sites' formulas as they were.  No HIP, no GPU.
#include <cstdio>
#include <vector>

#include "../ai-camera_amd/csrc/bank_call.hpp"

using namespace aic;

struct Site { const char* name; bool mode; int event_ints; };             // event_ints 0: no slot output
static const Site SITES[] = {{"bestshot", true, 16}, {"colours", true, 48}, {"scene", false, 0}, {"left", false, 0}};

static void layouts() {
    for (const Site& site : SITES)
        for (int S : {1, 2, 3, 256})
            for (long F : {0L, 1L, 3L, 5L, 17L})
                for (long total : {0L, 1L, 5L, 513L})
                    for (int host = 0; host < 2; ++host) {
                        const BankStage bs = BankStage::bank(S, F, site.mode, total, host != 0);
                        for (int cap : {0, 1, 7}) {
                            std::printf("layout site=%s S=%d F=%ld total=%ld cap=%d host=%d | o_mode=%zu o_off=%zu o_rows=%zu n_ints=%zu staged=%d", site.name, S,
                                        F, total, cap, host, site.mode ? bs.o_mode : 0, bs.o_off, bs.o_rows, bs.n_ints, (int)bs.staged);
                            if (site.event_ints) {
                                const SlotOut so(S, cap, site.event_ints);
                                std::printf(" o_pending=%zu o_status=%zu o_events=%zu out_ints=%zu", so.o_pending, so.o_status, so.o_events, so.n_ints);
                            }
                            std::printf("\n");
                        }
                    }
}

// rows of a tick of the prefix-sum cost: 3, and 40 at the middle tick
static int tick_rows(int k, int ticks) { return k == ticks / 2 ? 40 : 3; }

static void plans() {
    for (int ticks : {0, 1, 2, 7, 40})
        for (int tpl : {0, 1, 3, 64})
            for (int prefix = 0; prefix < 2; ++prefix) {
                const size_t unit = prefix ? 3 * 128 : 1000;                 // what an ordinary tick takes
                std::vector<size_t> off(ticks + 1, 0);
                for (int k = 0; k < ticks; ++k) off[k + 1] = off[k] + (prefix ? (size_t)tick_rows(k, ticks) * 128 : unit);
                for (size_t budget : {unit, unit - 1, unit * 5 / 2, (size_t)1 << 40})
                    for (int host = 0; host < 2; ++host) {
                        std::printf("plan ticks=%d tpl=%d prefix=%d budget=%zu frame=%zu |", ticks, tpl, prefix, budget, host ? unit : (size_t)0);
                        for (int lo = 0; lo < ticks;) {
                            const int hi = next_launch(lo, ticks, tpl, budget, host ? unit : 0, [&](int a, int b) { return off[b] - off[a]; });
                            std::printf(" %d:%d", lo, hi);
                            if (hi <= lo) return;                            // (would never end)
                            lo = hi;
                        }
                        std::printf("\n");
                    }
            }
}

static void fills() {
    const int32_t counts[6] = {2, 0, 3, 1, 0, 4};
    std::vector<int32_t> rows(10 * 6);
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = 1000 + (int)i;
    for (int mode = 0; mode < 2; ++mode)
        for (int with_counts = 0; with_counts < 2; ++with_counts)
            for (int host = 0; host < 2; ++host) {
                const long total = with_counts ? 10 : 0;
                const BankStage bs = BankStage::bank(2, 6, mode != 0, total, host != 0);
                int* h = new int[bs.n_ints];                                 // exactly the layout's size: an overrun is the sanitizer's
                for (size_t i = 0; i < bs.n_ints; ++i) h[i] = -7;
                bs.fill(h, with_counts ? counts : nullptr, rows.data());
                std::printf("fill mode=%d counts=%d host=%d n_ints=%zu |", mode, with_counts, host, bs.n_ints);
                for (size_t i = 0; i < bs.n_ints; ++i) std::printf(" %d", h[i]);
                std::printf(" | rows_of_1_3=%zu d_rows=%s\n", bs.rows_of(h, 1, 3), bs.d_rows(h, rows.data()) == h + bs.o_rows ? "staged" : "caller");
                delete[] h;
            }
    // Zones::update states its own offsets: fps[S] | fstart[S] | reset[S] | frame_off[F + 1] | frame_stream[F] | rows
    const BankStage z(2, 6, 6, 6 + 7 + 6, 10, true);
    int* h = new int[z.n_ints];
    for (size_t i = 0; i < z.n_ints; ++i) h[i] = -7;
    z.fill(h, counts, rows.data());
    std::printf("fill zones n_ints=%zu |", z.n_ints);
    for (size_t i = 0; i < z.n_ints; ++i) std::printf(" %d", h[i]);
    std::printf("\n");
    delete[] h;
}

int main() {
    layouts();
    plans();
    fills();
    return 0;
}
