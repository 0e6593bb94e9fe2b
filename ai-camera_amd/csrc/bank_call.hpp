// bank_call.hpp -- the arithmetic of a frame-bank call of the analytics stages, once: where the parts of a call's int
// staging buffer and of the slot stages' output buffer lie, how a call's ticks are cut into launches, and the constants of the slot table
// that the best-shot and the colour stage share (slot_walk.hpp).  Host arithmetic only: no HIP call, nothing but the standard library
// (tests/bank_call_probe.cpp builds it with the system compiler).  Growing the buffers, the copies and the launches are bank_stage.hpp's.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace aic {

// ---- the slot table of a stream (slot_walk.hpp): ints frame, status, 6 unused | ARRAYS arrays of 512, the first six of them these
constexpr int SLOT_TRACKS = 512;           // slots per stream = threads of the walk block
constexpr int SLOT_ST_SLOTS = 8;
enum { SLOT_A_ID = 0, SLOT_A_STATE, SLOT_A_LAST, SLOT_A_CLS, SLOT_A_FIRST, SLOT_A_SIGHT, SLOT_A_SHARED };
// state of a slot: 0 free, 1 live, 2 ENDED expired, 3 ENDED flushed; reason of an event
enum { SLOT_LIVE = 0, SLOT_EXPIRED = 1, SLOT_FLUSHED = 2 };
// what a launch without ticks does to a stream
enum { SLOT_MODE_NONE = 0, SLOT_MODE_DRAIN = 1, SLOT_MODE_FLUSH = 2 };
// the flags of a row that both stages set; a row is counted when it has all three
enum { SLOT_F_VALID = 1, SLOT_F_FIRST = 2, SLOT_F_NONEMPTY = 4 };

// ---- a stage's staging buffer, ints: reset[S] | (mode[S])? | frame_off[F + 1] | rows (host rows only: they ride behind)
// Zones::update has a prefix and a frame_stream[F] block of its own and states its offsets; the frame banks use bank().
struct BankStage {
    size_t S, F, o_mode, o_off, o_rows, n_ints;   // o_mode: only with a mode block; n_ints: the whole buffer
    bool staged;
    BankStage(int streams, long frames, size_t off, size_t rows, long total, bool host_rows)
        : S(streams), F(frames), o_mode(S), o_off(off), o_rows(rows), n_ints(rows + (host_rows ? (size_t)total * 6 : 0)), staged(host_rows) {}
    static BankStage bank(int streams, long frames, bool with_mode, long total, bool host_rows) {
        const size_t off = (with_mode ? 2 : 1) * (size_t)streams;
        return BankStage(streams, frames, off, off + frames + 1, total, host_rows);
    }
    // the blocks in front of frame_off are the caller's; counts NULL: a call without rows
    void fill(int* h, const int32_t* counts, const int32_t* rows6) const {
        h[o_off] = 0;
        for (size_t i = 0; i < F; ++i) h[o_off + i + 1] = h[o_off + i] + (counts ? counts[i] : 0);
        if (n_ints > o_rows) std::memcpy(h + o_rows, rows6, (n_ints - o_rows) * sizeof(int));
    }
    // the rows on the device: the staged copy, or the caller's pointer
    const int* d_rows(const int* d_stage, const int32_t* rows6) const { return staged ? d_stage + o_rows : rows6; }
    // rows of ticks [lo, hi), from the filled host buffer
    size_t rows_of(const int* h, int lo, int hi) const { return (size_t)(h[o_off + (size_t)hi * S] - h[o_off + (size_t)lo * S]); }
};

// ---- the slot stages' output buffer, ints: n_final[S] | pending[S] | status[S] | (16-byte aligned) events[S, cap, E]
struct SlotOut {
    size_t S, o_pending, o_status, o_events, n_ints;
    SlotOut(int streams, int cap, int event_ints)
        : S(streams), o_pending(S), o_status(2 * S), o_events((3 * S + 3) / 4 * 4), n_ints(o_events + S * cap * event_ints) {}
};

// ---- the tick chunk planner: the launch that starts at tick lo ends before the tick this returns.  One tick at the least; a launch
// grows while ticks_per_launch (0: no limit) allows and hi + 1 - lo ticks still fit the budget, in staged frames (frame_tick_bytes, 0 for
// frames in device memory) and in the stage's own per-launch buffers (launch_bytes(lo, hi) = what ticks [lo, hi) take in them).
template <class Bytes>
inline int next_launch(int lo, int ticks, int ticks_per_launch, size_t budget, size_t frame_tick_bytes, Bytes launch_bytes) {
    int hi = lo + 1;
    while (hi < ticks && (ticks_per_launch == 0 || hi - lo < ticks_per_launch) && launch_bytes(lo, hi + 1) <= budget &&
           (size_t)(hi + 1 - lo) * frame_tick_bytes <= budget)
        ++hi;
    return hi;
}

}  // namespace aic
