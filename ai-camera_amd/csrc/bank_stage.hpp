// bank_stage.hpp -- what the analytics stages share around a call on a bank of camera frames (bestshot.cpp, colours.cpp, scene.cpp,
// left.cpp; zones.cpp takes the staging layout and the C ABI shell): the argument checks of an update, the host or
// device counts, the staging upload, the launch loop, the launch options, the table-driven int options, and for the two slot stages
// reset, flush and the delivery of a call's lists.  The arithmetic is bank_call.hpp's.  A stage keeps its own checks and kernel launches.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "bank_call.hpp"
#include "row_stage.hpp"

namespace aic {

// ---- the C ABI shell: a NULL-checked handle under guarded; a destroy that lets the stage's stream run dry first
template <class H, class F>
inline int with_handle(H* h, F&& f) {
    return guarded([&] {
        AIC_REQUIRE(h, AIC_ERR_INVALID, "NULL argument");
        f();
    });
}
template <class H>
inline int destroy_handle(H* h, Device* dev) {
    return guarded([&] {
        if (h && dev) { dev->use(); (void)hipStreamSynchronize(dev->s_trk); }
        delete h;
    });
}

// ---- an int option of a stage's option struct O, by table: range, then the stage's own check on the changed copy
template <class O>
struct IntOpt {
    const char* name;
    int O::*field;
    int lo, hi;
};
template <class O, size_t N, class Check>
inline bool table_option(const IntOpt<O> (&table)[N], O& o, const std::string& k, int value, Check check) {
    for (const IntOpt<O>& t : table) {
        if (k != t.name) continue;
        AIC_REQUIRE(value >= t.lo && value <= t.hi, AIC_ERR_INVALID, k + " must be in " + std::to_string(t.lo) + ".." + std::to_string(t.hi));
        O n = o;
        n.*t.field = value;
        check(n);
        o = n;
        return true;
    }
    return false;
}

// ---- what every stage on a bank of frames holds, and the steps of its update
struct FrameBank {
    int device_id;
    Device* dev = nullptr;                       // resolved by the first call that reaches the device
    int streams;
    size_t frame_bytes;
    int ticks_per_launch = 0;                    // 0: as many ticks per launch as launch_budget_mb allows; k: at most k
    int launch_budget_mb = 1024;
    std::vector<char> reset_pending;
    DevBuf<int> d_stage;
    DevBuf<uint8_t> d_frames;
    PinBuf<int> h_stage;
    std::vector<int> h_counts;

    FrameBank(int device, int streams_, int h, int w)
        : device_id(device), streams(streams_), frame_bytes((size_t)h * w * 3), reset_pending(streams_, 1) {}

    bool launch_option(const std::string& k, int value, int ticks_max) {
        if (k == "ticks_per_launch") {
            AIC_REQUIRE(value >= 0 && value <= ticks_max, AIC_ERR_INVALID, "ticks_per_launch: 0 = as many as the budget allows, or 1..65536");
            ticks_per_launch = value;
        } else if (k == "launch_budget_mb") {
            AIC_REQUIRE(value >= 1 && value <= 65536, AIC_ERR_INVALID, "launch_budget_mb must be in 1..65536");
            launch_budget_mb = value;
        } else return false;
        return true;
    }
    // -1: every stream
    void reset_streams(int stream, const char* outside) {
        AIC_REQUIRE(stream >= -1 && stream < streams, AIC_ERR_INVALID, outside);
        for (int s = 0; s < streams; ++s)
            if (stream < 0 || stream == s) reset_pending[s] = 1;
    }
    void use_device() {
        if (!dev) dev = &device(device_id);
        dev->use();
    }
    // the shared checks of an update; returns the call's frames
    long check_call(int ticks, int ticks_max, int frames_mem, int rows_mem) const {
        AIC_REQUIRE(ticks >= 0 && ticks <= ticks_max, AIC_ERR_INVALID, "ticks must be in 0..65536");
        AIC_REQUIRE(frames_mem == AIC_HOST || frames_mem == AIC_DEVICE, AIC_ERR_INVALID, "frames_mem must be AIC_HOST or AIC_DEVICE");
        AIC_REQUIRE(rows_mem == AIC_HOST || rows_mem == AIC_DEVICE, AIC_ERR_INVALID, "rows_mem must be AIC_HOST or AIC_DEVICE");
        const long F = (long)ticks * streams;
        AIC_REQUIRE(F <= (1 << 20), AIC_ERR_INVALID, "more than 2^20 frames in one call");
        return F;
    }
    // The call's rows.  Host counts are checked before the device is touched (touch: the stage's touch_device and what it owes a call
    // that ends there); device counts are fetched behind it: they decide the launches.  check: the stage's own check of the total.
    template <class Touch, class Check>
    long count_rows(const int32_t*& counts, bool with_rows, long F, int rows_max, const int32_t* rows6, int rows_mem, Touch touch, Check check) {
        auto checked = [&](const int32_t* c) {
            const long total = check_row_counts(c, F, rows_max, rows6);
            check(total);
            return total;
        };
        long total = 0;
        if (with_rows && rows_mem == AIC_HOST) total = checked(counts);
        touch();
        if (with_rows && rows_mem == AIC_DEVICE) total = checked(counts = fetch_counts(h_counts, counts, F, dev->s_trk));
        return total;
    }
    // the staging buffer filled and on its way to the device: reset | (mode(s) when the stage has modes) | frame_off | host rows
    template <class Mode>
    BankStage upload(bool with_mode, Mode mode, long F, const int32_t* counts, long total, const int32_t* rows6, bool host_rows, const char* what) {
        const BankStage bs = BankStage::bank(streams, F, with_mode, total, host_rows);
        h_stage.ensure(bs.n_ints);
        grow(d_stage, bs.n_ints, what);
        int* h = h_stage.p;
        for (int s = 0; s < streams; ++s) {
            h[s] = reset_pending[s];
            if (with_mode) h[bs.o_mode + s] = mode(s);
        }
        bs.fill(h, counts, rows6);
        HIP_CHECK(hipMemcpyAsync(d_stage.p, h, bs.n_ints * sizeof(int), hipMemcpyHostToDevice, dev->s_trk));
        return bs;
    }
    BankStage upload(long F, const int32_t* counts, long total, const int32_t* rows6, bool host_rows) {
        return upload(false, [](int) { return 0; }, F, counts, total, rows6, host_rows, "the staged rows");
    }
    // the most rows of a frame of ticks [lo, hi): the row grids of a launch
    int max_rows(const int32_t* counts, int lo, int hi) const {
        int m = 0;
        for (long f = (long)lo * streams; f < (long)hi * streams; ++f) m = std::max(m, (int)counts[f]);
        return m;
    }
    // The launch loop: cuts the ticks (bank_call.hpp's planner; launch_bytes(lo, hi) = what ticks [lo, hi) take in the stage's per-launch
    // buffers), stages host frames, and hands body(lo, hi, the launch's frames on the device).
    template <class Bytes, class Body>
    void launches(const void* frames, int frames_mem, int ticks, Bytes launch_bytes, Body body) {
        const size_t budget = (size_t)launch_budget_mb << 20, tick_bytes = frame_bytes * streams;
        for (int lo = 0; lo < ticks;) {
            const int hi = next_launch(lo, ticks, ticks_per_launch, budget, frames_mem == AIC_HOST ? tick_bytes : 0, launch_bytes);
            const uint8_t* d_fr = static_cast<const uint8_t*>(frames) + (size_t)lo * tick_bytes;
            if (frames_mem == AIC_HOST) {
                grow(d_frames, (size_t)(hi - lo) * tick_bytes, "the staged frames");
                HIP_CHECK(hipMemcpyAsync(d_frames.p, d_fr, (size_t)(hi - lo) * tick_bytes, hipMemcpyHostToDevice, dev->s_trk));
                d_fr = d_frames.p;
            }
            body(lo, hi, d_fr);
            lo = hi;
        }
    }
};

// ---- the two stages on a slot table (slot_walk.hpp): streams stop, calls deliver lists of ENDED tracks
struct SlotBank : FrameBank {
    std::vector<int> stop;                       // 0 or the code a stream stopped with
    DevBuf<int> d_out;
    PinBuf<int> h_out;

    SlotBank(int device, int streams_, int h, int w) : FrameBank(device, streams_, h, w), stop(streams_, 0) {}

    void reset_stream(int stream, const char* outside) {
        AIC_REQUIRE(stream >= 0 && stream < streams, AIC_ERR_INVALID, outside);
        stop[stream] = 0;
        reset_pending[stream] = 1;
    }
    // an update drains every stream
    BankStage upload_update(long F, const int32_t* counts, long total, const int32_t* rows6, bool host_rows) {
        return upload(true, [](int) { return (int)SLOT_MODE_DRAIN; }, F, counts, total, rows6, host_rows, "the staged rows");
    }
    // a flush ends the live tracks of one stream, or of every stream (-1)
    BankStage upload_flush(int stream) {
        return upload(true, [&](int s) { return (int)(stream < 0 || stream == s ? SLOT_MODE_FLUSH : SLOT_MODE_NONE); }, 0, nullptr, 0, nullptr, false,
                      "the staging buffer");
    }
    SlotOut out(int cap, int event_ints) {
        const SlotOut so(streams, cap, event_ints);
        grow(d_out, so.n_ints, "the events");
        return so;
    }
    // The call's lists come back: counts first, then only the filled entries.  extra(s, n): the stage's own copy of stream s's n entries.
    template <class Extra>
    void finish(int cap, int event_ints, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status, Extra extra) {
        const size_t S = streams, o_ev = SlotOut(streams, cap, event_ints).o_events;
        hipStream_t st = dev->s_trk;
        h_out.ensure(3 * S);
        HIP_CHECK(hipMemcpyAsync(h_out.p, d_out.p, 3 * S * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::fill(reset_pending.begin(), reset_pending.end(), (char)0);
        const int* o = h_out.p;
        bool any = false;
        for (size_t s = 0; s < S; ++s) {
            const int n = std::min(std::max(o[s], 0), cap);
            n_final[s] = n, pending[s] = o[S + s], stop[s] = o[2 * S + s];
            if (status) status[s] = stop[s];
            if (!n) continue;
            any = true;
            HIP_CHECK(hipMemcpyAsync(events + s * cap * event_ints, d_out.p + o_ev + s * cap * event_ints, (size_t)n * event_ints * sizeof(int),
                                     hipMemcpyDeviceToHost, st));
            extra((int)s, n);
        }
        if (any) HIP_CHECK(hipStreamSynchronize(st));
    }
};

}  // namespace aic
