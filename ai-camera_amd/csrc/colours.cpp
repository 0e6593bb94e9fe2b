// colours.cpp -- the clothing-colour object (colours.hpp) and its C ABI.  Every argument is checked before the device is touched; the
// arithmetic runs in kernels_colours.hip or the call raises.  aic_colours_classify is the host's copy of the pixel rule.
#include "colours.hpp"
#include "row_stage.hpp"

#include <algorithm>

namespace aic {

void colours_check_params(int device, const aic_colours_config* p) {
    AIC_REQUIRE(p, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(p->streams >= 1 && p->streams <= CL_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p->frame_h >= 1 && p->frame_h <= CL_DIM_MAX && p->frame_w >= 1 && p->frame_w <= CL_DIM_MAX, AIC_ERR_INVALID,
                "frame height and width must be in 1..16384");
    AIC_REQUIRE(p->max_tracks >= 1 && p->max_tracks <= CL_TRACKS_MAX, AIC_ERR_INVALID, "max_tracks must be in 1..512");
    AIC_REQUIRE(p->forget_after >= 0 && p->forget_after <= (1 << 24), AIC_ERR_INVALID, "forget_after must be in 0..2^24");
    AIC_REQUIRE(0 <= p->torso0 && p->torso0 < p->torso1 && p->torso1 <= 256, AIC_ERR_INVALID, "torso_q8 must be 0 <= a < b <= 256");
    AIC_REQUIRE(0 <= p->legs0 && p->legs0 < p->legs1 && p->legs1 <= 256, AIC_ERR_INVALID, "legs_q8 must be 0 <= a < b <= 256");
    AIC_REQUIRE(p->inset_q8 >= 0 && p->inset_q8 < 128, AIC_ERR_INVALID, "inset_q8 must be in 0..127");
    AIC_REQUIRE(p->min_w >= 1 && p->min_w <= CL_DIM_MAX && p->min_h >= 1 && p->min_h <= CL_DIM_MAX, AIC_ERR_INVALID,
                "min_w and min_h must be in 1..16384");
    AIC_REQUIRE(p->max_cover_q8 >= 0 && p->max_cover_q8 <= 256, AIC_ERR_INVALID, "max_cover_q8 must be in 0..256");
}

Colours::Colours(int device, const aic_colours_config& p)
    : device_id(device), g{p.streams, p.frame_h, p.frame_w, p.max_tracks, p.forget_after, p.torso0, p.torso1, p.legs0, p.legs1, p.inset_q8, p.min_w,
                           p.min_h, p.max_cover_q8},
      reset_pending(p.streams, 1), stop(p.streams, 0) {}

void Colours::reset(int stream) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the colour bank");
    stop[stream] = 0;
    reset_pending[stream] = 1;
}

void Colours::touch_device() {
    if (!dev) dev = &device(device_id);
    dev->use();
    if (!d_state.p) {
        grow(d_state, (size_t)g.streams * CL_ST_INTS, "the slot tables");
        HIP_CHECK(hipMemsetAsync(d_state.p, 0, d_state.bytes(), dev->s_trk));
    }
}

static void check_outputs(int cap, const int32_t* n_final, const int32_t* events, const int32_t* pending) {
    AIC_REQUIRE(cap >= 0 && cap <= CL_CAP_MAX, AIC_ERR_INVALID, "cap must be in 0..4096");
    AIC_REQUIRE(n_final && pending, AIC_ERR_INVALID, "NULL n_final or pending");
    AIC_REQUIRE(cap == 0 || events, AIC_ERR_INVALID, "NULL events");
}

// outputs of a call, ints: n_final[S] | pending[S] | status[S] | (16-byte aligned) events[S, cap, 48]
static size_t out_events_at(int S) { return ((size_t)3 * S + 3) / 4 * 4; }

void Colours::update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap,
                     int32_t* n_final, int32_t* events, int32_t* row_tags, int32_t* pending, int32_t* status) {
    const int S = g.streams;
    AIC_REQUIRE(ticks >= 0 && ticks <= CL_TICKS_MAX, AIC_ERR_INVALID, "ticks must be in 0..65536");
    AIC_REQUIRE(frames_mem == AIC_HOST || frames_mem == AIC_DEVICE, AIC_ERR_INVALID, "frames_mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(rows_mem == AIC_HOST || rows_mem == AIC_DEVICE, AIC_ERR_INVALID, "rows_mem must be AIC_HOST or AIC_DEVICE");
    check_outputs(cap, n_final, events, pending);
    const long F = (long)ticks * S;
    AIC_REQUIRE(F <= (1 << 20), AIC_ERR_INVALID, "more than 2^20 frames in one call");
    AIC_REQUIRE(F == 0 || (frames && counts), AIC_ERR_INVALID, "NULL frames or counts");
    auto check_counts = [&](const int32_t* c) {
        const long total = check_row_counts(c, F, CL_ROWS_MAX, rows6);
        AIC_REQUIRE(total <= (1 << 24), AIC_ERR_INVALID, "more than 2^24 rows in one call");
        return total;
    };
    long total = 0;
    if (rows_mem == AIC_HOST && F) total = check_counts(counts);

    touch_device();
    hipStream_t st = dev->s_trk;
    if (rows_mem == AIC_DEVICE && F) total = check_counts(counts = fetch_counts(h_counts, counts, F, st));   // the counts decide the launches
    // ---- staging: reset[S] | mode[S] | frame_off[F + 1] | rows (host memory only; row_stage.hpp)
    const size_t o_mode = S, o_off = 2 * (size_t)S;
    const RowStage rs(o_off, o_off + F + 1, total, rows_mem == AIC_HOST);
    h_stage.ensure(rs.n_ints);
    grow(d_stage, rs.n_ints, "the staged rows");
    int* h = h_stage.p;
    for (int s = 0; s < S; ++s) h[s] = reset_pending[s], h[o_mode + s] = CL_MODE_DRAIN;
    rs.fill(h, counts, F, rows6);
    HIP_CHECK(hipMemcpyAsync(d_stage.p, h, rs.n_ints * sizeof(int), hipMemcpyHostToDevice, st));
    const int* d_rows = rs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + o_off;
    const size_t o_ev = out_events_at(S);
    grow(d_out, o_ev + (size_t)S * cap * CL_EVENT_INTS, "the events");
    int* d_rt = nullptr;
    if (row_tags && total) {
        grow(d_tags, (size_t)total * 4, "the row tags");
        d_rt = d_tags.p;
    }
    int* o = d_out.p;

    {
        Prof pr(*dev, PROF_TRK, st, 0, (double)total * CL_INFO_INTS * sizeof(int));
        if (ticks == 0)
            launch_colours_walk(d_off, 0, d_rows, nullptr, 0, d_stage.p, d_stage.p + o_mode, 1, g, d_state.p, cap, o, o + S, o + 2 * S, o + o_ev, nullptr,
                                st);
        const size_t budget = (size_t)launch_budget_mb << 20, frame_bytes = (size_t)g.h * g.w * 3, tick_bytes = frame_bytes * S;
        const size_t info_bytes = CL_INFO_INTS * sizeof(int);
        for (int lo = 0; lo < ticks;) {
            int hi = lo + 1;                                                 // one tick at the least
            while (hi < ticks && (ticks_per_launch == 0 || hi - lo < ticks_per_launch) &&
                   (size_t)(h[o_off + (size_t)(hi + 1) * S] - h[o_off + (size_t)lo * S]) * info_bytes <= budget &&
                   (frames_mem == AIC_DEVICE || (size_t)(hi + 1 - lo) * tick_bytes <= budget))
                ++hi;
            const int base = h[o_off + (size_t)lo * S], rows = h[o_off + (size_t)hi * S] - base;
            int max_rows = 0;
            for (long f = (long)lo * S; f < (long)hi * S; ++f) max_rows = std::max(max_rows, (int)counts[f]);
            const uint8_t* d_fr = static_cast<const uint8_t*>(frames) + (size_t)lo * tick_bytes;
            if (frames_mem == AIC_HOST) {
                grow(d_frames, (size_t)(hi - lo) * tick_bytes, "the staged frames");
                HIP_CHECK(hipMemcpyAsync(d_frames.p, d_fr, (size_t)(hi - lo) * tick_bytes, hipMemcpyHostToDevice, st));
                d_fr = d_frames.p;
            }
            grow(d_info, std::max<size_t>(CL_INFO_INTS, (size_t)rows * CL_INFO_INTS), "the sampled rows");
            launch_colours_sample(d_fr, d_off + (size_t)lo * S, (hi - lo) * S, max_rows, d_rows, d_state.p, d_stage.p, lo == 0, g, base, d_info.p, st);
            launch_colours_walk(d_off + (size_t)lo * S, hi - lo, d_rows, d_info.p, base, d_stage.p, d_stage.p + o_mode, lo == 0, g, d_state.p, cap, o, o + S,
                                o + 2 * S, o + o_ev, d_rt, st);
            lo = hi;
        }
    }
    if (d_rt) HIP_CHECK(hipMemcpyAsync(row_tags, d_rt, (size_t)total * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    finish(cap, n_final, events, pending, status);
}

void Colours::flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    const int S = g.streams;
    AIC_REQUIRE(stream >= -1 && stream < S, AIC_ERR_INVALID, "stream outside the colour bank (-1 = every stream)");
    check_outputs(cap, n_final, events, pending);
    touch_device();
    hipStream_t st = dev->s_trk;
    h_stage.ensure(2 * (size_t)S + 1);
    grow(d_stage, 2 * (size_t)S + 1, "the staging buffer");
    int* h = h_stage.p;
    for (int s = 0; s < S; ++s) h[s] = reset_pending[s], h[S + s] = stream < 0 || stream == s ? CL_MODE_FLUSH : CL_MODE_NONE;
    h[2 * S] = 0;
    HIP_CHECK(hipMemcpyAsync(d_stage.p, h, (2 * (size_t)S + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    const size_t o_ev = out_events_at(S);
    grow(d_out, o_ev + (size_t)S * cap * CL_EVENT_INTS, "the events");
    int* o = d_out.p;
    launch_colours_walk(d_stage.p + 2 * S, 0, nullptr, nullptr, 0, d_stage.p, d_stage.p + S, 1, g, d_state.p, cap, o, o + S, o + 2 * S, o + o_ev, nullptr, st);
    finish(cap, n_final, events, pending, status);
}

void Colours::finish(int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    const int S = g.streams;
    hipStream_t st = dev->s_trk;
    const size_t o_ev = out_events_at(S);
    h_out.ensure(3 * (size_t)S);
    HIP_CHECK(hipMemcpyAsync(h_out.p, d_out.p, 3 * (size_t)S * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::fill(reset_pending.begin(), reset_pending.end(), (char)0);
    const int* o = h_out.p;
    bool any = false;
    for (int s = 0; s < S; ++s) {                                            // only the filled entries come back
        const int n = std::min(std::max(o[s], 0), cap);
        n_final[s] = n, pending[s] = o[S + s], stop[s] = o[2 * S + s];
        if (status) status[s] = stop[s];
        if (!n) continue;
        any = true;
        HIP_CHECK(hipMemcpyAsync(events + (size_t)s * cap * CL_EVENT_INTS, d_out.p + o_ev + (size_t)s * cap * CL_EVENT_INTS,
                                 (size_t)n * CL_EVENT_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (any) HIP_CHECK(hipStreamSynchronize(st));
}

void Colours::export_stream(int stream, int32_t* n, int32_t* events) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the colour bank");
    AIC_REQUIRE(n && events, AIC_ERR_INVALID, "NULL argument");
    *n = 0;
    if (!d_state.p || reset_pending[stream]) return;                         // nothing seen yet, or a reset the next call applies
    dev->use();
    hipStream_t st = dev->s_trk;
    h_state.resize(CL_ST_INTS);
    HIP_CHECK(hipMemcpyAsync(h_state.data(), d_state.p + (size_t)stream * CL_ST_INTS, CL_ST_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int* a = h_state.data() + CL_ST_SLOTS;
    auto at = [&](int arr, int t) { return a[arr * CL_TRACKS_MAX + t]; };
    int k = 0;
    for (int t = 0; t < g.max_tracks; ++t) {
        const int state = at(CL_A_STATE, t);
        if (!state) continue;
        int32_t* ev = events + (size_t)k * CL_EVENT_INTS;
        std::fill(ev, ev + CL_EVENT_INTS, 0);
        const int* acc = h_state.data() + CL_ST_ACC + t * 2 * CL_BINS;
        const int nu = at(CL_A_NU, t), nl = at(CL_A_NL, t);
        int tu, su, tl, sl;
        cl_describe(acc, nu, &tu, &su, ev + 16);
        cl_describe(acc + CL_BINS, nl, &tl, &sl, ev + 28);
        const int32_t head[14] = {state == 1 ? CL_LIVE : state == 3 ? CL_FLUSHED : CL_EXPIRED, stream, at(CL_A_ID, t), at(CL_A_CLS, t), at(CL_A_FIRST, t),
                                  at(CL_A_LAST, t), at(CL_A_SIGHT, t), nu, nl, tu, su, tl, sl, t};
        std::copy(head, head + 14, ev);
        ++k;
    }
    *n = k;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_colours_config_default(int streams, int frame_h, int frame_w, aic_colours_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_colours_config{streams, frame_h, frame_w, 128, 70, 51, 128, 141, 230, 64, 4, 4, 64};
    });
}

int aic_colours_create(int device, const aic_colours_config* config, aic_colours** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        colours_check_params(device, config);
        *out = new aic_colours(device, *config);
    });
}

int aic_colours_destroy(aic_colours* c) {
    return guarded([&] {
        if (c && c->c.dev) { c->c.dev->use(); (void)hipStreamSynchronize(c->c.dev->s_trk); }
        delete c;
    });
}

int aic_colours_option(aic_colours* c, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(c && key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        if (k == "ticks_per_launch") {
            AIC_REQUIRE(value >= 0 && value <= CL_TICKS_MAX, AIC_ERR_INVALID, "ticks_per_launch: 0 = as many as the budget allows, or 1..65536");
            c->c.ticks_per_launch = value;
        } else if (k == "launch_budget_mb") {
            AIC_REQUIRE(value >= 1 && value <= 65536, AIC_ERR_INVALID, "launch_budget_mb must be in 1..65536");
            c->c.launch_budget_mb = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown colours option: " + k);
    });
}

int aic_colours_reset(aic_colours* c, int stream) {
    return guarded([&] {
        AIC_REQUIRE(c, AIC_ERR_INVALID, "NULL argument");
        c->c.reset(stream);
    });
}

int aic_colours_update(aic_colours* c, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                       int rows_mem, int cap, int32_t* n_final, int32_t* events, int32_t* row_tags, int32_t* pending, int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(c, AIC_ERR_INVALID, "NULL argument");
        c->c.update(frames_bgr, frames_mem, ticks, counts, rows6, rows_mem, cap, n_final, events, row_tags, pending, status);
    });
}

int aic_colours_flush(aic_colours* c, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(c, AIC_ERR_INVALID, "NULL argument");
        c->c.flush(stream, cap, n_final, events, pending, status);
    });
}

int aic_colours_export(aic_colours* c, int stream, int32_t* n, int32_t* events) {
    return guarded([&] {
        AIC_REQUIRE(c, AIC_ERR_INVALID, "NULL argument");
        c->c.export_stream(stream, n, events);
    });
}

int aic_colours_classify(const uint8_t* bgr, int n, uint8_t* bins) {
    return guarded([&] {
        AIC_REQUIRE(n >= 0, AIC_ERR_INVALID, "a negative pixel count");
        AIC_REQUIRE(n == 0 || (bgr && bins), AIC_ERR_INVALID, "NULL argument");
        unsigned recip[256];
        for (unsigned d = 0; d < 256; ++d) recip[d] = cl_recip(d);
        for (int i = 0; i < n; ++i) bins[i] = (uint8_t)cl_classify(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], recip);
    });
}

}  // extern "C"
