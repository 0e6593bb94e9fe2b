// colours.cpp -- the clothing-colour object (colours.hpp) and its C ABI.  Every argument is checked before the device is touched; the
// arithmetic runs in kernels_colours.hip or the call raises.  aic_colours_classify is the host's copy of the pixel rule.
#include "colours.hpp"

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
    : SlotBank(device, p.streams, p.frame_h, p.frame_w),
      g{p.streams, p.frame_h, p.frame_w, p.max_tracks, p.forget_after, p.torso0, p.torso1, p.legs0, p.legs1, p.inset_q8, p.min_w, p.min_h,
        p.max_cover_q8} {}

void Colours::touch_device() {
    use_device();
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

void Colours::walk(const int* d_off, int n_ticks, const int* d_rows, int info_base, const BankStage& bs, int first, int cap, const SlotOut& so,
                   int* d_rt) {
    int* o = d_out.p;
    launch_colours_walk(d_off, n_ticks, d_rows, d_info.p, info_base, d_stage.p, d_stage.p + bs.o_mode, first, g, d_state.p, cap, o,
                        o + so.o_pending, o + so.o_status, o + so.o_events, d_rt, dev->s_trk);
}

void Colours::update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap,
                     int32_t* n_final, int32_t* events, int32_t* row_tags, int32_t* pending, int32_t* status) {
    const int S = g.streams;
    const long F = check_call(ticks, CL_TICKS_MAX, frames_mem, rows_mem);
    check_outputs(cap, n_final, events, pending);
    AIC_REQUIRE(F == 0 || (frames && counts), AIC_ERR_INVALID, "NULL frames or counts");
    const long total = count_rows(counts, F > 0, F, CL_ROWS_MAX, rows6, rows_mem, [&] { touch_device(); }, [](long t) {
        AIC_REQUIRE(t <= (1 << 24), AIC_ERR_INVALID, "more than 2^24 rows in one call");
    });
    hipStream_t st = dev->s_trk;
    const BankStage bs = upload_update(F, counts, total, rows6, rows_mem == AIC_HOST);
    const int* d_rows = bs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + bs.o_off;
    const SlotOut so = out(cap, CL_EVENT_INTS);
    int* d_rt = nullptr;
    if (row_tags && total) {
        grow(d_tags, (size_t)total * 4, "the row tags");
        d_rt = d_tags.p;
    }
    {
        const size_t info_bytes = CL_INFO_INTS * sizeof(int);
        Prof pr(*dev, PROF_TRK, st, 0, (double)total * info_bytes);
        if (ticks == 0) walk(d_off, 0, d_rows, 0, bs, 1, cap, so, nullptr);
        launches(frames, frames_mem, ticks, [&](int lo, int hi) { return bs.rows_of(h_stage.p, lo, hi) * info_bytes; },
                 [&](int lo, int hi, const uint8_t* d_fr) {
                     const int base = h_stage.p[bs.o_off + (size_t)lo * S];
                     grow(d_info, std::max<size_t>(CL_INFO_INTS, bs.rows_of(h_stage.p, lo, hi) * CL_INFO_INTS), "the sampled rows");
                     launch_colours_sample(d_fr, d_off + (size_t)lo * S, (hi - lo) * S, max_rows(counts, lo, hi), d_rows, d_state.p, d_stage.p, lo == 0, g,
                                           base, d_info.p, st);
                     walk(d_off + (size_t)lo * S, hi - lo, d_rows, base, bs, lo == 0, cap, so, d_rt);
                 });
    }
    if (d_rt) HIP_CHECK(hipMemcpyAsync(row_tags, d_rt, (size_t)total * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    finish(cap, CL_EVENT_INTS, n_final, events, pending, status, [](int, int) {});
}

void Colours::flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    AIC_REQUIRE(stream >= -1 && stream < g.streams, AIC_ERR_INVALID, "stream outside the colour bank (-1 = every stream)");
    check_outputs(cap, n_final, events, pending);
    touch_device();
    const BankStage bs = upload_flush(stream);
    walk(d_stage.p + bs.o_off, 0, nullptr, 0, bs, 1, cap, out(cap, CL_EVENT_INTS), nullptr);
    finish(cap, CL_EVENT_INTS, n_final, events, pending, status, [](int, int) {});
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

int aic_colours_destroy(aic_colours* c) { return destroy_handle(c, c ? c->c.dev : nullptr); }

int aic_colours_option(aic_colours* c, const char* key, int value) {
    return with_handle(c, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        AIC_REQUIRE(c->c.launch_option(k, value, CL_TICKS_MAX), AIC_ERR_INVALID, "unknown colours option: " + k);
    });
}

int aic_colours_reset(aic_colours* c, int stream) {
    return with_handle(c, [&] { c->c.reset(stream); });
}

int aic_colours_update(aic_colours* c, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                       int rows_mem, int cap, int32_t* n_final, int32_t* events, int32_t* row_tags, int32_t* pending, int32_t* status) {
    return with_handle(c, [&] { c->c.update(frames_bgr, frames_mem, ticks, counts, rows6, rows_mem, cap, n_final, events, row_tags, pending, status); });
}

int aic_colours_flush(aic_colours* c, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    return with_handle(c, [&] { c->c.flush(stream, cap, n_final, events, pending, status); });
}

int aic_colours_export(aic_colours* c, int stream, int32_t* n, int32_t* events) {
    return with_handle(c, [&] { c->c.export_stream(stream, n, events); });
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
