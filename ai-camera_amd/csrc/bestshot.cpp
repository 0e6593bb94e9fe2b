// bestshot.cpp -- the best-shot object (bestshot.hpp) and its C ABI.  Every argument is checked before the device is touched; the
// arithmetic runs in kernels_bestshot.hip or the call raises.
#include "bestshot.hpp"

#include <algorithm>

namespace aic {

void bestshot_check_params(int device, const aic_bestshot_config* p) {
    AIC_REQUIRE(p, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(p->streams >= 1 && p->streams <= BS_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p->frame_h >= 1 && p->frame_h <= BS_DIM_MAX && p->frame_w >= 1 && p->frame_w <= BS_DIM_MAX, AIC_ERR_INVALID,
                "frame height and width must be in 1..16384");
    AIC_REQUIRE(p->thumb_w >= 16 && p->thumb_w <= 128 && p->thumb_w % 8 == 0, AIC_ERR_INVALID, "thumb_w must be a multiple of 8 in 16..128");
    AIC_REQUIRE(p->thumb_h >= 16 && p->thumb_h <= 256 && p->thumb_h % 8 == 0, AIC_ERR_INVALID, "thumb_h must be a multiple of 8 in 16..256");
    AIC_REQUIRE(p->max_tracks >= 1 && p->max_tracks <= BS_TRACKS_MAX, AIC_ERR_INVALID, "max_tracks must be in 1..512");
    AIC_REQUIRE(p->forget_after >= 0 && p->forget_after <= (1 << 24), AIC_ERR_INVALID, "forget_after must be in 0..2^24");
    AIC_REQUIRE(p->region == BS_REGION_BOX || p->region == BS_REGION_HEAD, AIC_ERR_INVALID, "region must be 0 (box) or 1 (head)");
    AIC_REQUIRE(p->head_q8 >= 1 && p->head_q8 <= 256, AIC_ERR_INVALID, "head_q8 must be in 1..256");
    AIC_REQUIRE(p->pad >= 0 && p->pad <= 64, AIC_ERR_INVALID, "pad must be in 0..64");
    AIC_REQUIRE(p->min_w >= 1 && p->min_w <= BS_DIM_MAX && p->min_h >= 1 && p->min_h <= BS_DIM_MAX, AIC_ERR_INVALID,
                "min_w and min_h must be in 1..16384");
}

BestShot::BestShot(int device, const aic_bestshot_config& p)
    : SlotBank(device, p.streams, p.frame_h, p.frame_w),
      g{p.streams, p.frame_h, p.frame_w, p.thumb_w, p.thumb_h, p.max_tracks, p.forget_after, p.region, p.head_q8, p.pad, p.min_w, p.min_h} {}

void BestShot::touch_device() {
    use_device();
    if (!d_state.p) {
        grow(d_slot_thumbs, (size_t)g.streams * g.max_tracks * thumb_bytes(), "the resident slot thumbnails");
        grow(d_state, (size_t)g.streams * BS_ST_INTS, "the slot tables");
        HIP_CHECK(hipMemsetAsync(d_state.p, 0, d_state.bytes(), dev->s_trk));
    }
}

static void check_outputs(int cap, const int32_t* n_final, const int32_t* events, const uint8_t* thumbs, const int32_t* pending) {
    AIC_REQUIRE(cap >= 0 && cap <= BS_CAP_MAX, AIC_ERR_INVALID, "cap must be in 0..4096");
    AIC_REQUIRE(n_final && pending, AIC_ERR_INVALID, "NULL n_final or pending");
    AIC_REQUIRE(cap == 0 || (events && thumbs), AIC_ERR_INVALID, "NULL events or thumbs");
}

SlotOut BestShot::outputs(int cap) {
    const SlotOut so = out(cap, BS_EVENT_INTS);
    grow(d_out_thumbs, std::max<size_t>(16, (size_t)g.streams * cap * thumb_bytes()), "the output thumbnails");
    return so;
}

void BestShot::walk(const int* d_off, int n_ticks, const int* d_rows, int cand_base, const BankStage& bs, int first, int cap, const SlotOut& so) {
    int* o = d_out.p;
    launch_bestshot_walk(d_off, n_ticks, d_rows, d_info.p, d_cand.p, cand_base, d_stage.p, d_stage.p + bs.o_mode, first, g, d_state.p, d_slot_thumbs.p,
                         cap, o, o + so.o_pending, o + so.o_status, o + so.o_events, d_out_thumbs.p, dev->s_trk);
}

void BestShot::update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap,
                      int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status) {
    const int S = g.streams;
    const long F = check_call(ticks, BS_TICKS_MAX, frames_mem, rows_mem);
    check_outputs(cap, n_final, events, thumbs, pending);
    AIC_REQUIRE(F == 0 || (frames && counts), AIC_ERR_INVALID, "NULL frames or counts");
    const long total = count_rows(counts, F > 0, F, BS_ROWS_MAX, rows6, rows_mem, [&] { touch_device(); }, [](long t) {
        AIC_REQUIRE(t <= (1 << 24), AIC_ERR_INVALID, "more than 2^24 rows in one call");
    });
    hipStream_t st = dev->s_trk;
    const BankStage bs = upload_update(F, counts, total, rows6, rows_mem == AIC_HOST);
    const int* d_rows = bs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + bs.o_off;
    grow(d_info, std::max<size_t>(8, (size_t)total * 8), "the scored rows");
    const SlotOut so = outputs(cap);
    {
        Prof pr(*dev, PROF_TRK, st, 0, (double)total * thumb_bytes());
        if (ticks == 0) walk(d_off, 0, d_rows, 0, bs, 1, cap, so);
        launches(frames, frames_mem, ticks, [&](int lo, int hi) { return bs.rows_of(h_stage.p, lo, hi) * thumb_bytes(); },
                 [&](int lo, int hi, const uint8_t* d_fr) {
                     const int base = h_stage.p[bs.o_off + (size_t)lo * S];
                     grow(d_cand, std::max<size_t>(16, bs.rows_of(h_stage.p, lo, hi) * thumb_bytes()), "the candidate thumbnails");
                     launch_bestshot_score(d_fr, d_off + (size_t)lo * S, (hi - lo) * S, max_rows(counts, lo, hi), d_rows, d_state.p, d_stage.p, lo == 0, g,
                                           base, d_info.p, d_cand.p, st);
                     walk(d_off + (size_t)lo * S, hi - lo, d_rows, base, bs, lo == 0, cap, so);
                 });
    }
    if (stats && total) {
        h_info.resize((size_t)total * 8);
        HIP_CHECK(hipMemcpyAsync(h_info.data(), d_info.p, (size_t)total * 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    finish(cap, n_final, events, thumbs, pending, status);
    if (stats && total) {
        HIP_CHECK(hipStreamSynchronize(st));
        n_rows += total;
        for (long i = 0; i < total; ++i) n_candidates += (h_info[i * 8] & BS_F_CAND) != 0, n_stored += (h_info[i * 8] & BS_F_STORED) != 0;
    }
}

void BestShot::flush(int stream, int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status) {
    AIC_REQUIRE(stream >= -1 && stream < g.streams, AIC_ERR_INVALID, "stream outside the best-shot bank (-1 = every stream)");
    check_outputs(cap, n_final, events, thumbs, pending);
    touch_device();
    const BankStage bs = upload_flush(stream);
    walk(d_stage.p + bs.o_off, 0, nullptr, 0, bs, 1, cap, outputs(cap));
    finish(cap, n_final, events, thumbs, pending, status);
}

void BestShot::finish(int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status) {
    SlotBank::finish(cap, BS_EVENT_INTS, n_final, events, pending, status, [&](int s, int n) {
        HIP_CHECK(hipMemcpyAsync(thumbs + (size_t)s * cap * thumb_bytes(), d_out_thumbs.p + (size_t)s * cap * thumb_bytes(), (size_t)n * thumb_bytes(),
                                 hipMemcpyDeviceToHost, dev->s_trk));
    });
}

void BestShot::export_stream(int stream, int32_t* n, int32_t* events, uint8_t* thumbs) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the best-shot bank");
    AIC_REQUIRE(n && events && thumbs, AIC_ERR_INVALID, "NULL argument");
    *n = 0;
    if (!d_state.p || reset_pending[stream]) return;                         // nothing seen yet, or a reset the next call applies
    dev->use();
    hipStream_t st = dev->s_trk;
    h_state.resize(BS_ST_INTS);
    HIP_CHECK(hipMemcpyAsync(h_state.data(), d_state.p + (size_t)stream * BS_ST_INTS, BS_ST_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int* a = h_state.data() + BS_ST_SLOTS;
    auto at = [&](int arr, int t) { return a[arr * BS_TRACKS_MAX + t]; };
    int k = 0;
    for (int t = 0; t < g.max_tracks; ++t) {
        const int state = at(BS_A_STATE, t);
        if (!state) continue;
        const int has = at(BS_A_HAS, t);
        int32_t* ev = events + (size_t)k * BS_EVENT_INTS;
        const int32_t row[BS_EVENT_INTS] = {state == 1 ? BS_LIVE : state == 3 ? BS_FLUSHED : BS_EXPIRED, stream, at(BS_A_ID, t), at(BS_A_CLS, t),
                                            at(BS_A_FIRST, t), at(BS_A_LAST, t), at(BS_A_SIGHT, t), has, has ? at(BS_A_BFRAME, t) : 0,
                                            has ? at(BS_A_SCORE, t) : 0, has ? at(BS_A_C0, t) : 0, has ? at(BS_A_C1, t) : 0, has ? at(BS_A_C2, t) : 0,
                                            has ? at(BS_A_C3, t) : 0, t, 0};
        std::copy(row, row + BS_EVENT_INTS, ev);
        uint8_t* th = thumbs + (size_t)k * thumb_bytes();
        if (has)
            HIP_CHECK(hipMemcpyAsync(th, d_slot_thumbs.p + ((size_t)stream * g.max_tracks + t) * thumb_bytes(), thumb_bytes(), hipMemcpyDeviceToHost, st));
        else std::memset(th, 0, thumb_bytes());
        ++k;
    }
    HIP_CHECK(hipStreamSynchronize(st));
    *n = k;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_bestshot_params(int streams, int frame_h, int frame_w, aic_bestshot_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_bestshot_config{streams, frame_h, frame_w, 64, 128, 128, 70, BS_REGION_BOX, 64, 0, 8, 16};
    });
}

int aic_bestshot_create(int device, const aic_bestshot_config* params, aic_bestshot** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        bestshot_check_params(device, params);
        *out = new aic_bestshot(device, *params);
    });
}

int aic_bestshot_destroy(aic_bestshot* b) { return destroy_handle(b, b ? b->b.dev : nullptr); }

int aic_bestshot_option(aic_bestshot* b, const char* key, int value) {
    return with_handle(b, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        if (b->b.launch_option(k, value, BS_TICKS_MAX)) return;
        AIC_REQUIRE(k == "stats", AIC_ERR_INVALID, "unknown best-shot option: " + k);
        AIC_REQUIRE(value == 0 || value == 1, AIC_ERR_INVALID, "stats must be 0 or 1");
        b->b.stats = value;
    });
}

int aic_bestshot_reset(aic_bestshot* b, int stream) {
    return with_handle(b, [&] { b->b.reset(stream); });
}

int aic_bestshot_update(aic_bestshot* b, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                        int rows_mem, int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status) {
    return with_handle(b, [&] { b->b.update(frames_bgr, frames_mem, ticks, counts, rows6, rows_mem, cap, n_final, events, thumbs, pending, status); });
}

int aic_bestshot_flush(aic_bestshot* b, int stream, int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending,
                       int32_t* status) {
    return with_handle(b, [&] { b->b.flush(stream, cap, n_final, events, thumbs, pending, status); });
}

int aic_bestshot_counters(aic_bestshot* b, int64_t* rows, int64_t* candidates, int64_t* stored) {
    return with_handle(b, [&] {
        if (rows) *rows = b->b.n_rows;
        if (candidates) *candidates = b->b.n_candidates;
        if (stored) *stored = b->b.n_stored;
    });
}

int aic_bestshot_export(aic_bestshot* b, int stream, int32_t* n, int32_t* events, uint8_t* thumbs) {
    return with_handle(b, [&] { b->b.export_stream(stream, n, events, thumbs); });
}

}  // extern "C"
