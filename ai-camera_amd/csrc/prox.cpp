// prox.cpp -- the proximity object (prox.hpp) and its C ABI.  Every argument is checked before the device is touched; the arithmetic runs in
// kernels_prox.hip or the call raises.
#include "prox.hpp"

#include <algorithm>

namespace aic {

static void check_rules(const ProxOptions& o) {
    AIC_REQUIRE(o.near <= (o.metric == PROX_GROUND ? 1 << 24 : 4096), AIC_ERR_INVALID,
                "near must be in 1..2^24 ground units (metric 0) or 1..4096 per mille of body height (metric 1)");
    AIC_REQUIRE(o.still_speed <= o.run_speed, AIC_ERR_INVALID, "still_speed must not exceed run_speed");
}

void prox_check_params(int device, const aic_prox_config* p) {
    AIC_REQUIRE(p, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(p->streams >= 1 && p->streams <= PX_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p->frame_h >= 1 && p->frame_h <= PX_DIM_MAX && p->frame_w >= 1 && p->frame_w <= PX_DIM_MAX, AIC_ERR_INVALID,
                "frame height and width must be in 1..16384");
    AIC_REQUIRE(p->max_tracks >= 1 && p->max_tracks <= PX_TRACKS_MAX, AIC_ERR_INVALID, "max_tracks must be in 1..512");
    AIC_REQUIRE(p->forget_after >= 0 && p->forget_after <= (1 << 24), AIC_ERR_INVALID, "forget_after must be in 0..2^24");
    AIC_REQUIRE(p->metric == PROX_GROUND || p->metric == PROX_BODY, AIC_ERR_INVALID, "metric must be 0 (ground plane) or 1 (body height)");
    AIC_REQUIRE(p->near >= 1 && p->near <= (1 << 24), AIC_ERR_INVALID, "near must be in 1..2^24");
    AIC_REQUIRE(p->height_ratio_q8 >= 256 && p->height_ratio_q8 <= (1 << 16), AIC_ERR_INVALID, "height_ratio_q8 must be in 256..65536");
    AIC_REQUIRE(p->link_ticks >= 1 && p->link_ticks <= 32767, AIC_ERR_INVALID, "link_ticks must be in 1..32767");
    AIC_REQUIRE(p->unlink_ticks >= 1 && p->unlink_ticks <= 32767, AIC_ERR_INVALID, "unlink_ticks must be in 1..32767");
    AIC_REQUIRE(p->speed_shift >= 0 && p->speed_shift <= 12, AIC_ERR_INVALID, "speed_shift must be in 0..12");
    AIC_REQUIRE(p->still_speed >= 0 && p->still_speed <= (1 << 20), AIC_ERR_INVALID, "still_speed must be in 0..2^20");
    AIC_REQUIRE(p->run_speed >= 0 && p->run_speed <= (1 << 20), AIC_ERR_INVALID, "run_speed must be in 0..2^20");
    check_rules(ProxOptions{p->forget_after, p->metric, p->near, p->height_ratio_q8, p->link_ticks, p->unlink_ticks, p->speed_shift, p->still_speed,
                            p->run_speed});
}

Prox::Prox(int device, const aic_prox_config& p)
    : SlotBank(device, p.streams, p.frame_h, p.frame_w), g{p.streams, p.frame_h, p.frame_w, p.max_tracks},
      o{p.forget_after, p.metric, p.near, p.height_ratio_q8, p.link_ticks, p.unlink_ticks, p.speed_shift, p.still_speed, p.run_speed},
      grounds(p.streams, ProxGround{{1, 0, 0, 0, 1, 0, 0, 0, 1}, 0}) {}

void Prox::option(const std::string& k, int value) {
    static const IntOpt<ProxOptions> table[] = {{"forget_after", &ProxOptions::forget_after, 0, 1 << 24}, {"metric", &ProxOptions::metric, 0, 1},
                                                {"near", &ProxOptions::near, 1, 1 << 24}, {"height_ratio_q8", &ProxOptions::height_ratio_q8, 256, 1 << 16},
                                                {"link_ticks", &ProxOptions::link_ticks, 1, 32767}, {"unlink_ticks", &ProxOptions::unlink_ticks, 1, 32767},
                                                {"speed_shift", &ProxOptions::speed_shift, 0, 12}, {"still_speed", &ProxOptions::still_speed, 0, 1 << 20},
                                                {"run_speed", &ProxOptions::run_speed, 0, 1 << 20}};
    if (table_option(table, o, k, value, check_rules)) return;
    AIC_REQUIRE(launch_option(k, value, PX_TICKS_MAX), AIC_ERR_INVALID, "unknown proximity option: " + k);
}

void Prox::reset(int stream) { reset_stream(stream, "stream outside the proximity bank"); }

void Prox::set_ground(int stream, const int32_t* H, int shift) {
    AIC_REQUIRE(stream >= -1 && stream < g.streams, AIC_ERR_INVALID, "stream outside the proximity bank (-1 = every stream)");
    AIC_REQUIRE(H, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(shift >= 0 && shift <= 14, AIC_ERR_INVALID, "shift must be in 0..14");
    ProxGround m{};
    for (int k = 0; k < 9; ++k) {
        AIC_REQUIRE(H[k] >= -(1 << 30) && H[k] <= (1 << 30), AIC_ERR_INVALID, "a ground map entry outside -2^30..2^30");
        m.h[k] = H[k];
    }
    m.shift = shift;
    for (int s = 0; s < g.streams; ++s)
        if (stream < 0 || stream == s) grounds[s] = m;
}

// the device and the resident buffers
void Prox::touch_device() {
    use_device();
    hipStream_t st = dev->s_trk;
    if (!d_state.p) {
        grow(d_state, (size_t)g.streams * PX_ST_INTS, "the slot tables");
        HIP_CHECK(hipMemsetAsync(d_state.p, 0, d_state.bytes(), st));
    }
    if (!d_pairs.p) {
        grow(d_pairs, std::max<size_t>(2, (size_t)g.streams * g.pairs() * 2), "the pair tables");
        HIP_CHECK(hipMemsetAsync(d_pairs.p, 0, d_pairs.bytes(), st));
    }
    grow(d_ground, (size_t)g.streams * (sizeof(ProxGround) / sizeof(int)), "the ground maps");
}

static void check_outputs(int cap, const int32_t* n_final, const int32_t* events, const int32_t* pending) {
    AIC_REQUIRE(cap >= 0 && cap <= PX_CAP_MAX, AIC_ERR_INVALID, "cap must be in 0..4096");
    AIC_REQUIRE(n_final && pending, AIC_ERR_INVALID, "NULL n_final or pending");
    AIC_REQUIRE(cap == 0 || events, AIC_ERR_INVALID, "NULL events");
}

void Prox::walk(const int* d_off, int n_ticks, const int* d_rows, const BankStage& bs, int first, int cap, const SlotOut& so, const ProxOut& po) {
    int* out = d_out.p;
    const ProxRules r{o.metric, o.near, o.height_ratio_q8, o.link_ticks, o.unlink_ticks, o.speed_shift, o.still_speed, o.run_speed};
    launch_prox_walk(d_off, n_ticks, d_rows, d_stage.p, d_stage.p + bs.o_mode, first, g, o.forget_after, r, reinterpret_cast<const ProxGround*>(d_ground.p),
                     d_state.p, d_pairs.p, cap, out, out + so.o_pending, out + so.o_status, out + so.o_events, po, dev->s_trk);
}

void Prox::update(int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int cap_pairs, int32_t* n_final, int32_t* events,
                  int32_t* pending, int32_t* status, int32_t* records, int32_t* row_tags, int32_t* n_pair_events, int32_t* pair_events) {
    const int S = g.streams;
    const long F = check_call(ticks, PX_TICKS_MAX, AIC_DEVICE, rows_mem);
    check_outputs(cap, n_final, events, pending);
    AIC_REQUIRE(cap_pairs >= 0 && cap_pairs <= PX_CAP_PAIRS_MAX, AIC_ERR_INVALID, "cap_pairs must be in 0..4096");
    AIC_REQUIRE(F == 0 || counts, AIC_ERR_INVALID, "NULL counts");
    AIC_REQUIRE(F == 0 || (records && n_pair_events), AIC_ERR_INVALID, "NULL records or n_pair_events");
    AIC_REQUIRE(F == 0 || cap_pairs == 0 || pair_events, AIC_ERR_INVALID, "NULL pair_events");
    const long total = count_rows(counts, F > 0, F, PX_ROWS_MAX, rows6, rows_mem, [&] { touch_device(); }, [&](long t) {
        AIC_REQUIRE(t <= (1 << 24), AIC_ERR_INVALID, "more than 2^24 rows in one call");
        AIC_REQUIRE(t == 0 || row_tags, AIC_ERR_INVALID, "NULL row_tags");
    });
    hipStream_t st = dev->s_trk;
    const BankStage bs = upload_update(F, counts, total, rows6, rows_mem == AIC_HOST);
    const int* d_rows = bs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + bs.o_off;
    const SlotOut so = out(cap, PX_EVENT_INTS);
    if (F > 0) {                                                             // (the maps are pageable: the copy has left them on return)
        HIP_CHECK(hipMemcpyAsync(d_ground.p, grounds.data(), grounds.size() * sizeof(ProxGround), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    {
        const size_t frame_bytes_out = (PX_RECORD_INTS + 1 + (size_t)cap_pairs * PX_PAIR_EVENT_INTS) * sizeof(int), tag_bytes = PX_TAG_INTS * sizeof(int);
        Prof pr(*dev, PROF_TRK, st, 0, (double)total * (6 * sizeof(int) + tag_bytes) + (double)F * frame_bytes_out);
        if (ticks == 0) walk(d_off, 0, d_rows, bs, 1, cap, so, ProxOut{nullptr, nullptr, nullptr, nullptr, 0, 0});
        launches(nullptr, AIC_DEVICE, ticks,
                 [&](int lo, int hi) { return bs.rows_of(h_stage.p, lo, hi) * tag_bytes + (size_t)(hi - lo) * S * frame_bytes_out; },
                 [&](int lo, int hi, const uint8_t*) {
                     const size_t Fl = (size_t)(hi - lo) * S, f0 = (size_t)lo * S, rows_l = bs.rows_of(h_stage.p, lo, hi);
                     const size_t row0 = (size_t)h_stage.p[bs.o_off + f0], n_pe = Fl * cap_pairs * PX_PAIR_EVENT_INTS;
                     grow(d_rec, Fl * (PX_RECORD_INTS + 1), "the records");
                     grow(d_pe, std::max<size_t>(n_pe, 1), "the pair events");
                     grow(d_tags, std::max<size_t>(rows_l * PX_TAG_INTS, 1), "the row tags");
                     if (n_pe) HIP_CHECK(hipMemsetAsync(d_pe.p, 0, n_pe * sizeof(int), st));
                     int* d_npe = d_rec.p + Fl * PX_RECORD_INTS;
                     walk(d_off + f0, hi - lo, d_rows, bs, lo == 0, cap, so, ProxOut{d_rec.p, d_npe, d_pe.p, d_tags.p, cap_pairs, (int)row0});
                     HIP_CHECK(hipMemcpyAsync(records + f0 * PX_RECORD_INTS, d_rec.p, Fl * PX_RECORD_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
                     HIP_CHECK(hipMemcpyAsync(n_pair_events + f0, d_npe, Fl * sizeof(int), hipMemcpyDeviceToHost, st));
                     if (n_pe) HIP_CHECK(hipMemcpyAsync(pair_events + f0 * cap_pairs * PX_PAIR_EVENT_INTS, d_pe.p, n_pe * sizeof(int), hipMemcpyDeviceToHost, st));
                     if (rows_l) HIP_CHECK(hipMemcpyAsync(row_tags + row0 * PX_TAG_INTS, d_tags.p, rows_l * PX_TAG_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
                     HIP_CHECK(hipStreamSynchronize(st));                    // the launch's buffers are free for the next one
                 });
    }
    finish(cap, PX_EVENT_INTS, n_final, events, pending, status, [](int, int) {});
}

void Prox::flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    AIC_REQUIRE(stream >= -1 && stream < g.streams, AIC_ERR_INVALID, "stream outside the proximity bank (-1 = every stream)");
    check_outputs(cap, n_final, events, pending);
    touch_device();
    const BankStage bs = upload_flush(stream);
    walk(d_stage.p + bs.o_off, 0, nullptr, bs, 1, cap, out(cap, PX_EVENT_INTS), ProxOut{nullptr, nullptr, nullptr, nullptr, 0, 0});
    finish(cap, PX_EVENT_INTS, n_final, events, pending, status, [](int, int) {});
}

// the stream's table on the host; false: nothing seen yet, or a reset the next call applies
bool Prox::fetch_state(int stream) {
    if (!d_state.p || reset_pending[stream]) return false;
    dev->use();
    hipStream_t st = dev->s_trk;
    h_state.resize(PX_ST_INTS);
    HIP_CHECK(hipMemcpyAsync(h_state.data(), d_state.p + (size_t)stream * PX_ST_INTS, PX_ST_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return true;
}

void Prox::export_stream(int stream, int32_t* n, int32_t* events) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the proximity bank");
    AIC_REQUIRE(n && events, AIC_ERR_INVALID, "NULL argument");
    *n = 0;
    if (!fetch_state(stream)) return;
    const int* a = h_state.data() + SLOT_ST_SLOTS;
    auto at = [&](int arr, int t) { return a[arr * PX_TRACKS_MAX + t]; };
    int k = 0;
    for (int t = 0; t < g.max_tracks; ++t) {
        const int state = at(SLOT_A_STATE, t);
        if (!state) continue;
        const int32_t ev[PX_EVENT_INTS] = {state == 1 ? SLOT_LIVE : state == 3 ? SLOT_FLUSHED : SLOT_EXPIRED, stream, at(SLOT_A_ID, t), at(SLOT_A_CLS, t),
                                           at(SLOT_A_FIRST, t), at(SLOT_A_LAST, t), at(SLOT_A_SIGHT, t), at(PX_A_LINKS, t), at(PX_A_DIST, t),
                                           at(PX_A_MAXV, t), at(PX_A_VQ8, t), at(PX_A_PTICKS, t), at(PX_A_MAXP, t), at(PX_A_GX, t), at(PX_A_GY, t),
                                           at(PX_A_GAIT, t)};
        std::copy(ev, ev + PX_EVENT_INTS, events + (size_t)k * PX_EVENT_INTS);
        ++k;
    }
    *n = k;
}

void Prox::export_pairs(int stream, int32_t* n, int32_t* out6) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the proximity bank");
    AIC_REQUIRE(n && out6, AIC_ERR_INVALID, "NULL argument");
    *n = 0;
    if (!fetch_state(stream) || g.pairs() == 0) return;
    hipStream_t st = dev->s_trk;
    h_pairs.resize(g.pairs() * 2);
    HIP_CHECK(hipMemcpyAsync(h_pairs.data(), d_pairs.p + (size_t)stream * g.pairs() * 2, h_pairs.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int* a = h_state.data() + SLOT_ST_SLOTS;
    auto at = [&](int arr, int t) { return a[arr * PX_TRACKS_MAX + t]; };
    int k = 0;
    for (int lo = 0; lo < g.max_tracks; ++lo)
        for (int hi = lo + 1; hi < g.max_tracks; ++hi) {
            if (at(SLOT_A_STATE, lo) != 1 || at(SLOT_A_STATE, hi) != 1) continue;
            const int x = h_pairs[2 * (size_t)prox_pair_index(lo, hi)], since = h_pairs[2 * (size_t)prox_pair_index(lo, hi) + 1];
            if (!x) continue;
            const int32_t e[6] = {at(SLOT_A_ID, lo), at(SLOT_A_ID, hi), prox_linked(x), prox_on(x), prox_off(x), since};
            std::copy(e, e + 6, out6 + (size_t)k * 6);
            ++k;
        }
    *n = k;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_prox_config_default(int streams, int frame_h, int frame_w, aic_prox_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_prox_config{streams, frame_h, frame_w, 128, 70, PROX_BODY, 700, 384, 30, 60, 2, 5, 70};
    });
}

int aic_prox_create(int device, const aic_prox_config* config, aic_prox** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        prox_check_params(device, config);
        *out = new aic_prox(device, *config);
    });
}

int aic_prox_destroy(aic_prox* h) { return destroy_handle(h, h ? h->c.dev : nullptr); }

int aic_prox_option(aic_prox* h, const char* key, int value) {
    return with_handle(h, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        h->c.option(key, value);
    });
}

int aic_prox_reset(aic_prox* h, int stream) {
    return with_handle(h, [&] { h->c.reset(stream); });
}

int aic_prox_set_ground(aic_prox* h, int stream, const int32_t* H, int shift) {
    return with_handle(h, [&] { h->c.set_ground(stream, H, shift); });
}

int aic_prox_update(aic_prox* h, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int cap_pairs, int32_t* n_final,
                    int32_t* events, int32_t* pending, int32_t* status, int32_t* records, int32_t* row_tags, int32_t* n_pair_events,
                    int32_t* pair_events) {
    return with_handle(h, [&] {
        h->c.update(ticks, counts, rows6, rows_mem, cap, cap_pairs, n_final, events, pending, status, records, row_tags, n_pair_events, pair_events);
    });
}

int aic_prox_flush(aic_prox* h, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    return with_handle(h, [&] { h->c.flush(stream, cap, n_final, events, pending, status); });
}

int aic_prox_export(aic_prox* h, int stream, int32_t* n, int32_t* events) {
    return with_handle(h, [&] { h->c.export_stream(stream, n, events); });
}

int aic_prox_export_pairs(aic_prox* h, int stream, int32_t* n, int32_t* out6) {
    return with_handle(h, [&] { h->c.export_pairs(stream, n, out6); });
}

}  // extern "C"
