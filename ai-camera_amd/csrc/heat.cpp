// heat.cpp -- the heat-map object (heat.hpp) and its C ABI.  Every argument is checked before the device is touched; the arithmetic runs in
// kernels_heat.hip or the call raises.  aic_heat_lut is the host's copy of the default colour ramp.
#include "heat.hpp"

#include <algorithm>

namespace aic {

static int log2_of(int cell) { return cell == 4 ? 2 : cell == 8 ? 3 : cell == 16 ? 4 : 5; }

void heat_check_params(int device, const aic_heat_config* p) {
    AIC_REQUIRE(p, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(p->streams >= 1 && p->streams <= HT_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p->frame_h >= 1 && p->frame_h <= HT_DIM_MAX && p->frame_w >= 1 && p->frame_w <= HT_DIM_MAX, AIC_ERR_INVALID,
                "frame height and width must be in 1..16384");
    AIC_REQUIRE(p->cell == 4 || p->cell == 8 || p->cell == 16 || p->cell == 32, AIC_ERR_INVALID, "cell must be 4, 8, 16 or 32");
    AIC_REQUIRE(p->max_tracks >= 1 && p->max_tracks <= HT_TRACKS_MAX, AIC_ERR_INVALID, "max_tracks must be in 1..512");
    AIC_REQUIRE(p->forget_after >= 0 && p->forget_after <= (1 << 24), AIC_ERR_INVALID, "forget_after must be in 0..2^24");
    AIC_REQUIRE(p->anchor == HEAT_FOOT || p->anchor == HEAT_CENTRE, AIC_ERR_INVALID, "anchor must be 0 (foot) or 1 (centre)");
    AIC_REQUIRE(p->min_move >= 1 && p->min_move <= (1 << 20), AIC_ERR_INVALID, "min_move must be in 1..2^20");
    const HeatGeom g = heat_geom(*p);
    AIC_REQUIRE((long)g.gw * g.gh <= HT_CELLS_MAX, AIC_ERR_CAPACITY, "a grid of more than 32768 cells: choose a larger cell");
}

HeatGeom heat_geom(const aic_heat_config& p) {
    const int lc = log2_of(p.cell);
    return HeatGeom{p.streams, p.frame_h, p.frame_w, lc, (p.frame_w + p.cell - 1) >> lc, (p.frame_h + p.cell - 1) >> lc, p.max_tracks, p.forget_after,
                    p.anchor, p.min_move};
}

void heat_default_lut(uint8_t* bgr) {
    for (int L = 0; L < 256; ++L)
        for (int c = 0; c < 3; ++c) bgr[3 * L + c] = (uint8_t)heat_ramp(L, 2 - c);
}

Heat::Heat(int device, const aic_heat_config& p) : SlotBank(device, p.streams, p.frame_h, p.frame_w), g(heat_geom(p)), layer_reset(p.streams, 0) {
    uint8_t t[768];
    heat_default_lut(t);
    set_lut(t);
}

void Heat::option(const std::string& k, int value) {
    static const IntOpt<HeatOptions> table[] = {{"scale", &HeatOptions::scale, 0, 1}, {"alpha_q8", &HeatOptions::alpha_q8, 0, 256},
                                                {"floor", &HeatOptions::floor, 0, 255}, {"chunk_frames", &HeatOptions::chunk_frames, 0, HT_FRAMES_MAX}};
    if (table_option(table, o, k, value, [](const HeatOptions&) {})) return;
    AIC_REQUIRE(launch_option(k, value, HT_TICKS_MAX), AIC_ERR_INVALID, "unknown heat option: " + k);
}

void Heat::reset(int stream) {
    reset_stream(stream, "stream outside the heat bank");
    layer_reset[stream] = 1;
}

// the device, the resident buffers, and the layers of the streams reset since the last call, zeroed in stream order
void Heat::touch_device() {
    use_device();
    hipStream_t st = dev->s_trk;
    const size_t per = (size_t)HEAT_LAYERS * g.cells();
    if (!d_state.p) {
        grow(d_state, (size_t)g.streams * HT_ST_INTS, "the slot tables");
        HIP_CHECK(hipMemsetAsync(d_state.p, 0, d_state.bytes(), st));
    }
    if (!d_layers.p) {
        grow(d_layers, (size_t)g.streams * per, "the layers");
        HIP_CHECK(hipMemsetAsync(d_layers.p, 0, d_layers.bytes(), st));
        std::fill(layer_reset.begin(), layer_reset.end(), (char)0);
    }
    for (int s = 0; s < g.streams; ++s)
        if (layer_reset[s]) {
            HIP_CHECK(hipMemsetAsync(d_layers.p + s * per, 0, per * sizeof(int), st));
            layer_reset[s] = 0;
        }
}

static void check_outputs(int cap, const int32_t* n_final, const int32_t* events, const int32_t* pending) {
    AIC_REQUIRE(cap >= 0 && cap <= HT_CAP_MAX, AIC_ERR_INVALID, "cap must be in 0..4096");
    AIC_REQUIRE(n_final && pending, AIC_ERR_INVALID, "NULL n_final or pending");
    AIC_REQUIRE(cap == 0 || events, AIC_ERR_INVALID, "NULL events");
}

void Heat::walk(const int* d_off, int n_ticks, const int* d_rows, const BankStage& bs, int first, int cap, const SlotOut& so, int* d_rt) {
    int* out = d_out.p;
    launch_heat_walk(d_off, n_ticks, d_rows, d_stage.p, d_stage.p + bs.o_mode, first, g, d_state.p, d_layers.p, cap, out, out + so.o_pending,
                     out + so.o_status, out + so.o_events, d_rt, dev->s_trk);
}

void Heat::update(int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int32_t* n_final, int32_t* events, int32_t* row_tags,
                  int32_t* pending, int32_t* status) {
    const int S = g.streams;
    const long F = check_call(ticks, HT_TICKS_MAX, AIC_DEVICE, rows_mem);
    check_outputs(cap, n_final, events, pending);
    AIC_REQUIRE(F == 0 || counts, AIC_ERR_INVALID, "NULL counts");
    const long total = count_rows(counts, F > 0, F, HT_ROWS_MAX, rows6, rows_mem, [&] { touch_device(); }, [](long t) {
        AIC_REQUIRE(t <= (1 << 24), AIC_ERR_INVALID, "more than 2^24 rows in one call");
    });
    hipStream_t st = dev->s_trk;
    const BankStage bs = upload_update(F, counts, total, rows6, rows_mem == AIC_HOST);
    const int* d_rows = bs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + bs.o_off;
    const SlotOut so = out(cap, HT_EVENT_INTS);
    int* d_rt = nullptr;
    if (row_tags && total) {
        grow(d_tags, (size_t)total * 4, "the row tags");
        d_rt = d_tags.p;
    }
    {
        const size_t tag_bytes = 4 * sizeof(int);
        Prof pr(*dev, PROF_TRK, st, 0, (double)total * (6 * sizeof(int) + tag_bytes));
        if (ticks == 0) walk(d_off, 0, d_rows, bs, 1, cap, so, nullptr);
        launches(nullptr, AIC_DEVICE, ticks, [&](int lo, int hi) { return bs.rows_of(h_stage.p, lo, hi) * tag_bytes; },
                 [&](int lo, int hi, const uint8_t*) { walk(d_off + (size_t)lo * S, hi - lo, d_rows, bs, lo == 0, cap, so, d_rt); });
    }
    if (d_rt) HIP_CHECK(hipMemcpyAsync(row_tags, d_rt, (size_t)total * 4 * sizeof(int), hipMemcpyDeviceToHost, st));
    finish(cap, HT_EVENT_INTS, n_final, events, pending, status, [](int, int) {});
}

void Heat::flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    AIC_REQUIRE(stream >= -1 && stream < g.streams, AIC_ERR_INVALID, "stream outside the heat bank (-1 = every stream)");
    check_outputs(cap, n_final, events, pending);
    touch_device();
    const BankStage bs = upload_flush(stream);
    walk(d_stage.p + bs.o_off, 0, nullptr, bs, 1, cap, out(cap, HT_EVENT_INTS), nullptr);
    finish(cap, HT_EVENT_INTS, n_final, events, pending, status, [](int, int) {});
}

void Heat::export_stream(int stream, int32_t* n, int32_t* events) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the heat bank");
    AIC_REQUIRE(n && events, AIC_ERR_INVALID, "NULL argument");
    *n = 0;
    if (!d_state.p || reset_pending[stream]) return;                         // nothing seen yet, or a reset the next call applies
    dev->use();
    hipStream_t st = dev->s_trk;
    h_state.resize(HT_ST_INTS);
    HIP_CHECK(hipMemcpyAsync(h_state.data(), d_state.p + (size_t)stream * HT_ST_INTS, HT_ST_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int* a = h_state.data() + SLOT_ST_SLOTS;
    auto at = [&](int arr, int t) { return a[arr * HT_TRACKS_MAX + t]; };
    int k = 0;
    for (int t = 0; t < g.max_tracks; ++t) {
        const int state = at(SLOT_A_STATE, t);
        if (!state) continue;
        const int32_t ev[HT_EVENT_INTS] = {state == 1 ? SLOT_LIVE : state == 3 ? SLOT_FLUSHED : SLOT_EXPIRED, stream, at(SLOT_A_ID, t), at(SLOT_A_CLS, t),
                                           at(SLOT_A_FIRST, t), at(SLOT_A_LAST, t), at(SLOT_A_SIGHT, t), at(HT_A_CELLS, t), at(HT_A_SFX, t),
                                           at(HT_A_SFY, t), at(HT_A_FX, t), at(HT_A_FY, t), at(HT_A_PATH, t), at(HT_A_MAXSTEP, t), at(HT_A_MOVING, t),
                                           at(HT_A_CELL, t)};
        std::copy(ev, ev + HT_EVENT_INTS, events + (size_t)k * HT_EVENT_INTS);
        ++k;
    }
    *n = k;
}

static int check_layers(const HeatGeom& g, int stream, int layer_mask, bool all_streams) {
    AIC_REQUIRE(stream >= (all_streams ? -1 : 0) && stream < g.streams, AIC_ERR_INVALID,
                all_streams ? "stream outside the heat bank (-1 = every stream)" : "stream outside the heat bank");
    AIC_REQUIRE(layer_mask > 0 && layer_mask < (1 << HEAT_LAYERS), AIC_ERR_INVALID, "layer_mask must name at least one of the 12 layers");
    return __builtin_popcount((unsigned)layer_mask);
}

void Heat::decay(int stream, int layer_mask, int shift) {
    check_layers(g, stream, layer_mask, true);
    AIC_REQUIRE(shift >= 1 && shift <= 31, AIC_ERR_INVALID, "shift must be in 1..31");
    touch_device();
    launch_heat_decay(d_layers.p, g, stream, layer_mask, shift, dev->s_trk);
}

void Heat::export_layers(int stream, int layer_mask, int32_t* out) {
    check_layers(g, stream, layer_mask, false);
    AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
    touch_device();
    hipStream_t st = dev->s_trk;
    const size_t cells = g.cells();
    for (int l = 0, k = 0; l < HEAT_LAYERS; ++l)
        if ((layer_mask >> l) & 1)
            HIP_CHECK(hipMemcpyAsync(out + cells * k++, d_layers.p + ((size_t)stream * HEAT_LAYERS + l) * cells, cells * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

void Heat::import_layers(int stream, int layer_mask, const int32_t* in) {
    const int n = check_layers(g, stream, layer_mask, false);
    AIC_REQUIRE(in, AIC_ERR_INVALID, "NULL argument");
    const size_t cells = g.cells();
    for (size_t i = 0; i < cells * n; ++i) AIC_REQUIRE(in[i] >= 0 && in[i] <= HEAT_SAT, AIC_ERR_INVALID, "a layer value outside 0..2^30");
    touch_device();
    hipStream_t st = dev->s_trk;
    for (int l = 0, k = 0; l < HEAT_LAYERS; ++l)
        if ((layer_mask >> l) & 1)
            HIP_CHECK(hipMemcpyAsync(d_layers.p + ((size_t)stream * HEAT_LAYERS + l) * cells, in + cells * k++, cells * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                                     // the caller's array is free on return
}

void Heat::set_lut(const uint8_t* bgr) {
    AIC_REQUIRE(bgr, AIC_ERR_INVALID, "NULL argument");
    for (int L = 0; L < 256; ++L) lut[L] = (unsigned)bgr[3 * L] | (unsigned)bgr[3 * L + 1] << 8 | (unsigned)bgr[3 * L + 2] << 16;
    lut_dirty = true;
}

void Heat::render(void* frames, int n_frames, int mem, const int32_t* cameras, int layer) {
    const int S = g.streams;
    AIC_REQUIRE(n_frames >= 0 && n_frames <= HT_FRAMES_MAX, AIC_ERR_INVALID, "n_frames must be in 0..65536");
    AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(layer >= 0 && layer < HEAT_LAYERS, AIC_ERR_INVALID, "layer must be in 0..11");
    AIC_REQUIRE(n_frames == 0 || frames, AIC_ERR_INVALID, "NULL frames");
    if (cameras)
        for (int f = 0; f < n_frames; ++f) AIC_REQUIRE(cameras[f] >= 0 && cameras[f] < S, AIC_ERR_INVALID, "a camera outside the heat bank");
    touch_device();
    if (n_frames == 0) return;
    hipStream_t st = dev->s_trk;
    // ---- staging ints: frame_cam[n_frames] | used[n_used]
    h_stage.ensure((size_t)n_frames + S);
    grow(d_stage, (size_t)n_frames + S, "the staging buffer");
    std::vector<char> seen(S, 0);
    int n_used = 0;
    for (int f = 0; f < n_frames; ++f) {
        const int c = cameras ? cameras[f] : f % S;
        h_stage.p[f] = c;
        if (!seen[c]) seen[c] = 1, h_stage.p[n_frames + n_used++] = c;
    }
    HIP_CHECK(hipMemcpyAsync(d_stage.p, h_stage.p, ((size_t)n_frames + n_used) * sizeof(int), hipMemcpyHostToDevice, st));
    grow(d_max, S, "the maxima");
    grow(d_levels, (size_t)S * g.cells(), "the levels");
    grow(d_lut, 256, "the colour table");
    if (lut_dirty) {
        HIP_CHECK(hipMemcpyAsync(d_lut.p, lut, sizeof(lut), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));                                 // lut is pageable: the copy has left it
        lut_dirty = false;
    }
    launch_heat_levels(d_layers.p, g, layer, o.scale, d_stage.p + n_frames, n_used, d_max.p, d_levels.p, st);
    const int chunk = std::min(o.chunk_frames > 0 ? o.chunk_frames : n_frames, 65535);
    uint8_t* fr = static_cast<uint8_t*>(frames);
    for (int lo = 0; lo < n_frames; lo += chunk) {
        const int n = std::min(chunk, n_frames - lo);
        uint8_t* d_fr = fr + (size_t)lo * frame_bytes;
        if (mem == AIC_HOST) {
            grow(d_frames, (size_t)n * frame_bytes, "the staged frames");
            HIP_CHECK(hipMemcpyAsync(d_frames.p, d_fr, (size_t)n * frame_bytes, hipMemcpyHostToDevice, st));
            d_fr = d_frames.p;
        }
        {
            Prof pr(*dev, PROF_MISC, st, 0, 2.0 * n * frame_bytes);
            launch_heat_render(d_fr, n, d_stage.p + lo, g, d_max.p, d_levels.p, d_lut.p, o.alpha_q8, o.floor, st);
        }
        if (mem == AIC_HOST) {
            HIP_CHECK(hipMemcpyAsync(fr + (size_t)lo * frame_bytes, d_frames.p, (size_t)n * frame_bytes, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));                             // the staging buffer is free for the next chunk
        }
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_heat_config_default(int streams, int frame_h, int frame_w, aic_heat_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_heat_config{streams, frame_h, frame_w, 16, 128, 70, HEAT_FOOT, 4};
    });
}

int aic_heat_create(int device, const aic_heat_config* config, aic_heat** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        heat_check_params(device, config);
        *out = new aic_heat(device, *config);
    });
}

int aic_heat_destroy(aic_heat* h) { return destroy_handle(h, h ? h->c.dev : nullptr); }

int aic_heat_option(aic_heat* h, const char* key, int value) {
    return with_handle(h, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        h->c.option(key, value);
    });
}

int aic_heat_reset(aic_heat* h, int stream) {
    return with_handle(h, [&] { h->c.reset(stream); });
}

int aic_heat_update(aic_heat* h, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int32_t* n_final, int32_t* events,
                    int32_t* row_tags, int32_t* pending, int32_t* status) {
    return with_handle(h, [&] { h->c.update(ticks, counts, rows6, rows_mem, cap, n_final, events, row_tags, pending, status); });
}

int aic_heat_flush(aic_heat* h, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status) {
    return with_handle(h, [&] { h->c.flush(stream, cap, n_final, events, pending, status); });
}

int aic_heat_export(aic_heat* h, int stream, int32_t* n, int32_t* events) {
    return with_handle(h, [&] { h->c.export_stream(stream, n, events); });
}

int aic_heat_decay(aic_heat* h, int stream, int layer_mask, int shift) {
    return with_handle(h, [&] { h->c.decay(stream, layer_mask, shift); });
}

int aic_heat_export_layers(aic_heat* h, int stream, int layer_mask, int32_t* out) {
    return with_handle(h, [&] { h->c.export_layers(stream, layer_mask, out); });
}

int aic_heat_import_layers(aic_heat* h, int stream, int layer_mask, const int32_t* layers) {
    return with_handle(h, [&] { h->c.import_layers(stream, layer_mask, layers); });
}

int aic_heat_set_lut(aic_heat* h, const uint8_t* bgr) {
    return with_handle(h, [&] { h->c.set_lut(bgr); });
}

int aic_heat_lut(uint8_t* bgr) {
    return guarded([&] {
        AIC_REQUIRE(bgr, AIC_ERR_INVALID, "NULL argument");
        heat_default_lut(bgr);
    });
}

int aic_heat_render(aic_heat* h, uint8_t* frames_bgr, int n_frames, int mem, const int32_t* cameras, int layer) {
    return with_handle(h, [&] { h->c.render(frames_bgr, n_frames, mem, cameras, layer); });
}

}  // extern "C"
