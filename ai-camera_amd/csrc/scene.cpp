// scene.cpp -- the scene-watch object (scene.hpp) and its C ABI.  Every argument is checked before the device is touched; the
// arithmetic runs in kernels_scene.hip or the call raises.
#include "scene.hpp"

#include <algorithm>

namespace aic {

void scene_check_config(int device, const aic_scene_config* p) {
    AIC_REQUIRE(p, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(p->streams >= 1 && p->streams <= SC_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p->frame_h >= 1 && p->frame_h <= SC_DIM_MAX && p->frame_w >= 1 && p->frame_w <= SC_DIM_MAX, AIC_ERR_INVALID,
                "frame height and width must be in 1..16384");
    AIC_REQUIRE(p->cell == 4 || p->cell == 8 || p->cell == 16, AIC_ERR_INVALID, "cell must be 4, 8 or 16");
    AIC_REQUIRE(p->frame_h >= p->cell && p->frame_w >= p->cell, AIC_ERR_INVALID, "the frame is smaller than one cell");
}

Scene::Scene(int device, const aic_scene_config& p)
    : FrameBank(device, p.streams, p.frame_h, p.frame_w), g{p.streams, p.frame_h, p.frame_w, p.cell, p.frame_h / p.cell, p.frame_w / p.cell} {}

void Scene::option(const std::string& k, int value) {
    static const IntOpt<ScOpts> table[] = {
        {"thresh", &ScOpts::thresh, 0, 255}, {"noise_k_q4", &ScOpts::noise_k_q4, 0, 4096}, {"warmup", &ScOpts::warmup, 1, 1 << 20},
        {"big_thresh", &ScOpts::big_thresh, 0, 255}, {"learn_shift", &ScOpts::learn_shift, 1, 12}, {"slow_extra", &ScOpts::slow_extra, 0, 8},
        {"dev_init_q8", &ScOpts::dev_init_q8, 0, 65280}, {"min_neighbours", &ScOpts::min_neighbours, 1, 9}, {"dark_luma", &ScOpts::dark_luma, 0, 256},
        {"bright_luma", &ScOpts::bright_luma, 0, 255}, {"min_ref_q8", &ScOpts::min_ref_q8, 0, 1 << 20}, {"defocus_q8", &ScOpts::defocus_q8, 0, 256},
        {"scene_q16", &ScOpts::scene_q16, 0, 65536}, {"ref_shift", &ScOpts::ref_shift, 1, 12}, {"hold", &ScOpts::hold, 1, 1 << 20},
        {"gate_cells", &ScOpts::gate_cells, 1, 1 << 24}, {"gate_hold", &ScOpts::gate_hold, 0, 1 << 20}};
    if (launch_option(k, value, SC_TICKS_MAX)) return;
    const bool known = table_option(table, o, k, value, [](const ScOpts& n) {
        AIC_REQUIRE(n.learn_shift + n.slow_extra <= 14, AIC_ERR_INVALID, "learn_shift + slow_extra must not exceed 14");
    });
    AIC_REQUIRE(known, AIC_ERR_INVALID, "unknown scene option: " + k);
}

void Scene::touch_device() {
    use_device();
    if (!d_scalars.p) {
        const size_t n = (size_t)g.streams * cells();
        grow(d_bg, n, "the background model");
        grow(d_dev, n, "the background model");
        grow(d_prev, n, "the background model");
        grow(d_scalars, (size_t)g.streams * SC_S_INTS, "the stream scalars");
        HIP_CHECK(hipMemsetAsync(d_bg.p, 0, d_bg.bytes(), dev->s_trk));
        HIP_CHECK(hipMemsetAsync(d_dev.p, 0, d_dev.bytes(), dev->s_trk));
        HIP_CHECK(hipMemsetAsync(d_prev.p, 0, d_prev.bytes(), dev->s_trk));
        HIP_CHECK(hipMemsetAsync(d_scalars.p, 0, d_scalars.bytes(), dev->s_trk));
    }
}

void Scene::update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int32_t* records,
                   uint8_t* masks, int32_t* row_motion) {
    const int S = g.streams;
    const long F = check_call(ticks, SC_TICKS_MAX, frames_mem, rows_mem);
    AIC_REQUIRE(F == 0 || (frames && records), AIC_ERR_INVALID, "NULL frames or records");
    const bool with_rows = counts != nullptr && F > 0;
    AIC_REQUIRE(counts || !row_motion, AIC_ERR_INVALID, "row_motion without counts");
    const long total = count_rows(counts, with_rows, F, SC_ROWS_MAX, rows6, rows_mem, [&] { touch_device(); }, [&](long t) {
        AIC_REQUIRE(t == 0 || row_motion, AIC_ERR_INVALID, "rows without row_motion");
    });
    if (F == 0) return;
    hipStream_t st = dev->s_trk;
    const BankStage bs = upload(F, with_rows ? counts : nullptr, total, rows6, with_rows && rows_mem == AIC_HOST);
    const int* d_rows = bs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + bs.o_off;
    grow(d_rec, (size_t)F * SC_RECORD_INTS, "the records");
    grow(d_rm, std::max<size_t>(8, (size_t)total), "the row motion");

    const size_t tick_cells = cells() * S;
    {
        Prof pr(*dev, PROF_MISC, st, 0, (double)F * frame_bytes);
        launches(frames, frames_mem, ticks, [&](int lo, int hi) { return (size_t)(hi - lo) * tick_cells; }, [&](int lo, int hi, const uint8_t* d_fr) {
            const int n = hi - lo, n_frames = n * S;
            grow(d_gray, (size_t)n * tick_cells, "the gray grids");
            grow(d_bits, (size_t)n * tick_cells, "the model bits");
            grow(d_mask, (size_t)n * tick_cells, "the masks");
            grow(d_acc, (size_t)n_frames * SC_A_INTS, "the tick sums");
            HIP_CHECK(hipMemsetAsync(d_acc.p, 0, (size_t)n_frames * SC_A_INTS * sizeof(int), st));
            launch_scene_gray(d_fr, n_frames, g, d_gray.p, st);
            launch_scene_model(d_gray.p, n, g, o, d_scalars.p, d_stage.p, lo == 0, d_bg.p, d_dev.p, d_prev.p, d_bits.p, st);
            launch_scene_stats(d_gray.p, d_bits.p, n_frames, g, o, d_mask.p, d_acc.p, st);
            if (total) launch_scene_rows(d_mask.p, d_off + (size_t)lo * S, n_frames, max_rows(counts, lo, hi), d_rows, g, d_rm.p, st);
            launch_scene_walk(d_acc.p, n, g, o, d_stage.p, lo == 0, d_scalars.p, d_rec.p + (size_t)lo * S * SC_RECORD_INTS, st);
            if (masks) HIP_CHECK(hipMemcpyAsync(masks + (size_t)lo * tick_cells, d_mask.p, (size_t)n * tick_cells, hipMemcpyDeviceToHost, st));
        });
    }
    HIP_CHECK(hipMemcpyAsync(records, d_rec.p, (size_t)F * SC_RECORD_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    if (total) HIP_CHECK(hipMemcpyAsync(row_motion, d_rm.p, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::fill(reset_pending.begin(), reset_pending.end(), (char)0);
}

void Scene::export_stream(int stream, int32_t* bg, int32_t* dv, int32_t* prev, int32_t* scalars) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the scene bank");
    AIC_REQUIRE(bg && dv && prev && scalars, AIC_ERR_INVALID, "NULL argument");
    const size_t n = cells();
    std::fill(bg, bg + n, 0), std::fill(dv, dv + n, 0), std::fill(prev, prev + n, 0), std::fill(scalars, scalars + SC_S_INTS, 0);
    if (!d_scalars.p || reset_pending[stream]) return;                       // nothing seen yet, or a reset the next call applies
    dev->use();
    hipStream_t st = dev->s_trk;
    std::vector<uint16_t> hb(n), hd(n);
    std::vector<uint8_t> hp(n);
    HIP_CHECK(hipMemcpyAsync(hb.data(), d_bg.p + stream * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hd.data(), d_dev.p + stream * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hp.data(), d_prev.p + stream * n, n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(scalars, d_scalars.p + (size_t)stream * SC_S_INTS, SC_S_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::copy(hb.begin(), hb.end(), bg), std::copy(hd.begin(), hd.end(), dv), std::copy(hp.begin(), hp.end(), prev);
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_scene_config_default(int streams, int frame_h, int frame_w, aic_scene_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_scene_config{streams, frame_h, frame_w, 8};
    });
}

int aic_scene_create(int device, const aic_scene_config* config, aic_scene** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        scene_check_config(device, config);
        *out = new aic_scene(device, *config);
    });
}

int aic_scene_destroy(aic_scene* s) { return destroy_handle(s, s ? s->s.dev : nullptr); }

int aic_scene_option(aic_scene* s, const char* key, int value) {
    return with_handle(s, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        s->s.option(key, value);
    });
}

int aic_scene_reset(aic_scene* s, int stream) {
    return with_handle(s, [&] { s->s.reset(stream); });
}

int aic_scene_update(aic_scene* s, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                     int rows_mem, int32_t* records, uint8_t* masks, int32_t* row_motion) {
    return with_handle(s, [&] { s->s.update(frames_bgr, frames_mem, ticks, counts, rows6, rows_mem, records, masks, row_motion); });
}

int aic_scene_export(aic_scene* s, int stream, int32_t* bg, int32_t* dev, int32_t* prev, int32_t* scalars) {
    return with_handle(s, [&] { s->s.export_stream(stream, bg, dev, prev, scalars); });
}

}  // extern "C"
