// left.cpp -- the left-objects stage (left.hpp) and its C ABI.  Every argument is checked before the device is touched; the
// arithmetic runs in kernels_left.hip (and launch_scene_gray) or the call raises.
#include "left.hpp"

#include <algorithm>

namespace aic {

void left_check_config(int device, const aic_left_config* p) {
    AIC_REQUIRE(p, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(p->streams >= 1 && p->streams <= SC_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p->frame_h >= 1 && p->frame_h <= SC_DIM_MAX && p->frame_w >= 1 && p->frame_w <= SC_DIM_MAX, AIC_ERR_INVALID,
                "frame height and width must be in 1..16384");
    AIC_REQUIRE(p->cell == 4 || p->cell == 8 || p->cell == 16, AIC_ERR_INVALID, "cell must be 4, 8 or 16");
    AIC_REQUIRE(p->frame_h >= p->cell && p->frame_w >= p->cell, AIC_ERR_INVALID, "the frame is smaller than one cell");
    AIC_REQUIRE(p->max_objects >= 1 && p->max_objects <= LF_OBJECTS_MAX, AIC_ERR_INVALID, "max_objects must be in 1..64");
    AIC_REQUIRE((long)(p->frame_h / p->cell) * (p->frame_w / p->cell) <= LF_CELLS_MAX, AIC_ERR_CAPACITY,
                "a grid of more than 32768 cells: choose a larger cell");
}

Left::Left(int device, const aic_left_config& p)
    : FrameBank(device, p.streams, p.frame_h, p.frame_w), g{p.streams, p.frame_h, p.frame_w, p.cell, p.frame_h / p.cell, p.frame_w / p.cell},
      max_objects(p.max_objects) {}

void Left::option(const std::string& k, int value) {
    static const IntOpt<LfOpts> table[] = {
        {"fast_shift", &LfOpts::fast_shift, 1, 8}, {"slow_shift", &LfOpts::slow_shift, 1, 12}, {"thresh", &LfOpts::thresh, 1, 255},
        {"warmup", &LfOpts::warmup, 1, 1 << 20}, {"decay", &LfOpts::decay, 0, 64}, {"min_ticks", &LfOpts::min_ticks, 1, 65534},
        {"absorb_ticks", &LfOpts::absorb_ticks, 2, 65535}, {"pad_cells", &LfOpts::pad_cells, 0, 8}, {"owner_window", &LfOpts::owner_window, 0, 1 << 20},
        {"min_cells", &LfOpts::min_cells, 1, LF_CELLS_MAX}, {"max_cells", &LfOpts::max_cells, 1, LF_CELLS_MAX},
        {"alarm_hold", &LfOpts::alarm_hold, 1, 1 << 20}, {"gone_ticks", &LfOpts::gone_ticks, 0, 1 << 20}};
    if (launch_option(k, value, SC_TICKS_MAX)) return;
    const bool known = table_option(table, o, k, value, [&](const LfOpts& n) {
        AIC_REQUIRE(n.absorb_ticks > n.min_ticks, AIC_ERR_INVALID, k + ": absorb_ticks must exceed min_ticks");
        AIC_REQUIRE(n.max_cells >= n.min_cells, AIC_ERR_INVALID, k + ": max_cells must not be below min_cells");
    });
    AIC_REQUIRE(known, AIC_ERR_INVALID, "unknown left-objects option: " + k);
}

void Left::touch_device() {
    use_device();
    if (!d_scalars.p) {
        const size_t n = (size_t)g.streams * cells();
        hipStream_t st = dev->s_trk;
        grow(d_fast, n, "the cell model");
        grow(d_slow, n, "the cell model");
        grow(d_still, n, "the cell model");
        grow(d_last_id, n, "the cell model");
        grow(d_last_tick, n, "the cell model");
        grow(d_slots, (size_t)g.streams * max_objects * LF_OBJECT_INTS, "the object slots");
        grow(d_total, 1, "the event count");
        grow(d_scalars, (size_t)g.streams * LF_S_INTS, "the stream scalars");
        HIP_CHECK(hipMemsetAsync(d_fast.p, 0, d_fast.bytes(), st));
        HIP_CHECK(hipMemsetAsync(d_slow.p, 0, d_slow.bytes(), st));
        HIP_CHECK(hipMemsetAsync(d_still.p, 0, d_still.bytes(), st));
        HIP_CHECK(hipMemsetAsync(d_last_id.p, 0, d_last_id.bytes(), st));
        HIP_CHECK(hipMemsetAsync(d_last_tick.p, 0, d_last_tick.bytes(), st));
        HIP_CHECK(hipMemsetAsync(d_slots.p, 0, d_slots.bytes(), st));
        HIP_CHECK(hipMemsetAsync(d_scalars.p, 0, d_scalars.bytes(), st));
    }
}

void Left::update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap_events,
                  int32_t* records, int32_t* objects, int32_t* events, int32_t* n_events, int32_t* status, uint8_t* cand, int32_t* labels) {
    const int S = g.streams, M = max_objects;
    const long F = check_call(ticks, SC_TICKS_MAX, frames_mem, rows_mem);
    AIC_REQUIRE(cap_events >= 0 && cap_events <= (1 << 24), AIC_ERR_INVALID, "cap_events must be in 0..2^24");
    AIC_REQUIRE(n_events, AIC_ERR_INVALID, "NULL n_events");
    AIC_REQUIRE(cap_events == 0 || events, AIC_ERR_INVALID, "NULL events");
    AIC_REQUIRE(F == 0 || (frames && records && objects), AIC_ERR_INVALID, "NULL frames, records or objects");
    const bool with_rows = counts != nullptr && F > 0;
    const long total = count_rows(counts, with_rows, F, SC_ROWS_MAX, rows6, rows_mem, [&] {
        touch_device();
        *n_events = 0;
        if (status) *status = AIC_OK;
    }, [](long) {});
    if (F == 0) return;
    hipStream_t st = dev->s_trk;
    const BankStage bs = upload(F, with_rows ? counts : nullptr, total, rows6, with_rows && rows_mem == AIC_HOST);
    const int* d_rows = bs.d_rows(d_stage.p, rows6);
    const int* d_off = d_stage.p + bs.o_off;
    grow(d_events, std::max<size_t>(1, (size_t)cap_events * LF_EVENT_INTS), "the events");
    HIP_CHECK(hipMemsetAsync(d_total.p, 0, sizeof(int), st));

    const size_t tick_cells = cells() * S, cell_bytes = labels ? 20 : 16;
    {
        Prof pr(*dev, PROF_MISC, st, 0, (double)F * frame_bytes);
        const auto launch_bytes = [&](int lo, int hi) { return (size_t)(hi - lo) * tick_cells * cell_bytes; };
        launches(frames, frames_mem, ticks, launch_bytes, [&](int lo, int hi, const uint8_t* d_fr) {
            const int n = hi - lo, n_frames = n * S;
            const size_t nc = (size_t)n * tick_cells;
            grow(d_gray, nc, "the gray grids");
            grow(d_occ, nc, "the occupancy");
            grow(d_occ_id, nc, "the occupancy");
            grow(d_cand, nc, "the candidates");
            grow(d_slow8, nc, "the background grids");
            grow(d_own_tick, nc, "the owners");
            grow(d_own_id, nc, "the owners");
            if (labels) grow(d_labels, nc, "the labels");
            grow(d_head, (size_t)n_frames * LF_HEAD_INTS, "the blob tables");
            grow(d_blobs, (size_t)n_frames * LF_BLOBS_MAX * LF_BLOB_INTS, "the blob tables");
            grow(d_rec, (size_t)n_frames * LF_RECORD_INTS, "the records");
            grow(d_obj, (size_t)n_frames * M * LF_OBJECT_INTS, "the objects");
            grow(d_evc, (size_t)n_frames, "the events");
            grow(d_ev, (size_t)n_frames * 2 * M * LF_EVENT_INTS, "the events");
            const LfFrames fr{d_gray.p, d_occ.p, d_cand.p, d_slow8.p, d_occ_id.p, d_own_tick.p, d_own_id.p};
            const LfCells cs{d_fast.p, d_slow.p, d_still.p, d_last_id.p, d_last_tick.p};
            HIP_CHECK(hipMemsetAsync(d_occ.p, 0, nc, st));
            launch_scene_gray(d_fr, n_frames, g, d_gray.p, st);
            if (total) {
                const int max_rows = this->max_rows(counts, lo, hi);
                if (max_rows) HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_occ_id.p), LF_NONE, nc, st));
                launch_left_occupancy(d_off + (size_t)lo * S, n_frames, max_rows, d_rows, g, o.pad_cells, d_occ.p, d_occ_id.p, st);
            }
            launch_left_model(fr, n, g, o, d_scalars.p, d_stage.p, lo == 0, cs, st);
            launch_left_blobs(fr, n_frames, g, o, d_head.p, d_blobs.p, labels ? d_labels.p : nullptr, st);
            launch_left_walk(d_head.p, d_blobs.p, n, lo, g, o, M, d_stage.p, lo == 0, d_scalars.p, d_slots.p, d_rec.p, d_obj.p, d_evc.p, d_ev.p, st);
            launch_left_events(d_evc.p, d_ev.p, n_frames, M, cap_events, d_events.p, d_total.p, st);
            const size_t f0 = (size_t)lo * S;
            HIP_CHECK(hipMemcpyAsync(records + f0 * LF_RECORD_INTS, d_rec.p, (size_t)n_frames * LF_RECORD_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(objects + f0 * M * LF_OBJECT_INTS, d_obj.p, (size_t)n_frames * M * LF_OBJECT_INTS * sizeof(int),
                                     hipMemcpyDeviceToHost, st));
            if (cand) HIP_CHECK(hipMemcpyAsync(cand + (size_t)lo * tick_cells, d_cand.p, nc, hipMemcpyDeviceToHost, st));
            if (labels) HIP_CHECK(hipMemcpyAsync(labels + (size_t)lo * tick_cells, d_labels.p, nc * sizeof(int), hipMemcpyDeviceToHost, st));
        });
    }
    int n_ev = 0;
    HIP_CHECK(hipMemcpyAsync(&n_ev, d_total.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::fill(reset_pending.begin(), reset_pending.end(), (char)0);
    const int got = std::min(n_ev, cap_events);
    if (got) {
        HIP_CHECK(hipMemcpyAsync(events, d_events.p, (size_t)got * LF_EVENT_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    *n_events = n_ev;
    if (n_ev > cap_events) {                                                 // the state has advanced; only the list is cut
        if (status) *status = AIC_ERR_CAPACITY;
        else throw Error(AIC_ERR_CAPACITY, std::to_string(n_ev) + " events for a list of " + std::to_string(cap_events) + ": the first are delivered");
    }
}

void Left::export_stream(int stream, int32_t* fast, int32_t* slow, int32_t* still, int32_t* last_id, int32_t* last_tick, int32_t* slots,
                         int32_t* scalars) {
    AIC_REQUIRE(stream >= 0 && stream < g.streams, AIC_ERR_INVALID, "stream outside the bank");
    AIC_REQUIRE(fast && slow && still && last_id && last_tick && slots && scalars, AIC_ERR_INVALID, "NULL argument");
    const size_t n = cells(), ns = (size_t)max_objects * LF_OBJECT_INTS;
    for (int32_t* p : {fast, slow, still, last_id, last_tick}) std::fill(p, p + n, 0);
    std::fill(slots, slots + ns, 0), std::fill(scalars, scalars + LF_S_INTS, 0);
    if (!d_scalars.p || reset_pending[stream]) return;                       // nothing seen yet, or a reset the next call applies
    dev->use();
    hipStream_t st = dev->s_trk;
    std::vector<uint16_t> hf(n), hs(n), ht(n);
    HIP_CHECK(hipMemcpyAsync(hf.data(), d_fast.p + stream * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(hs.data(), d_slow.p + stream * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(ht.data(), d_still.p + stream * n, n * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(last_id, d_last_id.p + stream * n, n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(last_tick, d_last_tick.p + stream * n, n * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(slots, d_slots.p + stream * ns, ns * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(scalars, d_scalars.p + (size_t)stream * LF_S_INTS, LF_S_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::copy(hf.begin(), hf.end(), fast), std::copy(hs.begin(), hs.end(), slow), std::copy(ht.begin(), ht.end(), still);
    for (int j = 0; j < max_objects; ++j) {                                  // the slots hold cell boxes, x1 y1 inclusive: pixels, exclusive
        int32_t* sl = slots + (size_t)j * LF_OBJECT_INTS;
        if (sl[LF_O_UID] == 0) continue;
        sl[LF_O_X0] *= g.c, sl[LF_O_Y0] *= g.c, sl[LF_O_X1] = (sl[LF_O_X1] + 1) * g.c, sl[LF_O_Y1] = (sl[LF_O_Y1] + 1) * g.c;
    }
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_left_config_default(int streams, int frame_h, int frame_w, aic_left_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_left_config{streams, frame_h, frame_w, 8, 32};
    });
}

int aic_left_create(int device, const aic_left_config* config, aic_left** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        left_check_config(device, config);
        *out = new aic_left(device, *config);
    });
}

int aic_left_destroy(aic_left* s) { return destroy_handle(s, s ? s->s.dev : nullptr); }

int aic_left_option(aic_left* s, const char* key, int value) {
    return with_handle(s, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        s->s.option(key, value);
    });
}

int aic_left_reset(aic_left* s, int stream) {
    return with_handle(s, [&] { s->s.reset(stream); });
}

int aic_left_update(aic_left* s, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem,
                    int cap_events, int32_t* records, int32_t* objects, int32_t* events, int32_t* n_events, int32_t* status, uint8_t* cand,
                    int32_t* labels) {
    return with_handle(s, [&] {
        s->s.update(frames_bgr, frames_mem, ticks, counts, rows6, rows_mem, cap_events, records, objects, events, n_events, status, cand, labels);
    });
}

int aic_left_export(aic_left* s, int stream, int32_t* fast, int32_t* slow, int32_t* still, int32_t* last_id, int32_t* last_tick, int32_t* slots,
                    int32_t* scalars) {
    return with_handle(s, [&] { s->s.export_stream(stream, fast, slow, still, last_id, last_tick, slots, scalars); });
}

}  // extern "C"
