// bytetrack.cpp -- the ByteTrack tracker object (a bank of streams, epoch_bank.hpp: its kernel launch, error texts, export) and its C ABI.
// There is no host implementation of the algorithm: the recurrence runs in kernels_bytetrack.hip or the call raises.
#include "bytetrack_host.hpp"

#include <algorithm>
#include <cmath>

namespace aic {

// Parameter checks of aic_bytetrack_create / aic_pipeline_create_bytetrack: nothing is touched before they pass.
BtParams bytetrack_params(const aic_bytetrack_params& p, int* first_id) {
    auto unit = [](double x) { return x > 0.0 && x <= 1.0; };
    AIC_REQUIRE(unit(p.track_thresh) && unit(p.low_thresh) && unit(p.match_thresh), AIC_ERR_INVALID,
                "track_thresh, low_thresh and match_thresh must be in (0, 1]");
    AIC_REQUIRE((float)p.low_thresh < (float)p.track_thresh, AIC_ERR_INVALID, "low_thresh must be below track_thresh");
    AIC_REQUIRE(p.new_track_thresh >= 0.0 && std::isfinite(p.new_track_thresh), AIC_ERR_INVALID, "new_track_thresh must be >= 0 (0 = track_thresh + 0.1)");
    AIC_REQUIRE(p.track_buffer >= 0 && p.frame_rate > 0, AIC_ERR_INVALID, "track_buffer must be >= 0 and frame_rate > 0");
    AIC_REQUIRE(p.max_tracks >= 0 && p.max_tracks <= TRK_DEV_TMAX, AIC_ERR_INVALID, "max_tracks must be in 0..512 (0 = 512)");
    AIC_REQUIRE(p.first_track_id >= 0, AIC_ERR_INVALID, "first_track_id must be >= 0");
    BtParams b{};
    b.track_thresh = (float)p.track_thresh, b.low_thresh = (float)p.low_thresh, b.match_thresh = (float)p.match_thresh;
    b.new_thresh = (float)(p.new_track_thresh > 0.0 ? p.new_track_thresh : p.track_thresh + 0.1);   // byte_tracker.py: det_thresh
    b.second_thresh = 0.5f, b.unconf_thresh = 0.7f, b.dup_dist = 0.15f;
    b.max_lost = (int)((double)p.frame_rate / 30.0 * (double)p.track_buffer);                       // byte_tracker.py: max_time_lost
    b.fuse = p.fuse_score ? 1 : 0;
    b.cap = p.max_tracks ? p.max_tracks : TRK_DEV_TMAX;
    b.no_fast = 0;
    if (first_id) *first_id = p.first_track_id;
    return b;
}

ByteTracker::ByteTracker(Device& d, const BtParams& p, int first_id, int streams)
    : EpochBank(d, p, first_id, streams, bt_table_bytes(p.cap), (size_t)TRK_DEV_NMAX * TRK_DEV_NMAX) {}

void ByteTracker::launch(const BtParams& p, const EpochCall& c, hipStream_t s) { launch_bytetrack_epoch(p, c, s); }

std::string byte_err_text(int err) {
    if (err == 1) return "track capacity exhausted (raise max_tracks)";
    if (err == 3) return "an assignment problem beyond the epoch kernel's capacity (tracks + detections > 512, or > 512 detections in a frame)";
    return "the assignment problem has no finite solution";
}

void ByteTracker::update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                               int32_t* n_out, int32_t* out6, float* out_conf) {
    AIC_REQUIRE(k >= 0 && cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "ByteTrack tracker stopped by an earlier error: " + fail_msg);
    const int32_t fps = k;
    update(&fps, counts, xyxy, conf, cls, cap_rows, n_out, out6, out_conf, nullptr);
}

void ByteTracker::counters(int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side) {
    const std::vector<char> hb = fetch_table(stream, sizeof(BtHdr));
    const BtHdr& h = *reinterpret_cast<const BtHdr*>(hb.data());
    if (n_fast) *n_fast = h.n_fast;
    if (n_lsap) *n_lsap = h.n_lsap;
    if (max_side) *max_side = h.max_side;
}

int ByteTracker::export_state(int stream, int cap_rows, const ByteExport& e, int32_t* n_tracked) {
    AIC_REQUIRE(stream >= 0 && stream < n_streams, AIC_ERR_INVALID, "stream outside the bank");
    // after an error the covariances hold the failing epoch's values and the rest the epoch before: there is no state to report
    AIC_REQUIRE(!stop_code[stream], AIC_ERR_INVALID, "ByteTrack tracker stopped by an earlier error (no consistent state to export): " + stop_msg[stream]);
    std::vector<char> h = fetch_table(stream, tbl_bytes);
    return byte_export(bt_table(h.data(), prm.cap), cap_rows, e, n_tracked, [](int, int) {});
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_bytetrack_create(int device_id, const aic_bytetrack_params* p, aic_bytetrack** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const BtParams b = bytetrack_params(*p, &first);
        *out = new aic_bytetrack(device(device_id), b, first);
    });
}

int aic_bytetrack_destroy(aic_bytetrack* t) {
    return guarded([&] { delete t; });
}

int aic_bytetrack_option(aic_bytetrack* t, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(t && key, AIC_ERR_INVALID, "NULL argument");
        t->t.option(key, value);
    });
}

int aic_bytetrack_update_batch(aic_bytetrack* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf, const int32_t* cls,
                               int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf) {
    return guarded([&] {
        AIC_REQUIRE(t && (k <= 0 || counts), AIC_ERR_INVALID, "NULL argument");
        t->t.update_batch(k, counts, boxes_xyxy, conf, cls, cap_rows, n_out, out6, out_conf);
    });
}

int aic_bytetrack_export(aic_bytetrack* t, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated, int32_t* start_frame,
                         int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov, int32_t* n_tracks, int32_t* n_tracked) {
    return guarded([&] {
        AIC_REQUIRE(t && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const int n = t->t.export_state(0, cap, {track_id, state, is_activated, start_frame, end_frame, cls, score, mean, cov}, n_tracked);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_bytetrack_counters(aic_bytetrack* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side) {
    return guarded([&] {
        AIC_REQUIRE(t, AIC_ERR_INVALID, "NULL tracker");
        t->t.counters(0, n_fast, n_lsap, max_side);
    });
}

// ---- banks
int aic_bytetrack_bank_create(int device_id, const aic_bytetrack_params* p, int streams, aic_bytetrack_bank** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const BtParams b = bytetrack_params(*p, &first);
        AIC_REQUIRE(streams >= 1 && streams <= BANK_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
        *out = new aic_bytetrack_bank(device(device_id), b, first, streams);
    });
}

int aic_bytetrack_bank_destroy(aic_bytetrack_bank* b) {
    return guarded([&] { delete b; });
}

int aic_bytetrack_bank_option(aic_bytetrack_bank* b, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(b && key, AIC_ERR_INVALID, "NULL argument");
        b->t.option(key, value);
    });
}

int aic_bytetrack_bank_update(aic_bytetrack_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* boxes_xyxy,
                              const float* conf, const int32_t* cls, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf,
                              int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(b && frames_per_stream, AIC_ERR_INVALID, "NULL argument");
        b->t.require_counts(frames_per_stream, counts);
        b->t.update(frames_per_stream, counts, boxes_xyxy, conf, cls, cap_rows, n_out, out6, out_conf, status);
    });
}

int aic_bytetrack_bank_reset(aic_bytetrack_bank* b, int stream) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.reset_stream(stream);
    });
}

int aic_bytetrack_bank_export(aic_bytetrack_bank* b, int stream, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated,
                              int32_t* start_frame, int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov,
                              int32_t* n_tracks, int32_t* n_tracked) {
    return guarded([&] {
        AIC_REQUIRE(b && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const int n = b->t.export_state(stream, cap, {track_id, state, is_activated, start_frame, end_frame, cls, score, mean, cov}, n_tracked);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_bytetrack_bank_counters(aic_bytetrack_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.counters(stream, n_fast, n_lsap, max_side);
    });
}

}  // extern "C"
