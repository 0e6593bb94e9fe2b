// botsort.cpp -- the BoT-SORT tracker object (a bank of streams, epoch_bank.hpp: its kernel launch, the features it stages, error texts,
// export) and its C ABI.
// There is no host implementation of the algorithm: the recurrence runs in kernels_botsort.hip or the call raises.
#include "botsort_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace aic {

// Parameter checks of aic_botsort_create: nothing is touched before they pass.
BsParams botsort_params(const aic_botsort_params& p, int* first_id) {
    auto unit = [](double x) { return x > 0.0 && x <= 1.0; };
    AIC_REQUIRE(unit(p.track_high_thresh) && unit(p.track_low_thresh) && unit(p.match_thresh) && unit(p.new_track_thresh), AIC_ERR_INVALID,
                "track_high_thresh, track_low_thresh, new_track_thresh and match_thresh must be in (0, 1]");
    AIC_REQUIRE((float)p.track_low_thresh < (float)p.track_high_thresh, AIC_ERR_INVALID, "track_low_thresh must be below track_high_thresh");
    AIC_REQUIRE(unit(p.proximity_thresh) && unit(p.appearance_thresh), AIC_ERR_INVALID, "proximity_thresh and appearance_thresh must be in (0, 1]");
    AIC_REQUIRE(p.feat_alpha >= 0.0 && p.feat_alpha < 1.0, AIC_ERR_INVALID, "feat_alpha must be in [0, 1)");
    AIC_REQUIRE(p.track_buffer >= 0 && p.frame_rate > 0, AIC_ERR_INVALID, "track_buffer must be >= 0 and frame_rate > 0");
    AIC_REQUIRE(p.feature_dim >= 0 && p.feature_dim <= 4096 && p.feature_dim % 4 == 0, AIC_ERR_INVALID,
                "feature_dim must be a multiple of 4 in 0..4096 (0 = 512)");
    AIC_REQUIRE(p.max_tracks >= 0 && p.max_tracks <= TRK_DEV_TMAX, AIC_ERR_INVALID, "max_tracks must be in 0..512 (0 = 512)");
    AIC_REQUIRE(p.first_track_id >= 0, AIC_ERR_INVALID, "first_track_id must be >= 0");
    BsParams b{};
    b.high = (float)p.track_high_thresh, b.low = (float)p.track_low_thresh, b.new_thresh = (float)p.new_track_thresh;
    b.match_thresh = (float)p.match_thresh, b.proximity = (float)p.proximity_thresh, b.appearance = (float)p.appearance_thresh;
    b.second_thresh = 0.5f, b.unconf_thresh = 0.7f, b.dup_dist = 0.15f;
    b.alpha = (float)p.feat_alpha, b.one_minus_alpha = 1.0f - b.alpha;
    b.max_lost = (int)((double)p.frame_rate / 30.0 * (double)p.track_buffer);
    b.fuse = p.fuse_score ? 1 : 0, b.reid = p.with_reid ? 1 : 0;
    b.cap = p.max_tracks ? p.max_tracks : TRK_DEV_TMAX;
    b.dim = p.feature_dim ? p.feature_dim : 512;
    b.no_fast = 0;
    if (first_id) *first_id = p.first_track_id;
    return b;
}

BotSortTracker::BotSortTracker(Device& d, const BsParams& p, int first_id, int streams)
    : EpochBank(d, p, first_id, streams, bs_table_bytes(p.cap), (size_t)TRK_DEV_NMAX * TRK_DEV_NMAX), feat_stride((size_t)p.cap * p.dim) {
    d_feat.alloc(feat_stride * streams);
    HIP_CHECK(hipMemsetAsync(d_feat.p, 0, d_feat.bytes(), dev->s_trk));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void BotSortTracker::launch(const BsParams& p, const EpochCall& c, hipStream_t s) { launch_botsort_epoch(p, c, d_feat.p, feat_stride, warps, s); }

// the raw features of every row of the call -> unit rows, once, before the epochs; the call's camera motion -> the launches
void BotSortTracker::extra_staged(EpochDets& dets, const float* d_warps, float* d_feat_n, int rows, hipStream_t s) {
    if (dets.feat) {
        launch_botsort_normalize(dets.feat, d_feat_n, rows, prm.dim, s);
        dets.feat_n = d_feat_n;
    }
    warps = d_warps;
}

void BotSortTracker::reset_stream(int s) {
    EpochBank::reset_stream(s);                                   // the table, has_feat with it
    HIP_CHECK(hipMemsetAsync(d_feat.p + (size_t)s * feat_stride, 0, feat_stride * 4, dev->s_trk));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void BotSortTracker::update_bank(const int32_t* frames_per_stream, const int32_t* counts, const float* xyxy, const float* conf,
                                 const int32_t* cls, const float* feat, const int32_t* valid, const float* warps6, int cap_rows,
                                 int32_t* n_out, int32_t* out6, float* out_conf, int32_t* status) {
    // Every row's feature goes over (the band is decided on the device); a caller that wants to spare the 4 * dim bytes and the normalise of
    // a low-band row can mark it valid = 0, or hand over the high band only as the pipeline's filter does for s <= track_low_thresh.
    const BankExtra x{prm.reid ? feat : nullptr, valid, warps6, prm.dim};
    struct Clear { const float*& w; ~Clear() { w = nullptr; } } clear{warps};   // the staged warps are this call's
    update(frames_per_stream, counts, xyxy, conf, cls, cap_rows, n_out, out6, out_conf, status, &x);
}

void BotSortTracker::update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, const float* feat,
                                  const int32_t* valid, const float* warps6, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf) {
    AIC_REQUIRE(k >= 0 && cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "BoT-SORT tracker stopped by an earlier error: " + fail_msg);
    const int32_t fps = k;
    update_bank(&fps, counts, xyxy, conf, cls, feat, valid, warps6, cap_rows, n_out, out6, out_conf, nullptr);
}

void BotSortTracker::counters(int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_app, int64_t* cyc_cost,
                              int64_t* cyc_all) {
    const std::vector<char> hb = fetch_table(stream, sizeof(BsHdr));
    const BsHdr& h = *reinterpret_cast<const BsHdr*>(hb.data());
    if (n_fast) *n_fast = h.n_fast;
    if (n_lsap) *n_lsap = h.n_lsap;
    if (max_side) *max_side = h.max_side;
    if (n_app) *n_app = h.n_app;
    if (cyc_cost) *cyc_cost = h.cyc_cost;
    if (cyc_all) *cyc_all = h.cyc_all;
}

int BotSortTracker::export_state(int stream, int cap_rows, const ByteExport& e, int32_t* has_feat, float* smooth, int32_t* n_tracked) {
    AIC_REQUIRE(stream >= 0 && stream < n_streams, AIC_ERR_INVALID, "stream outside the bank");
    // after an error the covariances hold the failing epoch's values and the rest the epoch before: there is no state to report
    AIC_REQUIRE(!stop_code[stream], AIC_ERR_INVALID, "BoT-SORT tracker stopped by an earlier error (no consistent state to export): " + stop_msg[stream]);
    std::vector<char> h = fetch_table(stream, tbl_bytes);
    std::vector<float> hf;
    if (smooth) {
        hf.resize(feat_stride);
        HIP_CHECK(hipMemcpy(hf.data(), d_feat.p + (size_t)stream * feat_stride, hf.size() * 4, hipMemcpyDeviceToHost));
    }
    const BsTable t = bs_table(h.data(), prm.cap, hf.data());
    return byte_export(t, cap_rows, e, n_tracked, [&](int i, int sl) {
        if (has_feat) has_feat[i] = t.hasf[sl];
        if (smooth) {                                             // a slot without a feature may hold a former track's: report zeros
            float* o = smooth + (size_t)i * prm.dim;
            if (t.hasf[sl]) std::copy(t.feat + (size_t)sl * prm.dim, t.feat + (size_t)(sl + 1) * prm.dim, o);
            else std::fill(o, o + prm.dim, 0.f);
        }
    });
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_botsort_create(int device_id, const aic_botsort_params* p, aic_botsort** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const BsParams b = botsort_params(*p, &first);
        *out = new aic_botsort(device(device_id), b, first);
    });
}

int aic_botsort_destroy(aic_botsort* t) {
    return guarded([&] { delete t; });
}

int aic_botsort_option(aic_botsort* t, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(t && key, AIC_ERR_INVALID, "NULL argument");
        t->t.option(key, value);
    });
}

int aic_botsort_update_batch(aic_botsort* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf, const int32_t* cls,
                             const float* feat, const int32_t* valid, const float* warps, int cap_rows, int32_t* n_out, int32_t* out6,
                             float* out_conf) {
    return guarded([&] {
        AIC_REQUIRE(t && (k == 0 || counts), AIC_ERR_INVALID, "NULL argument");
        long total = 0;
        for (int f = 0; f < k; ++f) total += counts[f];
        AIC_REQUIRE(total == 0 || (boxes_xyxy && conf && cls), AIC_ERR_INVALID, "NULL detection arrays");
        t->t.update_batch(k, counts, boxes_xyxy, conf, cls, feat, valid, warps, cap_rows, n_out, out6, out_conf);
    });
}

int aic_botsort_export(aic_botsort* t, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated, int32_t* start_frame,
                       int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov, int32_t* has_feat, float* smooth_feat,
                       int32_t* n_tracks, int32_t* n_tracked) {
    return guarded([&] {
        AIC_REQUIRE(t && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const int n = t->t.export_state(0, cap, {track_id, state, is_activated, start_frame, end_frame, cls, score, mean, cov}, has_feat,
                                        smooth_feat, n_tracked);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_botsort_counters(aic_botsort* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_appearance, int64_t* cost_cycles,
                         int64_t* kernel_cycles) {
    return guarded([&] {
        AIC_REQUIRE(t, AIC_ERR_INVALID, "NULL tracker");
        t->t.counters(0, n_fast, n_lsap, max_side, n_appearance, cost_cycles, kernel_cycles);
    });
}

// ---- banks
int aic_botsort_bank_create(int device_id, const aic_botsort_params* p, int streams, aic_botsort_bank** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const BsParams b = botsort_params(*p, &first);
        AIC_REQUIRE(streams >= 1 && streams <= BANK_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
        *out = new aic_botsort_bank(device(device_id), b, first, streams);
    });
}

int aic_botsort_bank_destroy(aic_botsort_bank* b) {
    return guarded([&] { delete b; });
}

int aic_botsort_bank_option(aic_botsort_bank* b, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(b && key, AIC_ERR_INVALID, "NULL argument");
        b->t.option(key, value);
    });
}

int aic_botsort_bank_update(aic_botsort_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* boxes_xyxy,
                            const float* conf, const int32_t* cls, const float* feat, const int32_t* valid, const float* warps, int cap_rows,
                            int32_t* n_out, int32_t* out6, float* out_conf, int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(b && frames_per_stream, AIC_ERR_INVALID, "NULL argument");
        b->t.require_counts(frames_per_stream, counts);
        b->t.update_bank(frames_per_stream, counts, boxes_xyxy, conf, cls, feat, valid, warps, cap_rows, n_out, out6, out_conf, status);
    });
}

int aic_botsort_bank_reset(aic_botsort_bank* b, int stream) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.reset_stream(stream);
    });
}

int aic_botsort_bank_export(aic_botsort_bank* b, int stream, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated,
                            int32_t* start_frame, int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov, int32_t* has_feat,
                            float* smooth_feat, int32_t* n_tracks, int32_t* n_tracked) {
    return guarded([&] {
        AIC_REQUIRE(b && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const int n = b->t.export_state(stream, cap, {track_id, state, is_activated, start_frame, end_frame, cls, score, mean, cov}, has_feat,
                                        smooth_feat, n_tracked);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_botsort_bank_counters(aic_botsort_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_appearance,
                              int64_t* cost_cycles, int64_t* kernel_cycles) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.counters(stream, n_fast, n_lsap, max_side, n_appearance, cost_cycles, kernel_cycles);
    });
}

}  // extern "C"
