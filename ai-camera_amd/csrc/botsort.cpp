// botsort.cpp -- the BoT-SORT tracker object (device table, epoch planning, launch, error check, read-back) and its C ABI.
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

BotSortTracker::BotSortTracker(Device& d, const BsParams& p, int first_id) : dev(&d), prm(p) {
    dev->use();
    const size_t bytes = bs_table_bytes(prm.cap);
    d_tbl.alloc(bytes);
    d_feat.alloc((size_t)prm.cap * prm.dim);
    tbl = bs_table(d_tbl.p, prm.cap, d_feat.p);
    HIP_CHECK(hipMemsetAsync(d_tbl.p, 0, bytes, dev->s_trk));
    HIP_CHECK(hipMemsetAsync(d_feat.p, 0, d_feat.bytes(), dev->s_trk));
    BsHdr h{};
    h.next_id = first_id;
    HIP_CHECK(hipMemcpyAsync(tbl.hdr, &h, sizeof(h), hipMemcpyHostToDevice, dev->s_trk));
    d_ext.alloc((size_t)TRK_DEV_NMAX * TRK_DEV_NMAX);
    h_hdr.alloc(sizeof(BsHdr));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void BotSortTracker::run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) {
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "BoT-SORT tracker stopped by an earlier error: " + fail_msg);
    const int kmax = epoch_frames > 0 ? epoch_frames : TRK_KMAX;
    BsParams p = prm;
    p.no_fast = lsap_fast ? 0 : 1;
    for (int f = 0; f < frames;) {
        const int k = std::min(kmax, frames - f);
        {
            Prof pr(*dev, PROF_TRK, s, 0, 0);
            launch_botsort_epoch(tbl, p, dets, warps, f, k, d_ext.p, out, s);
        }
        f += k;
    }
    HIP_CHECK(hipMemcpyAsync(h_hdr.p, tbl.hdr, sizeof(BsHdr), hipMemcpyDeviceToHost, s));
}

void BotSortTracker::check_epochs() {
    const BsHdr* h = reinterpret_cast<const BsHdr*>(h_hdr.p);
    if (h->err == 0) return;
    failed = true;
    const std::string at = " (frame " + std::to_string(h->err_frame) + " of the call)";
    if (h->err == 1) fail_msg = "track capacity exhausted (raise max_tracks)" + at;
    else if (h->err == 3) fail_msg = "an assignment problem beyond the epoch kernel's capacity (tracks + detections > 512, or > 512 detections in a frame)" + at;
    else fail_msg = "the assignment problem has no finite solution" + at;
    AIC_REQUIRE(false, AIC_ERR_CAPACITY, "BoT-SORT: " + fail_msg);
}

void BotSortTracker::update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, const float* feat,
                                  const int32_t* valid, const float* warps6, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf) {
    dev->use();
    AIC_REQUIRE(k >= 0 && cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "BoT-SORT tracker stopped by an earlier error: " + fail_msg);
    if (k == 0) return;
    long total = 0;
    for (int f = 0; f < k; ++f) {
        AIC_REQUIRE(counts[f] >= 0, AIC_ERR_INVALID, "negative detection count");
        AIC_REQUIRE(counts[f] <= TRK_DEV_NMAX, AIC_ERR_CAPACITY, "BoT-SORT: more than 512 detections in one frame");
        total += counts[f];
    }
    hipStream_t s = dev->s_trk;
    const int n = (int)total;
    const bool has_feat = feat != nullptr && prm.reid && n > 0;
    auto up = [](size_t x) { return (x + 15) / 16 * 16; };
    // Every row's feature goes over (the band is decided on the device); a caller that wants to spare the 4 * dim bytes and the normalise of
    // a low-band row can mark it valid = 0, or hand over the high band only as the pipeline's filter does for s <= track_low_thresh.
    // staging (host == device layout): frame_n[k] | frame_d0[k] | warps[k*6] | tlwh[n*4] | conf[n] | cls[n] | valid[n] | feat[n*dim] ||
    //                                  n_tracks[k] | rows[k*cap*6] | conf[k*cap]        and, device only, feat_n[n*dim] behind them
    const size_t o_d0 = (size_t)k * 4, o_warp = up((size_t)k * 8), o_tlwh = up(o_warp + (size_t)k * 24), o_conf = o_tlwh + (size_t)n * 16;
    const size_t o_cls = o_conf + (size_t)n * 4, o_valid = o_cls + (size_t)n * 4, o_feat = up(o_valid + (size_t)n * 4);
    const size_t o_out = up(o_feat + (has_feat ? (size_t)n * prm.dim * 4 : 0));
    const size_t o_rows = o_out + up((size_t)k * 4), o_oconf = o_rows + (size_t)k * cap_rows * 24;
    const size_t bytes = up(o_oconf + (size_t)k * cap_rows * 4);
    const size_t o_featn = bytes, dbytes = bytes + (has_feat ? (size_t)n * prm.dim * 4 : 0);
    HIP_CHECK(hipStreamSynchronize(s));
    h_api.ensure(bytes);
    d_api.ensure(dbytes);
    int* hn = reinterpret_cast<int*>(h_api.p);
    int* hd = reinterpret_cast<int*>(h_api.p + o_d0);
    int d0 = 0;
    for (int f = 0; f < k; ++f) { hn[f] = counts[f]; hd[f] = d0; d0 += counts[f]; }
    if (warps6) std::memcpy(h_api.p + o_warp, warps6, (size_t)k * 24);
    float* ht = reinterpret_cast<float*>(h_api.p + o_tlwh);
    for (int j = 0; j < n; ++j) {                                 // tlbr -> tlwh, fp32
        const float* b = xyxy + (size_t)j * 4;
        ht[j * 4 + 0] = b[0], ht[j * 4 + 1] = b[1], ht[j * 4 + 2] = b[2] - b[0], ht[j * 4 + 3] = b[3] - b[1];
    }
    if (n) {
        std::memcpy(h_api.p + o_conf, conf, (size_t)n * 4);
        std::memcpy(h_api.p + o_cls, cls, (size_t)n * 4);
        if (valid) std::memcpy(h_api.p + o_valid, valid, (size_t)n * 4);
        if (has_feat) std::memcpy(h_api.p + o_feat, feat, (size_t)n * prm.dim * 4);
    }
    HIP_CHECK(hipMemcpyAsync(d_api.p, h_api.p, o_out, hipMemcpyHostToDevice, s));
    const float* d_featn = nullptr;
    if (has_feat) {
        launch_botsort_normalize(reinterpret_cast<const float*>(d_api.p + o_feat), reinterpret_cast<float*>(d_api.p + o_featn), n, prm.dim, s);
        d_featn = reinterpret_cast<const float*>(d_api.p + o_featn);
    }
    EpochDets dets{reinterpret_cast<const int*>(d_api.p), reinterpret_cast<const int*>(d_api.p + o_d0),
                   reinterpret_cast<const float*>(d_api.p + o_tlwh), reinterpret_cast<const float*>(d_api.p + o_conf),
                   reinterpret_cast<const int*>(d_api.p + o_cls), valid ? reinterpret_cast<const int*>(d_api.p + o_valid) : nullptr,
                   has_feat ? reinterpret_cast<const float*>(d_api.p + o_feat) : nullptr, d_featn};
    EpochOut out{reinterpret_cast<int*>(d_api.p + o_out), reinterpret_cast<int*>(d_api.p + o_rows), reinterpret_cast<float*>(d_api.p + o_oconf),
                 cap_rows, nullptr, nullptr, 0};
    warps = warps6 ? reinterpret_cast<const float*>(d_api.p + o_warp) : nullptr;
    run_epochs(dets, k, out, s);
    warps = nullptr;
    HIP_CHECK(hipMemcpyAsync(h_api.p + o_out, d_api.p + o_out, bytes - o_out, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    check_epochs();
    const int* on = reinterpret_cast<const int*>(h_api.p + o_out);
    const int* rows = reinterpret_cast<const int*>(h_api.p + o_rows);
    const float* oc = reinterpret_cast<const float*>(h_api.p + o_oconf);
    for (int f = 0; f < k; ++f) {
        const int kk = std::min(on[f], cap_rows);
        if (n_out) n_out[f] = on[f];                              // the true count: rows beyond cap_rows are not stored
        if (out6) std::copy(rows + (size_t)f * cap_rows * 6, rows + ((size_t)f * cap_rows + kk) * 6, out6 + (size_t)f * cap_rows * 6);
        if (out_conf) std::copy(oc + (size_t)f * cap_rows, oc + (size_t)f * cap_rows + kk, out_conf + (size_t)f * cap_rows);
    }
}

void BotSortTracker::counters(int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_app, int64_t* cyc_cost, int64_t* cyc_all) {
    dev->use();
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    BsHdr h{};
    HIP_CHECK(hipMemcpy(&h, tbl.hdr, sizeof(h), hipMemcpyDeviceToHost));
    if (n_fast) *n_fast = h.n_fast;
    if (n_lsap) *n_lsap = h.n_lsap;
    if (max_side) *max_side = h.max_side;
    if (n_app) *n_app = h.n_app;
    if (cyc_cost) *cyc_cost = h.cyc_cost;
    if (cyc_all) *cyc_all = h.cyc_all;
}

int BotSortTracker::export_state(int cap_rows, int32_t* id, int32_t* state, int32_t* act, int32_t* start, int32_t* end, int32_t* cls,
                                 float* score, float* mean, float* cov, int32_t* has_feat, float* smooth, int32_t* n_tracked) {
    dev->use();
    // after an error the covariances hold the failing epoch's values and the rest the epoch before: there is no state to report
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "BoT-SORT tracker stopped by an earlier error (no consistent state to export): " + fail_msg);
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    std::vector<char> h(bs_table_bytes(prm.cap));
    HIP_CHECK(hipMemcpy(h.data(), d_tbl.p, h.size(), hipMemcpyDeviceToHost));
    std::vector<float> hf;
    if (smooth) {
        hf.resize((size_t)prm.cap * prm.dim);
        HIP_CHECK(hipMemcpy(hf.data(), d_feat.p, hf.size() * 4, hipMemcpyDeviceToHost));
    }
    const BsTable t = bs_table(h.data(), prm.cap, hf.data());
    const int ntl = t.hdr->n_tracked, nll = t.hdr->n_lost, n = ntl + nll;
    if (n_tracked) *n_tracked = ntl;
    for (int i = 0; i < n && i < cap_rows; ++i) {
        const int sl = i < ntl ? t.tl[i] : t.ll[i - ntl];
        const BtTrack& r = t.trk[sl];
        if (id) id[i] = r.id;
        if (state) state[i] = r.state;
        if (act) act[i] = r.act;
        if (start) start[i] = r.start;
        if (end) end[i] = r.end;
        if (cls) cls[i] = r.cls;
        if (score) score[i] = r.score;
        if (mean) std::copy(t.mean + (size_t)sl * 8, t.mean + (size_t)sl * 8 + 8, mean + (size_t)i * 8);
        if (cov) std::copy(t.cov + (size_t)sl * 64, t.cov + (size_t)sl * 64 + 64, cov + (size_t)i * 64);
        if (has_feat) has_feat[i] = t.hasf[sl];
        if (smooth) {                                             // a slot without a feature may hold a former track's: report zeros
            float* o = smooth + (size_t)i * prm.dim;
            if (t.hasf[sl]) std::copy(t.feat + (size_t)sl * prm.dim, t.feat + (size_t)(sl + 1) * prm.dim, o);
            else std::fill(o, o + prm.dim, 0.f);
        }
    }
    return n;
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
        const std::string k(key);
        if (k == "lsap_fast") t->t.lsap_fast = value != 0;
        else if (k == "epoch_frames") {
            AIC_REQUIRE(value >= 0 && value <= TRK_KMAX, AIC_ERR_INVALID, "epoch_frames must be in 0..16 (0 = default)");
            t->t.epoch_frames = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown BoT-SORT option: " + k);
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
        const int n = t->t.export_state(cap, track_id, state, is_activated, start_frame, end_frame, cls, score, mean, cov, has_feat,
                                        smooth_feat, n_tracked);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_botsort_counters(aic_botsort* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_appearance, int64_t* cost_cycles,
                         int64_t* kernel_cycles) {
    return guarded([&] {
        AIC_REQUIRE(t, AIC_ERR_INVALID, "NULL tracker");
        t->t.counters(n_fast, n_lsap, max_side, n_appearance, cost_cycles, kernel_cycles);
    });
}

}  // extern "C"
