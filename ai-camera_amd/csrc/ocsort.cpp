// ocsort.cpp -- the OC-SORT tracker object (device table, epoch planning, launch, error check, read-back) and its C ABI.
// There is no host implementation of the algorithm: the recurrence runs in kernels_ocsort.hip or the call raises.
#include "ocsort_host.hpp"

#include <algorithm>
#include <cmath>

#include "kf7_math.hpp"

namespace aic {

// Parameter checks of aic_ocsort_create / aic_pipeline_create_ocsort: nothing is touched before they pass.
OcParams ocsort_params(const aic_ocsort_params& p, int* first_id) {
    auto unit = [](double x) { return x > 0.0 && x <= 1.0; };
    AIC_REQUIRE(unit(p.det_thresh) && unit(p.iou_threshold), AIC_ERR_INVALID, "det_thresh and iou_threshold must be in (0, 1]");
    AIC_REQUIRE(!p.use_byte || (float)p.det_thresh > 0.1f, AIC_ERR_INVALID, "use_byte needs det_thresh above the low band's floor 0.1");
    AIC_REQUIRE(p.inertia >= 0.0 && p.inertia <= 1.0, AIC_ERR_INVALID, "inertia must be in [0, 1]");
    AIC_REQUIRE(p.max_age >= 0 && p.min_hits >= 0, AIC_ERR_INVALID, "max_age and min_hits must be >= 0");
    AIC_REQUIRE(p.delta_t >= 1 && p.delta_t <= OC_DTMAX, AIC_ERR_INVALID, "delta_t must be in 1..8");
    AIC_REQUIRE(p.max_tracks >= 0 && p.max_tracks <= TRK_DEV_TMAX, AIC_ERR_INVALID, "max_tracks must be in 0..512 (0 = 512)");
    AIC_REQUIRE(p.first_track_id >= 0, AIC_ERR_INVALID, "first_track_id must be >= 0");
    OcParams o{};
    o.det_thresh = (float)p.det_thresh, o.iou_thresh = (float)p.iou_threshold, o.inertia = (float)p.inertia, o.low_thresh = 0.1f;
    o.max_age = p.max_age, o.min_hits = p.min_hits, o.delta_t = p.delta_t, o.use_byte = p.use_byte ? 1 : 0;
    o.cap = p.max_tracks ? p.max_tracks : TRK_DEV_TMAX;
    o.no_fast = 0;
    if (first_id) *first_id = p.first_track_id;
    return o;
}

OcSortTracker::OcSortTracker(Device& d, const OcParams& p, int first_id) : dev(&d), prm(p) {
    dev->use();
    const size_t bytes = oc_table_bytes(prm.cap);
    d_tbl.alloc(bytes);
    tbl = oc_table(d_tbl.p, prm.cap);
    HIP_CHECK(hipMemsetAsync(d_tbl.p, 0, bytes, dev->s_trk));
    OcHdr h{};
    h.next_id = first_id;
    HIP_CHECK(hipMemcpyAsync(tbl.hdr, &h, sizeof(h), hipMemcpyHostToDevice, dev->s_trk));
    d_ext.alloc((size_t)TRK_DEV_NMAX * TRK_DEV_TMAX);
    h_hdr.alloc(sizeof(OcHdr));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void OcSortTracker::run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) {
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "OC-SORT tracker stopped by an earlier error: " + fail_msg);
    const int kmax = epoch_frames > 0 ? epoch_frames : TRK_KMAX;
    OcParams p = prm;
    p.no_fast = lsap_fast ? 0 : 1;
    for (int f = 0; f < frames;) {
        const int k = std::min(kmax, frames - f);
        {
            Prof pr(*dev, PROF_TRK, s, 0, 0);
            launch_ocsort_epoch(tbl, p, dets, f, k, d_ext.p, out, s);
        }
        f += k;
    }
    HIP_CHECK(hipMemcpyAsync(h_hdr.p, tbl.hdr, sizeof(OcHdr), hipMemcpyDeviceToHost, s));
}

void OcSortTracker::check_epochs() {
    const OcHdr* h = reinterpret_cast<const OcHdr*>(h_hdr.p);
    if (h->err == 0) return;
    failed = true;
    const std::string at = " (frame " + std::to_string(h->err_frame) + " of the call)";
    if (h->err == 1) fail_msg = "track capacity exhausted (raise max_tracks)" + at;
    else if (h->err == 3) fail_msg = "more than 512 detections in one frame" + at;
    else fail_msg = "the assignment problem has no finite solution (a detection box that is not finite?)" + at;
    AIC_REQUIRE(false, AIC_ERR_CAPACITY, "OC-SORT: " + fail_msg);
}

void OcSortTracker::update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                                 int32_t* n_out, int32_t* out6, float* out_conf) {
    dev->use();
    AIC_REQUIRE(k >= 0 && cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "OC-SORT tracker stopped by an earlier error: " + fail_msg);
    if (k == 0) return;
    long total = 0;
    for (int f = 0; f < k; ++f) {
        AIC_REQUIRE(counts[f] >= 0, AIC_ERR_INVALID, "negative detection count");
        AIC_REQUIRE(counts[f] <= TRK_DEV_NMAX, AIC_ERR_CAPACITY, "OC-SORT: more than 512 detections in one frame");
        total += counts[f];
    }
    hipStream_t s = dev->s_trk;
    const int n = (int)total;
    // staging (host == device layout): frame_n[k] | frame_d0[k] | tlwh[n*4] | conf[n] | cls[n] || n_tracks[k] | rows[k*cap*6] | conf[k*cap]
    const size_t o_d0 = (size_t)k * 4, o_tlwh = (((size_t)k * 8 + 15) / 16) * 16, o_conf = o_tlwh + (size_t)n * 16, o_cls = o_conf + (size_t)n * 4;
    const size_t o_out = ((o_cls + (size_t)n * 4 + 15) / 16) * 16;
    const size_t o_rows = o_out + (((size_t)k * 4 + 15) / 16) * 16, o_oconf = o_rows + (size_t)k * cap_rows * 24;
    const size_t bytes = o_oconf + (size_t)k * cap_rows * 4;
    HIP_CHECK(hipStreamSynchronize(s));
    h_api.ensure(bytes);
    d_api.ensure(bytes);
    int* hn = reinterpret_cast<int*>(h_api.p);
    int* hd = reinterpret_cast<int*>(h_api.p + o_d0);
    int d0 = 0;
    for (int f = 0; f < k; ++f) { hn[f] = counts[f]; hd[f] = d0; d0 += counts[f]; }
    float* ht = reinterpret_cast<float*>(h_api.p + o_tlwh);
    for (int j = 0; j < n; ++j) {                                 // xyxy -> tlwh, fp32: the detection format of every tracker here
        const float* b = xyxy + (size_t)j * 4;
        ht[j * 4 + 0] = b[0], ht[j * 4 + 1] = b[1], ht[j * 4 + 2] = b[2] - b[0], ht[j * 4 + 3] = b[3] - b[1];
    }
    if (n) {
        std::memcpy(h_api.p + o_conf, conf, (size_t)n * 4);
        std::memcpy(h_api.p + o_cls, cls, (size_t)n * 4);
    }
    HIP_CHECK(hipMemcpyAsync(d_api.p, h_api.p, o_out, hipMemcpyHostToDevice, s));
    EpochDets dets{reinterpret_cast<const int*>(d_api.p), reinterpret_cast<const int*>(d_api.p + o_d0),
                   reinterpret_cast<const float*>(d_api.p + o_tlwh), reinterpret_cast<const float*>(d_api.p + o_conf),
                   reinterpret_cast<const int*>(d_api.p + o_cls), nullptr, nullptr, nullptr};
    EpochOut out{reinterpret_cast<int*>(d_api.p + o_out), reinterpret_cast<int*>(d_api.p + o_rows), reinterpret_cast<float*>(d_api.p + o_oconf),
                 cap_rows, nullptr, nullptr, 0};
    run_epochs(dets, k, out, s);
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

OcHdr OcSortTracker::header() {
    dev->use();
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    OcHdr h{};
    HIP_CHECK(hipMemcpy(&h, tbl.hdr, sizeof(h), hipMemcpyDeviceToHost));
    return h;
}

int OcSortTracker::export_state(int cap_rows, const OcExport& e) {
    dev->use();
    // after an error the covariances hold the failing epoch's values and the rest the epoch before: there is no state to report
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "OC-SORT tracker stopped by an earlier error (no consistent state to export): " + fail_msg);
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    std::vector<char> h(oc_table_bytes(prm.cap));
    HIP_CHECK(hipMemcpy(h.data(), d_tbl.p, h.size(), hipMemcpyDeviceToHost));
    const OcTable t = oc_table(h.data(), prm.cap);
    const int n = t.hdr->n_tracks;
    for (int i = 0; i < n && i < cap_rows; ++i) {
        const int sl = t.tl[i];
        const OcTrack& r = t.trk[sl];
        if (e.id) e.id[i] = r.id;
        if (e.age) e.age[i] = r.age;
        if (e.hits) e.hits[i] = r.hits;
        if (e.streak) e.streak[i] = r.streak;
        if (e.tsu) e.tsu[i] = r.tsu;
        if (e.cls) e.cls[i] = r.cls;
        if (e.frozen) e.frozen[i] = r.kstate == KF7_FROZEN;
        if (e.has_obs) e.has_obs[i] = r.has_obs;
        if (e.score) e.score[i] = r.score;
        if (e.last) std::copy(r.last, r.last + 4, e.last + (size_t)i * 4);
        if (e.vel) std::copy(r.vel, r.vel + 2, e.vel + (size_t)i * 2);
        if (e.mean) std::copy(t.mean + (size_t)sl * 8, t.mean + (size_t)sl * 8 + 7, e.mean + (size_t)i * 7);
        if (e.cov)
            for (int a = 0; a < 7; ++a) std::copy(t.cov + (size_t)sl * 64 + a * 8, t.cov + (size_t)sl * 64 + a * 8 + 7, e.cov + (size_t)i * 49 + a * 7);
    }
    return n;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_ocsort_create(int device_id, const aic_ocsort_params* p, aic_ocsort** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const OcParams o = ocsort_params(*p, &first);
        *out = new aic_ocsort(device(device_id), o, first);
    });
}

int aic_ocsort_destroy(aic_ocsort* t) {
    return guarded([&] { delete t; });
}

int aic_ocsort_option(aic_ocsort* t, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(t && key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        if (k == "lsap_fast") t->t.lsap_fast = value != 0;
        else if (k == "epoch_frames") {
            AIC_REQUIRE(value >= 0 && value <= TRK_KMAX, AIC_ERR_INVALID, "epoch_frames must be in 0..16 (0 = default)");
            t->t.epoch_frames = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown OC-SORT option: " + k);
    });
}

int aic_ocsort_update_batch(aic_ocsort* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf, const int32_t* cls,
                            int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf) {
    return guarded([&] {
        AIC_REQUIRE(t && (k == 0 || counts), AIC_ERR_INVALID, "NULL argument");
        long total = 0;
        for (int f = 0; f < k; ++f) total += counts[f];
        AIC_REQUIRE(total == 0 || (boxes_xyxy && conf && cls), AIC_ERR_INVALID, "NULL detection arrays");
        t->t.update_batch(k, counts, boxes_xyxy, conf, cls, cap_rows, n_out, out6, out_conf);
    });
}

int aic_ocsort_export(aic_ocsort* t, int cap, int32_t* track_id, int32_t* age, int32_t* hits, int32_t* hit_streak, int32_t* time_since_update,
                      int32_t* cls, int32_t* frozen, int32_t* has_obs, float* score, float* last_observation, float* velocity, float* mean,
                      float* cov, int32_t* n_tracks) {
    return guarded([&] {
        AIC_REQUIRE(t && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const OcExport e{track_id, age, hits, hit_streak, time_since_update, cls, frozen, has_obs, score, last_observation, velocity, mean, cov};
        const int n = t->t.export_state(cap, e);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_ocsort_counters(aic_ocsort* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_oru, int32_t* max_gap, int64_t* n_ocr,
                        int64_t* n_byte) {
    return guarded([&] {
        AIC_REQUIRE(t, AIC_ERR_INVALID, "NULL tracker");
        const OcHdr h = t->t.header();
        if (n_fast) *n_fast = h.n_fast;
        if (n_lsap) *n_lsap = h.n_lsap;
        if (max_side) *max_side = h.max_side;
        if (n_oru) *n_oru = h.n_oru;
        if (max_gap) *max_gap = h.max_gap;
        if (n_ocr) *n_ocr = h.n_ocr;
        if (n_byte) *n_byte = h.n_byte;
    });
}

}  // extern "C"
