// ocsort.cpp -- the OC-SORT tracker object (a bank of streams, epoch_bank.hpp: its kernel launch, error texts, export) and its C ABI.
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

OcSortTracker::OcSortTracker(Device& d, const OcParams& p, int first_id, int streams)
    : EpochBank(d, p, first_id, streams, oc_table_bytes(p.cap), (size_t)TRK_DEV_NMAX * TRK_DEV_TMAX) {}

void OcSortTracker::launch(const OcParams& p, const EpochCall& c, hipStream_t s) { launch_ocsort_epoch(p, c, s); }

std::string OcSortTracker::err_text(int err) const {
    if (err == 1) return "track capacity exhausted (raise max_tracks)";
    if (err == 3) return "more than 512 detections in one frame";
    return "the assignment problem has no finite solution (a detection box that is not finite?)";
}

void OcSortTracker::update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                                 int32_t* n_out, int32_t* out6, float* out_conf) {
    AIC_REQUIRE(k >= 0 && cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "OC-SORT tracker stopped by an earlier error: " + fail_msg);
    const int32_t fps = k;
    update(&fps, counts, xyxy, conf, cls, cap_rows, n_out, out6, out_conf, nullptr);
}

OcHdr OcSortTracker::header(int stream) {
    const std::vector<char> hb = fetch_table(stream, sizeof(OcHdr));
    return *reinterpret_cast<const OcHdr*>(hb.data());
}

int OcSortTracker::export_state(int stream, int cap_rows, const OcExport& e) {
    AIC_REQUIRE(stream >= 0 && stream < n_streams, AIC_ERR_INVALID, "stream outside the bank");
    // after an error the covariances hold the failing epoch's values and the rest the epoch before: there is no state to report
    AIC_REQUIRE(!stop_code[stream], AIC_ERR_INVALID, "OC-SORT tracker stopped by an earlier error (no consistent state to export): " + stop_msg[stream]);
    std::vector<char> h = fetch_table(stream, tbl_bytes);
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
        t->t.option(key, value);
    });
}

int aic_ocsort_update_batch(aic_ocsort* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf, const int32_t* cls,
                            int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf) {
    return guarded([&] {
        AIC_REQUIRE(t && (k <= 0 || counts), AIC_ERR_INVALID, "NULL argument");
        t->t.update_batch(k, counts, boxes_xyxy, conf, cls, cap_rows, n_out, out6, out_conf);
    });
}

int aic_ocsort_export(aic_ocsort* t, int cap, int32_t* track_id, int32_t* age, int32_t* hits, int32_t* hit_streak, int32_t* time_since_update,
                      int32_t* cls, int32_t* frozen, int32_t* has_obs, float* score, float* last_observation, float* velocity, float* mean,
                      float* cov, int32_t* n_tracks) {
    return guarded([&] {
        AIC_REQUIRE(t && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const OcExport e{track_id, age, hits, hit_streak, time_since_update, cls, frozen, has_obs, score, last_observation, velocity, mean, cov};
        const int n = t->t.export_state(0, cap, e);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_ocsort_counters(aic_ocsort* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_oru, int32_t* max_gap, int64_t* n_ocr,
                        int64_t* n_byte) {
    return guarded([&] {
        AIC_REQUIRE(t, AIC_ERR_INVALID, "NULL tracker");
        const OcHdr h = t->t.header(0);
        if (n_fast) *n_fast = h.n_fast;
        if (n_lsap) *n_lsap = h.n_lsap;
        if (max_side) *max_side = h.max_side;
        if (n_oru) *n_oru = h.n_oru;
        if (max_gap) *max_gap = h.max_gap;
        if (n_ocr) *n_ocr = h.n_ocr;
        if (n_byte) *n_byte = h.n_byte;
    });
}

// ---- banks
int aic_ocsort_bank_create(int device_id, const aic_ocsort_params* p, int streams, aic_ocsort_bank** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const OcParams o = ocsort_params(*p, &first);
        AIC_REQUIRE(streams >= 1 && streams <= BANK_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
        *out = new aic_ocsort_bank(device(device_id), o, first, streams);
    });
}

int aic_ocsort_bank_destroy(aic_ocsort_bank* b) {
    return guarded([&] { delete b; });
}

int aic_ocsort_bank_option(aic_ocsort_bank* b, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(b && key, AIC_ERR_INVALID, "NULL argument");
        b->t.option(key, value);
    });
}

int aic_ocsort_bank_update(aic_ocsort_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* boxes_xyxy,
                           const float* conf, const int32_t* cls, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf,
                           int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(b && frames_per_stream, AIC_ERR_INVALID, "NULL argument");
        b->t.require_counts(frames_per_stream, counts);
        b->t.update(frames_per_stream, counts, boxes_xyxy, conf, cls, cap_rows, n_out, out6, out_conf, status);
    });
}

int aic_ocsort_bank_reset(aic_ocsort_bank* b, int stream) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.reset_stream(stream);
    });
}

int aic_ocsort_bank_export(aic_ocsort_bank* b, int stream, int cap, int32_t* track_id, int32_t* age, int32_t* hits, int32_t* hit_streak,
                           int32_t* time_since_update, int32_t* cls, int32_t* frozen, int32_t* has_obs, float* score, float* last_observation,
                           float* velocity, float* mean, float* cov, int32_t* n_tracks) {
    return guarded([&] {
        AIC_REQUIRE(b && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const OcExport e{track_id, age, hits, hit_streak, time_since_update, cls, frozen, has_obs, score, last_observation, velocity, mean, cov};
        const int n = b->t.export_state(stream, cap, e);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_ocsort_bank_counters(aic_ocsort_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_oru,
                             int32_t* max_gap, int64_t* n_ocr, int64_t* n_byte) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        const OcHdr h = b->t.header(stream);
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
