// bytetrack.cpp -- the ByteTrack tracker object (device table, epoch planning, launch, error check, read-back) and its C ABI.
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

ByteTracker::ByteTracker(Device& d, const BtParams& p, int first_id) : dev(&d), prm(p) {
    dev->use();
    const size_t bytes = bt_table_bytes(prm.cap);
    d_tbl.alloc(bytes);
    tbl = bt_table(d_tbl.p, prm.cap);
    HIP_CHECK(hipMemsetAsync(d_tbl.p, 0, bytes, dev->s_trk));
    BtHdr h{};
    h.next_id = first_id;
    HIP_CHECK(hipMemcpyAsync(tbl.hdr, &h, sizeof(h), hipMemcpyHostToDevice, dev->s_trk));
    d_ext.alloc((size_t)TRK_DEV_NMAX * TRK_DEV_NMAX);
    h_hdr.alloc(sizeof(BtHdr));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void ByteTracker::run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) {
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "ByteTrack tracker stopped by an earlier error: " + fail_msg);
    const int kmax = epoch_frames > 0 ? epoch_frames : TRK_KMAX;
    BtParams p = prm;
    p.no_fast = lsap_fast ? 0 : 1;
    for (int f = 0; f < frames;) {
        const int k = std::min(kmax, frames - f);
        {
            Prof pr(*dev, PROF_TRK, s, 0, 0);
            launch_bytetrack_epoch(tbl, p, dets, f, k, d_ext.p, out, s);
        }
        f += k;
    }
    HIP_CHECK(hipMemcpyAsync(h_hdr.p, tbl.hdr, sizeof(BtHdr), hipMemcpyDeviceToHost, s));
}

void ByteTracker::check_epochs() {
    const BtHdr* h = reinterpret_cast<const BtHdr*>(h_hdr.p);
    if (h->err == 0) return;
    failed = true;
    const std::string at = " (frame " + std::to_string(h->err_frame) + " of the call)";
    if (h->err == 1) fail_msg = "track capacity exhausted (raise max_tracks)" + at;
    else if (h->err == 3) fail_msg = "an assignment problem beyond the epoch kernel's capacity (tracks + detections > 512, or > 512 detections in a frame)" + at;
    else fail_msg = "the assignment problem has no finite solution" + at;
    AIC_REQUIRE(false, AIC_ERR_CAPACITY, "ByteTrack: " + fail_msg);
}

void ByteTracker::update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                               int32_t* n_out, int32_t* out6, float* out_conf) {
    dev->use();
    AIC_REQUIRE(k >= 0 && cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "ByteTrack tracker stopped by an earlier error: " + fail_msg);
    if (k == 0) return;
    long total = 0;
    for (int f = 0; f < k; ++f) {
        AIC_REQUIRE(counts[f] >= 0, AIC_ERR_INVALID, "negative detection count");
        AIC_REQUIRE(counts[f] <= TRK_DEV_NMAX, AIC_ERR_CAPACITY, "ByteTrack: more than 512 detections in one frame");
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
    for (int j = 0; j < n; ++j) {                                 // tlbr -> tlwh (byte_tracker.py: STrack.tlbr_to_tlwh), fp32
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

void ByteTracker::counters(int64_t* n_fast, int64_t* n_lsap, int32_t* max_side) {
    dev->use();
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    BtHdr h{};
    HIP_CHECK(hipMemcpy(&h, tbl.hdr, sizeof(h), hipMemcpyDeviceToHost));
    if (n_fast) *n_fast = h.n_fast;
    if (n_lsap) *n_lsap = h.n_lsap;
    if (max_side) *max_side = h.max_side;
}

int ByteTracker::export_state(int cap_rows, int32_t* id, int32_t* state, int32_t* act, int32_t* start, int32_t* end, int32_t* cls,
                              float* score, float* mean, float* cov, int32_t* n_tracked) {
    dev->use();
    // after an error the covariances hold the failing epoch's values and the rest the epoch before: there is no state to report
    AIC_REQUIRE(!failed, AIC_ERR_INVALID, "ByteTrack tracker stopped by an earlier error (no consistent state to export): " + fail_msg);
    hipStream_t s = dev->s_trk;
    HIP_CHECK(hipStreamSynchronize(s));
    std::vector<char> h(bt_table_bytes(prm.cap));
    HIP_CHECK(hipMemcpy(h.data(), d_tbl.p, h.size(), hipMemcpyDeviceToHost));
    const BtTable t = bt_table(h.data(), prm.cap);
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
    }
    return n;
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
        const std::string k(key);
        if (k == "lsap_fast") t->t.lsap_fast = value != 0;
        else if (k == "epoch_frames") {
            AIC_REQUIRE(value >= 0 && value <= TRK_KMAX, AIC_ERR_INVALID, "epoch_frames must be in 0..16 (0 = default)");
            t->t.epoch_frames = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown ByteTrack option: " + k);
    });
}

int aic_bytetrack_update_batch(aic_bytetrack* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf, const int32_t* cls,
                               int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf) {
    return guarded([&] {
        AIC_REQUIRE(t && (k == 0 || counts), AIC_ERR_INVALID, "NULL argument");
        long total = 0;
        for (int f = 0; f < k; ++f) total += counts[f];
        AIC_REQUIRE(total == 0 || (boxes_xyxy && conf && cls), AIC_ERR_INVALID, "NULL detection arrays");
        t->t.update_batch(k, counts, boxes_xyxy, conf, cls, cap_rows, n_out, out6, out_conf);
    });
}

int aic_bytetrack_export(aic_bytetrack* t, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated, int32_t* start_frame,
                         int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov, int32_t* n_tracks, int32_t* n_tracked) {
    return guarded([&] {
        AIC_REQUIRE(t && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const int n = t->t.export_state(cap, track_id, state, is_activated, start_frame, end_frame, cls, score, mean, cov, n_tracked);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_bytetrack_counters(aic_bytetrack* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side) {
    return guarded([&] {
        AIC_REQUIRE(t, AIC_ERR_INVALID, "NULL tracker");
        t->t.counters(n_fast, n_lsap, max_side);
    });
}

}  // extern "C"
