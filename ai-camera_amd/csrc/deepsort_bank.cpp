// deepsort_bank.cpp -- the DeepSORT bank object (deepsort_bank.hpp) and its C ABI.  There is no host implementation behind it: the
// recurrence runs in kernels_trk_dev.hip or the call raises.
#include "deepsort_bank.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace aic {

TrkDevParams deepsort_bank_params(const aic_tracker_params& p, int streams, int* first_id) {
    AIC_REQUIRE(streams >= 1 && streams <= DEEPSORT_BANK_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(p.max_age >= 0 && p.n_init >= 0, AIC_ERR_INVALID, "negative tracker parameter");
    AIC_REQUIRE(p.nn_budget > 0, AIC_ERR_INVALID, "a DeepSORT bank runs the device association: nn_budget must be > 0");
    AIC_REQUIRE(p.max_tracks >= 0 && p.max_tracks <= TRK_DEV_TMAX, AIC_ERR_INVALID, "a DeepSORT bank runs the device association: max_tracks must be in 0..512 (0 = 512)");
    AIC_REQUIRE(p.feature_dim >= 0 && p.feature_dim <= 1024 && p.feature_dim % 4 == 0, AIC_ERR_INVALID,
                "a DeepSORT bank runs the device association: feature_dim must be a multiple of 4 in 0..1024 (0 = 512)");
    AIC_REQUIRE(p.first_track_id >= 0, AIC_ERR_INVALID, "first_track_id must be >= 0");
    TrkDevParams t{};
    t.max_cos = (float)p.max_cosine_distance, t.clamp_cos = (float)(p.max_cosine_distance + 1e-5);    // as Tracker::run_epochs
    t.max_iou = (float)p.max_iou_distance, t.clamp_iou = (float)(p.max_iou_distance + 1e-5);
    t.max_age = p.max_age, t.n_init = p.n_init, t.gmax = p.nn_budget;
    t.dim = p.feature_dim ? p.feature_dim : 512;
    t.cap = p.max_tracks ? p.max_tracks : TRK_DEV_TMAX;
    if (first_id) *first_id = p.first_track_id > 0 ? p.first_track_id : 1;
    return t;
}

DeepSortBank::DeepSortBank(Device& d, const TrkDevParams& p, int first, int streams)
    : dev(&d), prm(p), first_id(first), n_streams(streams), cap(p.cap), gmax(p.gmax), dim(p.dim),
      tbl_bytes(sizeof(DevTrkHdr) + (sizeof(DevTrack) + 4) * (size_t)p.cap), tbl_stride((tbl_bytes + 255) / 256 * 256),
      gal_stride((size_t)p.cap * p.gmax * p.dim), lsap_fast(getenv("AICAM_TRK_NOFAST") == nullptr),
      wave_cascade(getenv("AICAM_TRK_NOWAVE") == nullptr) {
    d.use();
    // every allocation before anything is written: one that does not fit throws out of the constructor and the others are released
    d_tbl.alloc(tbl_stride * streams);
    d_mean.alloc((size_t)cap * 8 * streams);
    d_cov.alloc((size_t)cap * 64 * streams);
    d_gal_raw.alloc(gal_stride * streams);
    d_gal_n.alloc(gal_stride * streams);
    d_appends.alloc((size_t)TRK_APPENDS_INTS * streams);
    stop_code.assign(streams, 0);
    stop_msg.assign(streams, std::string());
    tbl_init.assign(tbl_bytes, 0);
    DevTrkHdr* h = reinterpret_cast<DevTrkHdr*>(tbl_init.data());
    h->next_id = first_id, h->n_free = cap;
    int* fr = reinterpret_cast<int*>(tbl_init.data() + sizeof(DevTrkHdr) + sizeof(DevTrack) * (size_t)cap);
    for (int i = 0; i < cap; ++i) fr[i] = cap - 1 - i;             // handed out from the end: lowest slot first (Tracker::Tracker)
    hipStream_t s = dev->s_trk;
    HIP_CHECK(hipMemsetAsync(d_mean.p, 0, d_mean.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_cov.p, 0, d_cov.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_appends.p, 0, d_appends.bytes(), s));
    for (int q = 0; q < streams; ++q) clear_table(q);
    HIP_CHECK(hipStreamSynchronize(s));
}

void DeepSortBank::clear_table(int s) {
    HIP_CHECK(hipMemcpyAsync(table(s), tbl_init.data(), tbl_bytes, hipMemcpyHostToDevice, dev->s_trk));   // pageable source: copied before the call returns
}

void DeepSortBank::reset_stream(int s) {
    check_stream(s);
    dev->use();
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    clear_table(s);                                               // glen = 0 everywhere: the galleries are empty with it
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    stop_code[s] = 0, stop_msg[s].clear();
}

static std::string err_text(int err) {
    if (err == 1) return "track capacity exhausted (raise max_tracks)";
    if (err == 3) return "frame beyond the epoch kernel's capacity";
    return "the assignment problem has no finite solution";
}

void DeepSortBank::plan_epochs(BankPlan& pl, const int32_t* counts, const int* d0, bool feats, const int32_t* valid) const {
    const int S = n_streams, st = pl.frame_stride;
    const int kmax = std::max(1, std::min(std::min(TRK_KMAX, epoch_frames > 0 ? epoch_frames : TRK_KMAX), gmax));
    auto row_of = [&](int q, int i) { return pl.stream_f0[q] + i * st; };
    for (int f = 0; f < pl.kmax_s;) {
        int ke = std::min(kmax, pl.kmax_s - f);
        for (int q = 0; q < S; ++q) {
            int dn = 0, kk = 0;
            while (kk < ke && f + kk < pl.stream_k[q] && dn + counts[row_of(q, f + kk)] <= TRK_DEV_DNMAX) dn += counts[row_of(q, f + kk)], ++kk;
            if (f + kk < pl.stream_k[q]) ke = std::min(ke, kk);     // cut by the row budget, not by the stream's end
        }
        BankPlan::Epoch e{f, ke, 0};
        for (int q = 0; q < S; ++q) {
            EpochStreamPlan p{};
            p.map0 = (int)pl.row_map.size();
            p.nmax = 1;
            bool any_valid = false;
            for (int i = f; i < f + ke && i < pl.stream_k[q]; ++i) {
                const int row = row_of(q, i), c = counts[row];
                pl.e0[row] = p.dn;
                p.dn += c, p.nmax = std::max(p.nmax, c);
                for (int j = 0; j < c; ++j) {
                    pl.row_map.push_back(d0[row] + j);
                    any_valid |= !valid || valid[d0[row] + j] != 0;
                }
            }
            p.dn_pad = std::max(32, (p.dn + 31) / 32 * 32);
            p.has_sm = (feats && any_valid) ? 1 : 0;          // a stream without detections, or without features, runs without SM / GRAM
            if (p.has_sm) e.dn_pad_max = std::max(e.dn_pad_max, p.dn_pad);
            pl.plans.push_back(p);
        }
        pl.dn_pad_call = std::max(pl.dn_pad_call, e.dn_pad_max);
        pl.epochs.push_back(e);
        f += ke;
    }
}

// scratch slices for what the call needs (not the kernels' maxima: SM alone is 71 MB per stream there)
void DeepSortBank::size_scratch(const BankPlan& pl) {
    const int S = n_streams;
    sm_stride = std::max(sm_stride, (size_t)cap * (TRK_KMAX + 1) * pl.dn_pad_call);
    gram_stride = std::max(gram_stride, (size_t)pl.dn_pad_call * pl.dn_pad_call);
    cost_stride = std::max(cost_stride, (size_t)3 * cap * pl.nmax_call);
    sub_stride = std::max(sub_stride, (size_t)cap * pl.nmax_call);
    d_sm.ensure(sm_stride * S), d_gram.ensure(gram_stride * S), d_cost.ensure(cost_stride * S), d_sub.ensure(sub_stride * S);
}

// the plan block of a call (DeepSortPlanBlock, epoch_stage.hpp) into the start of its staging buffer
static void fill_plan(char* h, const DeepSortPlanBlock& b, const BankPlan& pl) {
    std::memcpy(h, pl.plans.data(), b.o_map);
    if (!pl.row_map.empty()) std::memcpy(h + b.o_map, pl.row_map.data(), pl.row_map.size() * 4);
    std::memcpy(h + b.o_e0, pl.e0.data(), pl.e0.size() * 4);
    std::memcpy(h + b.o_f0, pl.stream_f0.data(), pl.stream_f0.size() * 4);
    std::memcpy(h + b.o_k, pl.stream_k.data(), pl.stream_k.size() * 4);
}

void DeepSortBank::launch_epochs(const BankPlan& pl, const char* d_base, const DeepSortPlanBlock& b, const EpochDets& dets, const EpochOut& out,
                                 hipStream_t s) {
    const int S = n_streams;
    auto ints = [&](size_t o) { return reinterpret_cast<const int*>(d_base + o); };
    EpochBankArgs bk{};
    bk.tbl = d_tbl.p, bk.tbl_stride = tbl_stride;
    bk.mean_stride = (size_t)cap * 8, bk.cov_stride = (size_t)cap * 64, bk.gal_stride = gal_stride;
    bk.sm_stride = sm_stride, bk.gram_stride = gram_stride, bk.cost_stride = cost_stride, bk.sub_stride = sub_stride;
    bk.stream_f0 = ints(b.o_f0), bk.stream_k = ints(b.o_k);
    bk.frame_stride = pl.frame_stride;
    bk.row_map = ints(b.o_map);
    bk.frame_e0 = ints(b.o_e0);
    TrkDevParams p = prm;
    p.no_fast = lsap_fast ? 0 : 1, p.no_wave = wave_cascade ? 0 : 1;
    const EpochScratch scr{d_sm.p, d_gram.p, d_cost.p, d_sub.p, d_appends.p};
    for (size_t e = 0; e < pl.epochs.size(); ++e) {
        const BankPlan::Epoch& ep = pl.epochs[e];
        bk.plan = reinterpret_cast<const EpochStreamPlan*>(d_base) + e * S;
        if (ep.dn_pad_max > 0) {
            Prof pr(*dev, PROF_TRK, s, 0, 0);
            launch_trk_epoch_prep_bank(bk, S, d_gal_n.p, gmax, dim, cap, dets.feat_n, ep.dn_pad_max, ep.f0, ep.k, d_sm.p, d_gram.p, s);
        }
        Prof pr(*dev, PROF_TRK, s, 0, 0);
        launch_trk_epoch_bank(bk, S, d_mean.p, d_cov.p, d_gal_raw.p, d_gal_n.p, p, dets, ep.f0, ep.k, pl.nmax_call, scr, out, s);
    }
}

void DeepSortBank::note_stops(const DevTrkHdr* hh) {
    for (int q = 0; q < n_streams; ++q) {
        if (stop_code[q] || hh[q].err == 0) continue;
        stop_code[q] = hh[q].err == 2 ? AIC_ERR_RUNTIME : AIC_ERR_CAPACITY;
        stop_msg[q] = "stream " + std::to_string(q) + ": " + err_text(hh[q].err) + " (frame " + std::to_string(hh[q].err_frame) + " of the call)";
    }
}

void DeepSortBank::run_group(const EpochDets& dets, const int* h_n, const int* h_d0, int frames, const EpochOut& out, hipStream_t s) {
    const int S = n_streams;
    AIC_REQUIRE(frames > 0 && frames % S == 0, AIC_ERR_INVALID, "a launch group must hold whole ticks of every stream");
    for (int q = 0; q < S; ++q)
        AIC_REQUIRE(!stop_code[q], AIC_ERR_INVALID, "DeepSORT bank stream stopped by an earlier error (reset it first): " + stop_msg[q]);
    BankPlan& pl = grp;
    pl = BankPlan{};
    pl.stream_f0.resize(S), pl.stream_k.assign(S, frames / S);
    for (int q = 0; q < S; ++q) pl.stream_f0[q] = q;
    pl.frame_stride = S, pl.kmax_s = frames / S;
    size_t n = 0;
    for (int f = 0; f < frames; ++f) {
        AIC_REQUIRE(h_n[f] >= 0 && h_n[f] <= TRK_DEV_NMAX, AIC_ERR_CAPACITY, "DeepSORT bank: more than 512 detections in one frame");
        pl.nmax_call = std::max(pl.nmax_call, h_n[f]);
        n += (size_t)h_n[f];
    }
    pl.e0.resize(frames);
    pl.row_map.reserve(n);
    // the crop validity lives in HBM: a stream's SM / GRAM are built whenever it has rows (Tracker::run_epochs)
    plan_epochs(pl, h_n, h_d0, dets.feat_n != nullptr, nullptr);
    StageCursor c; const DeepSortPlanBlock b(c, pl.epochs.size(), S, (size_t)frames, n);
    const size_t o_hdr = c.take((size_t)S * sizeof(DevTrkHdr), true), bytes = c.at;
    if (bytes > h_grp.n) {                                         // (the caller synced s behind the previous group)
        HIP_CHECK(hipStreamSynchronize(s));
        h_grp.alloc(bytes + bytes / 4), d_grp.alloc(bytes + bytes / 4);
    }
    size_scratch(pl);
    fill_plan(h_grp.p, b, pl);
    HIP_CHECK(hipMemcpyAsync(d_grp.p, h_grp.p, o_hdr, hipMemcpyHostToDevice, s));
    launch_epochs(pl, d_grp.p, b, dets, out, s);
    HIP_CHECK(hipMemcpy2DAsync(d_grp.p + o_hdr, sizeof(DevTrkHdr), d_tbl.p, tbl_stride, sizeof(DevTrkHdr), S, hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemcpyAsync(h_grp.p + o_hdr, d_grp.p + o_hdr, (size_t)S * sizeof(DevTrkHdr), hipMemcpyDeviceToHost, s));
    grp_hdr = o_hdr;
}

int DeepSortBank::check_group() {
    const DevTrkHdr* hh = reinterpret_cast<const DevTrkHdr*>(h_grp.p + grp_hdr);
    const std::vector<int> before = stop_code;
    note_stops(hh);
    int bad = -1;
    grp_good.assign(n_streams, 0);
    for (int q = 0; q < n_streams; ++q) {
        grp_good[q] = before[q] ? 0 : stop_code[q] ? hh[q].err_frame : grp.stream_k[q];
        if (bad < 0 && stop_code[q] && !before[q]) bad = q;
    }
    return bad;
}

void DeepSortBank::update(const int32_t* frames_per_stream, const int32_t* counts, const float* det_tlwh, const float* conf, const int32_t* cls,
                          const float* feat, const int32_t* valid, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf,
                          int32_t* status) {
    dev->use();
    AIC_REQUIRE(cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
    const int S = n_streams;
    const CallShape sh = check_call("DeepSORT bank", S, frames_per_stream, counts, det_tlwh && conf && cls, 1l << 30);
    AIC_REQUIRE(sh.err.empty(), sh.capacity ? AIC_ERR_CAPACITY : AIC_ERR_INVALID, sh.err);
    if (status) std::copy(stop_code.begin(), stop_code.end(), status);
    const std::vector<int> before = stop_code;
    int bad = -1;
    if (sh.F > 0) {
        hipStream_t s = dev->s_trk;
        const size_t k = (size_t)sh.F, n = (size_t)sh.total;
        const bool feats = feat != nullptr && n > 0;

        // ---- the call's epochs (plan_epochs: shared with run_group)
        BankPlan pl;
        pl.stream_f0.resize(S), pl.stream_k.assign(frames_per_stream, frames_per_stream + S);
        for (int q = 0, f = 0; q < S; ++q) { pl.stream_f0[q] = f; f += frames_per_stream[q]; }
        pl.frame_stride = 1, pl.kmax_s = sh.kmax_s, pl.nmax_call = std::max(1, sh.nmax);
        std::vector<int> d0(k);
        { int d = 0; for (size_t f = 0; f < k; ++f) { d0[f] = d; d += counts[f]; } }
        pl.e0.resize(k);
        pl.row_map.reserve(n);
        plan_epochs(pl, counts, d0.data(), feats, valid);

        // ---- the one staging layout (epoch_stage.hpp); this caller's own: the plan block in front, feat behind valid, the headers behind the outputs
        StageCursor c; const DeepSortPlanBlock pb(c, pl.epochs.size(), S, k, n);
        const CallStage L = deepsort_stage(c, S, k, n, cap_rows, feats, dim);
        HIP_CHECK(hipStreamSynchronize(s));
        h_api.ensure(L.bytes);
        d_api.ensure(L.o_featn + L.feat_bytes);
        size_scratch(pl);
        fill_plan(h_api.p, pb, pl);
        L.det.fill(h_api.p, counts, det_tlwh, false, conf, cls);
        L.det.fill_valid(h_api.p, feats, valid);
        if (feats) std::memcpy(h_api.p + L.o_feat, feat, L.feat_bytes);
        HIP_CHECK(hipMemcpyAsync(d_api.p, h_api.p, L.out.o_out, hipMemcpyHostToDevice, s));
        EpochDets dets = L.det.dets(d_api.p);
        if (feats) {
            float* fn = reinterpret_cast<float*>(d_api.p + L.o_featn);
            dets.feat = reinterpret_cast<const float*>(d_api.p + L.o_feat);
            launch_normalize_rows(dets.feat, fn, (int)n, dim, s);  // once over all rows of the call
            dets.feat_n = fn;
        }
        launch_epochs(pl, d_api.p, pb, dets, L.out.out(d_api.p), s);
        HIP_CHECK(hipMemcpy2DAsync(d_api.p + L.o_tail, sizeof(DevTrkHdr), d_tbl.p, tbl_stride, sizeof(DevTrkHdr), S, hipMemcpyDeviceToDevice, s));
        HIP_CHECK(hipMemcpyAsync(h_api.p + L.out.o_out, d_api.p + L.out.o_out, L.bytes - L.out.o_out, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        const DevTrkHdr* hh = reinterpret_cast<const DevTrkHdr*>(h_api.p + L.o_tail);
        note_stops(hh);
        // a stream stopped before the call delivers nothing; one that stopped in it, the frames before the failing one
        auto good = [&](int q, int i) { return i < (before[q] ? 0 : stop_code[q] ? hh[q].err_frame : frames_per_stream[q]); };
        deliver(L.out.host(h_api.p), cap_rows, S, frames_per_stream, good, n_out, out6, out_conf);
        for (int q = S - 1; q >= 0; --q)
            if (stop_code[q] && frames_per_stream[q] > 0) bad = q;
    }
    if (status) std::copy(stop_code.begin(), stop_code.end(), status);
    else AIC_REQUIRE(bad < 0, stop_code[bad], "DeepSORT bank: " + stop_msg[bad]);
}

std::vector<char> DeepSortBank::fetch_table(int s) {
    check_stream(s);
    dev->use();
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    std::vector<char> h(tbl_bytes);
    HIP_CHECK(hipMemcpy(h.data(), table(s), tbl_bytes, hipMemcpyDeviceToHost));
    return h;
}

int DeepSortBank::export_state(int stream, int cap_rows, int32_t* id, int32_t* state, int32_t* hits, int32_t* age, int32_t* tsu, int32_t* cls,
                               float* conf, int32_t* gallery_len, float* mean, float* cov) {
    check_stream(stream);
    // after an error the table is the failing frame's half-way state: there is no frame boundary to report
    AIC_REQUIRE(!stop_code[stream], AIC_ERR_INVALID, "DeepSORT bank stream stopped by an earlier error (no consistent state to export): " + stop_msg[stream]);
    const std::vector<char> h = fetch_table(stream);
    const DevTrkHdr* hh = reinterpret_cast<const DevTrkHdr*>(h.data());
    const DevTrack* ht = reinterpret_cast<const DevTrack*>(h.data() + sizeof(DevTrkHdr));
    std::vector<float> hm, hc;
    if (mean) {
        hm.resize((size_t)cap * 8);
        HIP_CHECK(hipMemcpy(hm.data(), d_mean.p + (size_t)stream * cap * 8, hm.size() * 4, hipMemcpyDeviceToHost));
    }
    if (cov) {
        hc.resize((size_t)cap * 64);
        HIP_CHECK(hipMemcpy(hc.data(), d_cov.p + (size_t)stream * cap * 64, hc.size() * 4, hipMemcpyDeviceToHost));
    }
    const int T = hh->n_tracks;
    for (int i = 0; i < T && i < cap_rows; ++i) {
        const DevTrack& r = ht[i];
        if (id) id[i] = r.id;
        if (state) state[i] = r.state;
        if (hits) hits[i] = r.hits;
        if (age) age[i] = r.age;
        if (tsu) tsu[i] = r.tsu;
        if (cls) cls[i] = r.cls;
        if (conf) conf[i] = r.conf;
        if (gallery_len) gallery_len[i] = r.glen;
        if (mean) std::copy(hm.begin() + (size_t)r.slot * 8, hm.begin() + (size_t)r.slot * 8 + 8, mean + (size_t)i * 8);
        if (cov) std::copy(hc.begin() + (size_t)r.slot * 64, hc.begin() + (size_t)r.slot * 64 + 64, cov + (size_t)i * 64);
    }
    return T;
}

void DeepSortBank::export_gallery(int stream, int index, float* out, int cap_rows) {
    check_stream(stream);
    AIC_REQUIRE(!stop_code[stream], AIC_ERR_INVALID, "DeepSORT bank stream stopped by an earlier error (no consistent state to export): " + stop_msg[stream]);
    const std::vector<char> h = fetch_table(stream);
    const DevTrkHdr* hh = reinterpret_cast<const DevTrkHdr*>(h.data());
    const DevTrack* ht = reinterpret_cast<const DevTrack*>(h.data() + sizeof(DevTrkHdr));
    AIC_REQUIRE(index >= 0 && index < hh->n_tracks, AIC_ERR_INVALID, "track index out of range");
    const DevTrack& r = ht[index];
    AIC_REQUIRE(r.glen <= cap_rows, AIC_ERR_CAPACITY, "gallery capacity too small");
    const float* g = d_gal_raw.p + (size_t)stream * gal_stride + (size_t)r.slot * gmax * dim;
    const int first = std::min(r.glen, gmax - r.ghead);          // the ring in FIFO order: [ghead, gmax) then [0, ...)
    if (first > 0) HIP_CHECK(hipMemcpy(out, g + (size_t)r.ghead * dim, (size_t)first * dim * 4, hipMemcpyDeviceToHost));
    if (r.glen > first) HIP_CHECK(hipMemcpy(out + (size_t)first * dim, g, (size_t)(r.glen - first) * dim * 4, hipMemcpyDeviceToHost));
}

void DeepSortBank::counters(int stream, int64_t* n_fast, int64_t* n_lsap) {
    const std::vector<char> h = fetch_table(stream);
    const DevTrkHdr* hh = reinterpret_cast<const DevTrkHdr*>(h.data());
    if (n_fast) *n_fast = hh->n_fast;
    if (n_lsap) *n_lsap = hh->n_lsap;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_deepsort_bank_create(int device_id, const aic_tracker_params* p, int streams, aic_deepsort_bank** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        int first = 1;
        const TrkDevParams t = deepsort_bank_params(*p, streams, &first);
        *out = new aic_deepsort_bank(device(device_id), t, first, streams);
    });
}

int aic_deepsort_bank_destroy(aic_deepsort_bank* b) {
    return guarded([&] { delete b; });
}

int aic_deepsort_bank_option(aic_deepsort_bank* b, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(b && key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        if (k == "lsap_fast") b->t.lsap_fast = value != 0;
        else if (k == "wave_cascade") b->t.wave_cascade = value != 0;
        else if (k == "epoch_frames") {
            AIC_REQUIRE(value >= 0 && value <= TRK_KMAX, AIC_ERR_INVALID, "epoch_frames must be in 0..16 (0 = default)");
            b->t.epoch_frames = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown DeepSORT bank option: " + k);
    });
}

int aic_deepsort_bank_update(aic_deepsort_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* det_tlwh,
                             const float* conf, const int32_t* cls, const float* feat, const int32_t* valid, int cap_rows, int32_t* n_out,
                             int32_t* out6, float* out_conf, int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(b && frames_per_stream, AIC_ERR_INVALID, "NULL argument");
        bool any = false;
        for (int s = 0; s < b->t.n_streams; ++s) any |= frames_per_stream[s] > 0;
        AIC_REQUIRE(!any || counts, AIC_ERR_INVALID, "NULL argument");
        b->t.update(frames_per_stream, counts, det_tlwh, conf, cls, feat, valid, cap_rows, n_out, out6, out_conf, status);
    });
}

int aic_deepsort_bank_reset(aic_deepsort_bank* b, int stream) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.reset_stream(stream);
    });
}

int aic_deepsort_bank_export(aic_deepsort_bank* b, int stream, int cap, int32_t* track_id, int32_t* state, int32_t* hits, int32_t* age,
                             int32_t* time_since_update, int32_t* cls, float* conf, int32_t* gallery_len, float* mean, float* cov,
                             int32_t* n_tracks) {
    return guarded([&] {
        AIC_REQUIRE(b && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const int n = b->t.export_state(stream, cap, track_id, state, hits, age, time_since_update, cls, conf, gallery_len, mean, cov);
        if (n_tracks) *n_tracks = n;
    });
}

int aic_deepsort_bank_export_gallery(aic_deepsort_bank* b, int stream, int index, float* out, int cap_rows) {
    return guarded([&] {
        AIC_REQUIRE(b && out, AIC_ERR_INVALID, "NULL argument");
        b->t.export_gallery(stream, index, out, cap_rows);
    });
}

int aic_deepsort_bank_counters(aic_deepsort_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL bank");
        b->t.counters(stream, n_fast, n_lsap);
    });
}

}  // extern "C"
