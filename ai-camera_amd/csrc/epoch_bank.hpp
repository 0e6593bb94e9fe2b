// epoch_bank.hpp -- a bank of epoch-tracker streams on one device: what ByteTracker, OcSortTracker and BotSortTracker share.  One allocation
// holds the streams' tables `stride` bytes apart, every epoch launch is one EpochCall (trk_dev.hpp) and runs one block per stream
// (byte_epoch.hpp through kernels_bytetrack.hip / kernels_botsort.hip; kernels_ocsort.hip), and a stream that meets a capacity error stops alone.  The single trackers of the C ABI and the pipeline's default
// are banks of one.  BoT-SORT stages features, validity and camera motion on top (BankExtra); the detector-only trackers pass none and
// their staging layout and launches are what they were without it.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "common.hpp"
#include "epoch_stage.hpp"
#include "epoch_tracker.hpp"

namespace aic {

constexpr int BANK_STREAMS_MAX = 256;

// What update() stages on top of the detections for a tracker that sees appearance (host pointers, any may be NULL)
struct BankExtra {
    const float* feat;              // [rows, dim] raw embeddings of every detection row of the call
    const int32_t* valid;           // [rows]
    const float* warps6;            // [F, 6] camera motion per frame
    int dim;
};

// Hdr: the table header (next_id, err, err_frame; at the start of every table).  Prm: the kernel's parameters (no_fast).
template <class Hdr, class Prm>
struct EpochBank : EpochTracker {
    Device* dev;
    Prm prm;
    int first_id;
    int n_streams = 0;
    size_t tbl_bytes, stride, ext_floats;   // one table; distance of two tables; HBM scratch of one stream
    DevBuf<char> d_tbl;
    DevBuf<float> d_ext;
    PinBuf<char> h_api, h_hdr;
    DevBuf<char> d_api;
    PinBuf<int> h_plan;             // the pipeline's tick-major plan: stream_f0[S] | stream_k[S]
    DevBuf<int> d_plan;
    int epoch_frames = 0;           // frames per epoch launch (0 = TRK_KMAX)
    bool lsap_fast = true;
    bool used = false;              // frames have gone through the bank
    std::vector<int> stop_code;     // per stream: 0, or the error code that stopped it
    std::vector<std::string> stop_msg;

    EpochBank(Device& d, const Prm& p, int first, int streams, size_t table_bytes, size_t ext_per_stream)
        : dev(&d), prm(p), first_id(first), tbl_bytes(table_bytes), stride((table_bytes + 255) / 256 * 256), ext_floats(ext_per_stream) {
        resize(streams);
    }

    virtual void launch(const Prm& p, const EpochCall& c, hipStream_t s) = 0;
    virtual std::string err_text(int err) const = 0;
    // update() with a BankExtra: the extras are on their way to the device (stream s), before the epochs.  dets.valid / dets.feat are set
    // where given; d_warps is NULL without camera motion, d_feat_n [rows, dim] is free device memory for the normalised features.
    virtual void extra_staged(EpochDets&, const float* /*d_warps*/, float* /*d_feat_n*/, int /*rows*/, hipStream_t) {}

    int streams() const override { return n_streams; }
    char* table(int s) const { return d_tbl.p + (size_t)s * stride; }
    const Hdr& host_hdr(int s) const { return *reinterpret_cast<const Hdr*>(h_hdr.p + (size_t)s * sizeof(Hdr)); }

    void resize(int streams) {
        dev->use();
        HIP_CHECK(hipStreamSynchronize(dev->s_trk));
        n_streams = streams;
        d_tbl.alloc(stride * streams);
        d_ext.alloc(ext_floats * streams);
        h_hdr.alloc(sizeof(Hdr) * streams);
        h_plan.alloc(2 * (size_t)streams);
        d_plan.alloc(2 * (size_t)streams);
        stop_code.assign(streams, 0);
        stop_msg.assign(streams, std::string());
        failed = false, fail_msg.clear();
        for (int s = 0; s < streams; ++s) clear_table(s);
        HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    }
    void clear_table(int s) {
        HIP_CHECK(hipMemsetAsync(table(s), 0, tbl_bytes, dev->s_trk));
        Hdr h{};
        h.next_id = first_id;
        HIP_CHECK(hipMemcpyAsync(table(s), &h, sizeof(h), hipMemcpyHostToDevice, dev->s_trk));   // pageable source: copied before the call returns
    }
    void set_streams(int streams) override {
        AIC_REQUIRE(streams >= 1 && streams <= BANK_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
        AIC_REQUIRE(!used, AIC_ERR_INVALID, "streams is set before the first frames go through the tracker");
        if (streams != n_streams) resize(streams);
    }
    // the stream's table as after create (ids from first_track_id again), a stop cleared: a camera reconnecting
    void reset_stream(int s) override {
        AIC_REQUIRE(s >= 0 && s < n_streams, AIC_ERR_INVALID, "stream outside the bank");
        dev->use();
        HIP_CHECK(hipStreamSynchronize(dev->s_trk));
        clear_table(s);
        HIP_CHECK(hipStreamSynchronize(dev->s_trk));
        stop_code[s] = 0, stop_msg[s].clear();
        failed = false, fail_msg.clear();
        for (int q = n_streams - 1; q >= 0; --q)
            if (stop_code[q]) failed = true, fail_msg = stop_msg[q];
    }

    // local frames [0, kmax_s) of every stream as epochs of one block per stream on stream s; the headers' copy lands in h_hdr behind them
    void run_bank(const EpochDets& dets, int kmax_s, const int* stream_f0, const int* stream_k, int frame_stride, const EpochOut& out,
                  hipStream_t s) {
        used = true;
        const int kmax = epoch_frames > 0 ? epoch_frames : TRK_KMAX;
        Prm p = prm;
        p.no_fast = lsap_fast ? 0 : 1;
        for (int f = 0; f < kmax_s;) {
            const int k = std::min(kmax, kmax_s - f);
            {
                Prof pr(*dev, PROF_TRK, s, 0, 0);
                launch(p, EpochCall{d_tbl.p, stride, n_streams, frame_stride, dets, f, k, stream_f0, stream_k, d_ext.p, out}, s);
            }
            f += k;
        }
        if (n_streams == 1) HIP_CHECK(hipMemcpyAsync(h_hdr.p, d_tbl.p, sizeof(Hdr), hipMemcpyDeviceToHost, s));
        else HIP_CHECK(hipMemcpy2DAsync(h_hdr.p, sizeof(Hdr), d_tbl.p, stride, sizeof(Hdr), n_streams, hipMemcpyDeviceToHost, s));
    }

    // The pipeline's hook: the group's frames, tick-major over the streams.  A stopped stream refuses the group.
    void run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) override {
        AIC_REQUIRE(!failed, AIC_ERR_INVALID, std::string(name()) + " tracker stopped by an earlier error: " + fail_msg);
        if (n_streams == 1) return run_bank(dets, frames, nullptr, nullptr, 1, out, s);
        AIC_REQUIRE(frames % n_streams == 0, AIC_ERR_INVALID, "a launch group must hold whole ticks of every stream");
        for (int q = 0; q < n_streams; ++q) h_plan.p[q] = q, h_plan.p[n_streams + q] = frames / n_streams;
        HIP_CHECK(hipMemcpyAsync(d_plan.p, h_plan.p, 2 * (size_t)n_streams * 4, hipMemcpyHostToDevice, s));   // the caller syncs s before the next group
        run_bank(dets, frames / n_streams, d_plan.p, d_plan.p + n_streams, n_streams, out, s);
    }

    // after the caller's sync: the streams that stopped in the launches behind it.  Returns the lowest one, or -1.
    int collect() {
        int first = -1;
        for (int q = 0; q < n_streams; ++q) {
            const Hdr& h = host_hdr(q);
            if (stop_code[q] || h.err == 0) continue;
            stop_code[q] = AIC_ERR_CAPACITY;
            stop_msg[q] = (n_streams > 1 ? "stream " + std::to_string(q) + ": " : std::string()) + err_text(h.err) + " (frame " +
                          std::to_string(h.err_frame) + " of the call)";
            if (first < 0) first = q;
        }
        for (int q = n_streams - 1; q >= 0; --q)
            if (stop_code[q]) failed = true, fail_msg = stop_msg[q];
        return first;
    }
    void check_epochs() override {
        const int q = collect();
        AIC_REQUIRE(q < 0, AIC_ERR_CAPACITY, std::string(name()) + ": " + stop_msg[q]);
    }

    // frames_per_stream[S] frames of every stream, stream-major (F in all): one staging upload, ceil(max k / epoch_frames) launches of S
    // blocks, one read-back, one sync.  status (may be NULL): per stream 0 or the code that stopped it; with status NULL a stopped stream
    // raises after the other streams' rows have been delivered.
    void update(const int32_t* frames_per_stream, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                int32_t* n_out, int32_t* out6, float* out_conf, int32_t* status, const BankExtra* x = nullptr) {
        dev->use();
        AIC_REQUIRE(cap_rows >= 0, AIC_ERR_INVALID, "negative frame count / row capacity");
        const int S = n_streams;
        const CallShape sh = check_call(name(), S, frames_per_stream, counts, xyxy && conf && cls);
        AIC_REQUIRE(sh.err.empty(), sh.capacity ? AIC_ERR_CAPACITY : AIC_ERR_INVALID, sh.err);
        if (status) std::copy(stop_code.begin(), stop_code.end(), status);
        const std::vector<int> before = stop_code;
        int bad = -1;
        if (sh.F > 0) {
            hipStream_t s = dev->s_trk;
            const size_t n = (size_t)sh.total;
            // the one staging layout (epoch_stage.hpp); this caller's own: the stream plan in front, the BankExtra fields around the outputs
            const CallStage L = bank_stage(S, (size_t)sh.F, n, cap_rows, x && x->valid, x && x->warps6, x && x->feat, x ? x->dim : 0);
            HIP_CHECK(hipStreamSynchronize(s));
            h_api.ensure(L.bytes);
            d_api.ensure(x ? L.o_featn + L.feat_bytes : L.bytes);
            int* hp = reinterpret_cast<int*>(h_api.p);
            for (int q = 0, f = 0; q < S; ++q) { hp[q] = f; hp[S + q] = frames_per_stream[q]; f += frames_per_stream[q]; }
            L.det.fill(h_api.p, counts, xyxy, true, conf, cls);
            if (n && L.det.has_valid) std::memcpy(h_api.p + L.det.o_valid, x->valid, n * 4);
            if (L.has_feat) std::memcpy(h_api.p + L.o_feat, x->feat, L.feat_bytes);
            if (L.has_warps) std::memcpy(h_api.p + L.o_warp, x->warps6, (size_t)sh.F * 24);
            HIP_CHECK(hipMemcpyAsync(d_api.p, h_api.p, L.out.o_out, hipMemcpyHostToDevice, s));
            EpochDets dets = L.det.dets(d_api.p, L.has_feat ? reinterpret_cast<const float*>(d_api.p + L.o_feat) : nullptr);
            if (x)
                extra_staged(dets, L.has_warps ? reinterpret_cast<const float*>(d_api.p + L.o_warp) : nullptr,
                             reinterpret_cast<float*>(d_api.p + L.o_featn), (int)n, s);
            const int* dp = reinterpret_cast<const int*>(d_api.p);
            if (S == 1) run_bank(dets, sh.kmax_s, nullptr, nullptr, 1, L.out.out(d_api.p), s);
            else run_bank(dets, sh.kmax_s, dp, dp + S, 1, L.out.out(d_api.p), s);
            HIP_CHECK(hipMemcpyAsync(h_api.p + L.out.o_out, d_api.p + L.out.o_out, L.bytes - L.out.o_out, hipMemcpyDeviceToHost, s));
            HIP_CHECK(hipStreamSynchronize(s));
            collect();
            // a stream stopped before the call delivers nothing; one that stopped in it, the frames before the failing one
            auto good = [&](int q, int i) { return i < (before[q] ? 0 : stop_code[q] ? host_hdr(q).err_frame : frames_per_stream[q]); };
            deliver(L.out.host(h_api.p), cap_rows, S, frames_per_stream, good, n_out, out6, out_conf);
            for (int q = S - 1; q >= 0; --q)
                if (stop_code[q] && frames_per_stream[q] > 0) bad = q;
        }
        if (status) std::copy(stop_code.begin(), stop_code.end(), status);
        else AIC_REQUIRE(bad < 0, stop_code[bad], std::string(name()) + ": " + stop_msg[bad]);
    }

    // aic_<tracker>_option and aic_<tracker>_bank_option: the options every epoch tracker takes
    void option(const std::string& k, int value) {
        if (k == "lsap_fast") lsap_fast = value != 0;
        else if (k == "epoch_frames") {
            AIC_REQUIRE(value >= 0 && value <= TRK_KMAX, AIC_ERR_INVALID, "epoch_frames must be in 0..16 (0 = default)");
            epoch_frames = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, std::string("unknown ") + name() + " option: " + k);
    }
    // aic_<tracker>_bank_update: counts may be NULL only when no stream has frames
    void require_counts(const int32_t* frames_per_stream, const int32_t* counts) const {
        bool any = false;
        for (int s = 0; s < n_streams; ++s) any |= frames_per_stream[s] > 0;
        AIC_REQUIRE(!any || counts, AIC_ERR_INVALID, "NULL argument");
    }

    // the stream's table on the host (export, counters)
    std::vector<char> fetch_table(int s, size_t bytes) {
        AIC_REQUIRE(s >= 0 && s < n_streams, AIC_ERR_INVALID, "stream outside the bank");
        dev->use();
        HIP_CHECK(hipStreamSynchronize(dev->s_trk));
        std::vector<char> h(bytes);
        HIP_CHECK(hipMemcpy(h.data(), table(s), bytes, hipMemcpyDeviceToHost));
        return h;
    }
};

}  // namespace aic
