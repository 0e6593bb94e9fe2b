// botsort_host.hpp -- the BoT-SORT tracker object (botsort.cpp): a bank of streams (epoch_bank.hpp) over the device tables of botsort.hpp,
// with the smoothed features as a second per-stream allocation.  Used by the C ABI (aic_botsort_*: a bank of one; aic_botsort_bank_*) and by
// the pipeline (aic_pipeline_create_botsort, aic_pipeline_create_botsort_bank).
#pragma once
#include "botsort.hpp"
#include "bytetrack_host.hpp"

namespace aic {

BsParams botsort_params(const aic_botsort_params& p, int* first_id);

struct BotSortTracker : EpochBank<BsHdr, BsParams> {
    DevBuf<float> d_feat;           // smoothed features [streams][cap, dim]: sized for the bank's streams, fixed at creation
    size_t feat_stride;             // floats between two streams' features
    const float* warps = nullptr;   // [rows, 6] camera motion of the next epochs (device memory, rows as the frames' of dets); NULL = none

    BotSortTracker(Device& d, const BsParams& p, int first_id, int streams = 1);
    const char* name() const override { return "BoT-SORT"; }
    void launch(const BsParams& p, const EpochCall& c, hipStream_t s) override;
    std::string err_text(int err) const override { return byte_err_text(err); }
    void extra_staged(EpochDets& dets, const float* d_warps, float* d_feat_n, int rows, hipStream_t s) override;
    void set_streams(int) override { AIC_REQUIRE(false, AIC_ERR_INVALID, "the streams of a BoT-SORT bank are fixed at creation"); }
    void reset_stream(int s) override;   // also the stream's smoothed features
    // frames_per_stream[S] frames of every stream, stream-major: EpochBank::update plus feat (all rows of the call or NULL), valid, warps6
    void update_bank(const int32_t* frames_per_stream, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls,
                     const float* feat, const int32_t* valid, const float* warps6, int cap_rows, int32_t* n_out, int32_t* out6,
                     float* out_conf, int32_t* status);
    // the single tracker's call: k consecutive frames of stream 0 of a bank of one
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, const float* feat,
                      const int32_t* valid, const float* warps6, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf);
    void counters(int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_app, int64_t* cyc_cost, int64_t* cyc_all);
    int export_state(int stream, int cap_rows, const ByteExport& e, int32_t* has_feat, float* smooth, int32_t* n_tracked);
};

}  // namespace aic

struct aic_botsort {
    aic::BotSortTracker t;
    aic_botsort(aic::Device& d, const aic::BsParams& p, int first_id) : t(d, p, first_id) {}
};
struct aic_botsort_bank {
    aic::BotSortTracker t;
    aic_botsort_bank(aic::Device& d, const aic::BsParams& p, int first_id, int streams) : t(d, p, first_id, streams) {}
};
