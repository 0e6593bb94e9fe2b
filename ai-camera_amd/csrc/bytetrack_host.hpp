// bytetrack_host.hpp -- the ByteTrack tracker object (bytetrack.cpp): a bank of streams (epoch_bank.hpp) over the device tables of
// bytetrack.hpp.  Used by the C ABI (aic_bytetrack_*: a bank of one; aic_bytetrack_bank_*) and by the pipeline (aic_pipeline_create_bytetrack).
#pragma once
#include "bytetrack.hpp"
#include "common.hpp"
#include "epoch_bank.hpp"

namespace aic {

BtParams bytetrack_params(const aic_bytetrack_params& p, int* first_id);

struct ByteTracker : EpochBank<BtHdr, BtParams> {
    ByteTracker(Device& d, const BtParams& p, int first_id, int streams = 1);
    const char* name() const override { return "ByteTrack"; }
    void launch(const BtParams& p, const EpochDets& dets, int f0, int k, const int* stream_f0, const int* stream_k, int frame_stride,
                const EpochOut& out, hipStream_t s) override;
    std::string err_text(int err) const override;
    // the single tracker's call: k consecutive frames of stream 0 of a bank of one
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                      int32_t* n_out, int32_t* out6, float* out_conf);
    void counters(int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side);
    int export_state(int stream, int cap_rows, int32_t* id, int32_t* state, int32_t* act, int32_t* start, int32_t* end, int32_t* cls,
                     float* score, float* mean, float* cov, int32_t* n_tracked);
};

}  // namespace aic

struct aic_bytetrack {
    aic::ByteTracker t;
    aic_bytetrack(aic::Device& d, const aic::BtParams& p, int first_id) : t(d, p, first_id) {}
};
struct aic_bytetrack_bank {
    aic::ByteTracker t;
    aic_bytetrack_bank(aic::Device& d, const aic::BtParams& p, int first_id, int streams) : t(d, p, first_id, streams) {}
};
