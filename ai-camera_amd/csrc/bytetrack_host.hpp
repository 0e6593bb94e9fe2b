// bytetrack_host.hpp -- the ByteTrack tracker object of one video stream (bytetrack.cpp): the device table of bytetrack.hpp, epoch
// planning and launch, error check and read-back.  Used by the C ABI (aic_bytetrack_*) and by the pipeline (aic_pipeline_create_bytetrack).
#pragma once
#include "bytetrack.hpp"
#include "common.hpp"
#include "epoch_tracker.hpp"

namespace aic {

BtParams bytetrack_params(const aic_bytetrack_params& p, int* first_id);

struct ByteTracker : EpochTracker {
    Device* dev;
    BtParams prm;
    DevBuf<char> d_tbl;
    BtTable tbl{};
    DevBuf<float> d_ext;            // extended matrices beyond the LDS arena
    PinBuf<char> h_api, h_hdr;
    DevBuf<char> d_api;
    int epoch_frames = 0;           // frames per epoch launch (0 = TRK_KMAX)
    bool lsap_fast = true;          // unique optima read off the costs (false: every problem through the LSAP)

    ByteTracker(Device& d, const BtParams& p, int first_id);
    // frames [0, frames) of `dets` as epochs on stream s; the header copy lands in h_hdr behind them (check_epochs() after the caller's sync)
    const char* name() const override { return "ByteTrack"; }
    void run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) override;
    void check_epochs() override;
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                      int32_t* n_out, int32_t* out6, float* out_conf);
    void counters(int64_t* n_fast, int64_t* n_lsap, int32_t* max_side);
    int export_state(int cap_rows, int32_t* id, int32_t* state, int32_t* act, int32_t* start, int32_t* end, int32_t* cls, float* score,
                     float* mean, float* cov, int32_t* n_tracked);
};

}  // namespace aic

struct aic_bytetrack {
    aic::ByteTracker t;
    aic_bytetrack(aic::Device& d, const aic::BtParams& p, int first_id) : t(d, p, first_id) {}
};
