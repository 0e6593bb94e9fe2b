// botsort_host.hpp -- the BoT-SORT tracker object of one video stream (botsort.cpp): the device table of botsort.hpp, epoch planning and
// launch, error check and read-back.  Used by the C ABI (aic_botsort_*) and by the pipeline (aic_pipeline_create_botsort).
#pragma once
#include "botsort.hpp"
#include "common.hpp"
#include "epoch_tracker.hpp"

namespace aic {

BsParams botsort_params(const aic_botsort_params& p, int* first_id);

struct BotSortTracker : EpochTracker {
    Device* dev;
    BsParams prm;
    DevBuf<char> d_tbl;
    DevBuf<float> d_feat;           // smoothed features [cap, dim]
    BsTable tbl{};
    DevBuf<float> d_ext;            // extended matrices beyond the LDS arena
    PinBuf<char> h_api, h_hdr;
    DevBuf<char> d_api;
    const float* warps = nullptr;   // [frames, 6] camera motion of the next run_epochs (device memory); NULL = none
    int epoch_frames = 0;           // frames per epoch launch (0 = TRK_KMAX)
    bool lsap_fast = true;          // unique optima read off the costs (false: every problem through the LSAP)

    BotSortTracker(Device& d, const BsParams& p, int first_id);
    const char* name() const override { return "BoT-SORT"; }
    void run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) override;
    void check_epochs() override;
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, const float* feat,
                      const int32_t* valid, const float* warps6, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf);
    void counters(int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_app, int64_t* cyc_cost, int64_t* cyc_all);
    int export_state(int cap_rows, int32_t* id, int32_t* state, int32_t* act, int32_t* start, int32_t* end, int32_t* cls, float* score,
                     float* mean, float* cov, int32_t* has_feat, float* smooth, int32_t* n_tracked);
};

}  // namespace aic

struct aic_botsort {
    aic::BotSortTracker t;
    aic_botsort(aic::Device& d, const aic::BsParams& p, int first_id) : t(d, p, first_id) {}
};
