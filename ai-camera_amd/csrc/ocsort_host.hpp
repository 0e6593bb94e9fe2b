// ocsort_host.hpp -- the OC-SORT tracker object of one video stream (ocsort.cpp): the device table of ocsort.hpp, epoch planning and launch,
// error check and read-back.  Used by the C ABI (aic_ocsort_*) and by the pipeline (aic_pipeline_create_ocsort).
#pragma once
#include "common.hpp"
#include "epoch_tracker.hpp"
#include "ocsort.hpp"

namespace aic {

OcParams ocsort_params(const aic_ocsort_params& p, int* first_id);

struct OcExport {                   // aic_ocsort_export's arrays, any may be NULL
    int32_t *id, *age, *hits, *streak, *tsu, *cls, *frozen, *has_obs;
    float *score, *last, *vel, *mean, *cov;
};

struct OcSortTracker : EpochTracker {
    Device* dev;
    OcParams prm;
    DevBuf<char> d_tbl;
    OcTable tbl{};
    DevBuf<float> d_ext;            // cost matrices beyond the LDS arena
    PinBuf<char> h_api, h_hdr;
    DevBuf<char> d_api;
    int epoch_frames = 0;           // frames per epoch launch (0 = TRK_KMAX)
    bool lsap_fast = true;          // stage 1 takes upstream's read-off where it applies (false: every problem through the LSAP)

    OcSortTracker(Device& d, const OcParams& p, int first_id);
    const char* name() const override { return "OC-SORT"; }
    void run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) override;
    void check_epochs() override;
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                      int32_t* n_out, int32_t* out6, float* out_conf);
    OcHdr header();
    int export_state(int cap_rows, const OcExport& e);
};

}  // namespace aic

struct aic_ocsort {
    aic::OcSortTracker t;
    aic_ocsort(aic::Device& d, const aic::OcParams& p, int first_id) : t(d, p, first_id) {}
};
