// ocsort_host.hpp -- the OC-SORT tracker object (ocsort.cpp): a bank of streams (epoch_bank.hpp) over the device tables of ocsort.hpp.
// Used by the C ABI (aic_ocsort_*: a bank of one; aic_ocsort_bank_*) and by the pipeline (aic_pipeline_create_ocsort).
#pragma once
#include "common.hpp"
#include "epoch_bank.hpp"
#include "ocsort.hpp"

namespace aic {

OcParams ocsort_params(const aic_ocsort_params& p, int* first_id);

struct OcExport {                   // aic_ocsort_export's arrays, any may be NULL
    int32_t *id, *age, *hits, *streak, *tsu, *cls, *frozen, *has_obs;
    float *score, *last, *vel, *mean, *cov;
};

struct OcSortTracker : EpochBank<OcHdr, OcParams> {
    OcSortTracker(Device& d, const OcParams& p, int first_id, int streams = 1);
    const char* name() const override { return "OC-SORT"; }
    void launch(const OcParams& p, const EpochCall& c, hipStream_t s) override;
    std::string err_text(int err) const override;
    // the single tracker's call: k consecutive frames of stream 0 of a bank of one
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                      int32_t* n_out, int32_t* out6, float* out_conf);
    OcHdr header(int stream);
    int export_state(int stream, int cap_rows, const OcExport& e);
};

}  // namespace aic

struct aic_ocsort {
    aic::OcSortTracker t;
    aic_ocsort(aic::Device& d, const aic::OcParams& p, int first_id) : t(d, p, first_id) {}
};
struct aic_ocsort_bank {
    aic::OcSortTracker t;
    aic_ocsort_bank(aic::Device& d, const aic::OcParams& p, int first_id, int streams) : t(d, p, first_id, streams) {}
};
