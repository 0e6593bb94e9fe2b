// deepsort_bank.hpp -- a bank of DeepSORT streams on one device (deepsort_bank.cpp, C ABI aic_deepsort_bank_*): S cameras per launch of the
// device association (kernels_trk_dev.hip, trk_dev.hpp: block s of trk_epoch_kernel = stream s, the stream as the second grid dimension
// of trk_epoch_prep_kernel and gallery_commit_kernel).  A stream computes exactly what an aic_tracker with "device_assoc" fed the same
// frames computes -- it is that tracker's code in its arithmetic order -- and a stream that exhausts max_tracks stops alone.
//
// Device association only: nn_budget > 0, max_tracks <= 512, feature_dim % 4 == 0; there is no host fallback and no gallery exchange
// between ranks (the cameras of one bank are linked by xcam.hpp).
//
// Memory per stream, resident:  table   32 + 52 * max_tracks bytes
//                               Kalman  (8 + 64) * 4 * max_tracks bytes
//                               galleries  2 * max_tracks * nn_budget * feature_dim * 4 bytes (raw rows for export + unit rows for the costs)
//   = 210 MB at the defaults 512 x 100 x 512, 26 MB at max_tracks 64: the number of streams is the caller's memory decision (<= 256).
// Scratch per stream, sized by the largest call so far (rows = detections of the stream in one epoch, padded to 32; n = detections per frame):
//   SM max_tracks * 17 * rows * 4, GRAM rows^2 * 4, full cost matrices 4 * max_tracks * n * 4 bytes  (2.3 MB at 64 tracks, 16 x 30 rows).
#pragma once
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"
#include "trk_dev.hpp"

namespace aic {

constexpr int DEEPSORT_BANK_STREAMS_MAX = 256;

// the checks of aic_deepsort_bank_create: nothing is touched before they pass.  Returns the kernel's parameters.
TrkDevParams deepsort_bank_params(const aic_tracker_params& p, int streams, int* first_id);

struct DeepSortBank {
    Device* dev;
    TrkDevParams prm;
    int first_id, n_streams, cap, gmax, dim;
    size_t tbl_bytes, tbl_stride, gal_stride;      // bytes of one table; bytes between two; floats of one gallery array of a stream
    DevBuf<char> d_tbl;
    DevBuf<float> d_mean, d_cov, d_gal_raw, d_gal_n;
    DevBuf<float> d_sm, d_gram, d_cost, d_sub;      // EpochScratch, one slice per stream
    DevBuf<int> d_appends;
    size_t sm_stride = 0, gram_stride = 0, cost_stride = 0, sub_stride = 0;
    PinBuf<char> h_api;
    DevBuf<char> d_api;
    std::vector<char> tbl_init;                     // a table as after create
    int epoch_frames = 0;                           // frames per epoch launch (0 = 16)
    bool lsap_fast, wave_cascade;
    std::vector<int> stop_code;                     // per stream: 0, or the error code that stopped it
    std::vector<std::string> stop_msg;

    DeepSortBank(Device& d, const TrkDevParams& p, int first, int streams);
    char* table(int s) const { return d_tbl.p + (size_t)s * tbl_stride; }
    void check_stream(int s) const { AIC_REQUIRE(s >= 0 && s < n_streams, AIC_ERR_INVALID, "stream outside the bank"); }
    void clear_table(int s);
    // the stream as after create (no tracks, empty galleries, ids from first_track_id again), a stop cleared
    void reset_stream(int s);
    // frames_per_stream[S] frames of every stream, stream-major: one staging upload, ceil(max k / k) x (prep + epoch + commit) launches of S
    // blocks (k common to the streams), one read-back with the S headers, one sync.  status (may be NULL): per stream 0 or the code that
    // stopped it; with status NULL a stopped stream raises after the other streams' rows have been delivered.
    void update(const int32_t* frames_per_stream, const int32_t* counts, const float* det_tlwh, const float* conf, const int32_t* cls,
                const float* feat, const int32_t* valid, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf, int32_t* status);
    std::vector<char> fetch_table(int s);
    int export_state(int stream, int cap_rows, int32_t* id, int32_t* state, int32_t* hits, int32_t* age, int32_t* tsu, int32_t* cls,
                     float* conf, int32_t* gallery_len, float* mean, float* cov);
    void export_gallery(int stream, int index, float* out, int cap_rows);
    void counters(int stream, int64_t* n_fast, int64_t* n_lsap);
};

}  // namespace aic

struct aic_deepsort_bank {
    aic::DeepSortBank t;
    aic_deepsort_bank(aic::Device& d, const aic::TrkDevParams& p, int first_id, int streams) : t(d, p, first_id, streams) {}
};
