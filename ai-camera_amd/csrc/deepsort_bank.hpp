// deepsort_bank.hpp -- a bank of DeepSORT streams on one device (deepsort_bank.cpp, C ABI aic_deepsort_bank_*): S cameras per launch of the
// device association (kernels_trk_dev.hip, trk_dev.hpp: block s of trk_epoch_kernel = stream s, the stream as the second grid dimension
// of trk_epoch_prep_kernel and gallery_commit_kernel).  A stream computes exactly what an aic_tracker with "device_assoc" fed the same
// frames computes -- it is that tracker's code in its arithmetic order -- and a stream that exhausts max_tracks stops alone.
// Two entries: update() stages a call's detections and features from host memory; run_group() is the pipeline's
// (aic_pipeline_create_deepsort_bank) and reads them where they already are in HBM.
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
#include "epoch_stage.hpp"
#include "kernels.hpp"
#include "trk_dev.hpp"

namespace aic {

constexpr int DEEPSORT_BANK_STREAMS_MAX = 256;

// the checks of aic_deepsort_bank_create: nothing is touched before they pass.  Returns the kernel's parameters.
TrkDevParams deepsort_bank_params(const aic_tracker_params& p, int streams, int* first_id);

// The epochs of one call, planned on the host from the per-frame counts: what update() and run_group() upload in front of their launches.
// Local frame i of stream q is row stream_f0[q] + i * frame_stride of the call's frame arrays (update: stream-major, stride 1;
// run_group: tick-major, stream_f0[q] = q, stride S).
struct BankPlan {
    struct Epoch { int f0, k, dn_pad_max; };
    std::vector<Epoch> epochs;
    std::vector<EpochStreamPlan> plans;             // [epochs][S]
    std::vector<int> row_map;                       // per (epoch, stream): epoch-local row -> detection row
    std::vector<int> e0;                            // [frames] first epoch-local row of the frame, by the frame's row
    std::vector<int> stream_f0, stream_k;           // [S]
    int frame_stride = 1, kmax_s = 0, nmax_call = 1, dn_pad_call = 0;
};

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
    PinBuf<char> h_grp;                             // run_group: plan | row_map | frame_e0 | stream_f0 | stream_k || headers[S]
    DevBuf<char> d_grp;
    size_t grp_hdr = 0;                             // offset of the headers in h_grp / d_grp
    BankPlan grp;                                   // the group between run_group() and check_group()
    std::vector<int> grp_good;                      // per stream, after check_group(): frames of the group that were delivered
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
    // The pipeline's entry: `frames` frames (a multiple of S) tick-major, frame t * S + s = tick t of stream s.  `dets` is device memory
    // (rows already normalised: feat_n), h_n / h_d0 its per-frame counts and first rows on the host.  Only the plan is uploaded -- no
    // box, no feature -- then the launches of update() with frame_stride = S; the S headers are gathered and read back on s.  No sync:
    // check_group() after the caller's.  A stream stopped before the call refuses the group.
    void run_group(const EpochDets& dets, const int* h_n, const int* h_d0, int frames, const EpochOut& out, hipStream_t s);
    // after the caller's sync: the group's headers -> per-stream stops (as update()), grp_good.  Returns the lowest stream that stopped
    // in the group, or -1.
    int check_group();
    // ---- what update() and run_group() share
    // the call's epochs.  k is common to the streams of a launch: the largest k <= min(epoch_frames or 16, gmax) for which every stream's
    // rows of the epoch stay within TRK_DEV_DNMAX.  valid (host, may be NULL = all): a stream's SM / GRAM are built when it has a valid row
    void plan_epochs(BankPlan& pl, const int32_t* counts, const int* d0, bool feats, const int32_t* valid) const;
    void size_scratch(const BankPlan& pl);
    // prep + epoch + commit of every epoch; the uploaded plan lies at d_base as b says
    void launch_epochs(const BankPlan& pl, const char* d_base, const DeepSortPlanBlock& b, const EpochDets& dets, const EpochOut& out,
                       hipStream_t s);
    void note_stops(const DevTrkHdr* hh);
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
