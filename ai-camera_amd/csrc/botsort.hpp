// botsort.hpp -- BoT-SORT with ReID on the device (BoTSORT.update of tracker/bot_sort.py, restated in tests/botsort_oracle.py): the
// structures shared by kernels_botsort.hip (the epoch kernel: one block per stream) and botsort.cpp (tracker object, a bank of streams).
//
// The track table lives in HBM between launches, indexed by SLOT:
//   BsHdr | BtTrack[cap] | tracked list[cap] | lost list[cap] | mean[cap][8] | cov[cap][64] | has_feat[cap]     and   smooth[cap][dim]
// A bank holds the tables of its streams `table_stride` bytes apart and their smoothed features `smooth_stride` floats apart.
// An epoch launch (ONE block of 512 threads per stream) loads the scalars, the lists and the means into LDS, walks k <= TRK_KMAX frames with no host
// round trip (covariances and smoothed features stay in HBM) and writes them back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bytetrack.hpp"

namespace aic {

struct BsHdr {
    int32_t n_tracked, n_lost, next_id, frame_id;
    int32_t err;                    // 0 ok; 1 track slots exhausted; 3 an assignment problem beyond the LSAPs (extended side > 512)
    int32_t err_frame;
    int32_t max_side;               // largest extended side since creation
    int32_t pad;
    int64_t n_fast, n_lsap;         // assignment problems settled by the unique-optimum check / by the LSAP, since creation
    int64_t n_app;                  // matched pairs (stages 1 and 3) whose winning term was the appearance distance (d_emb < d_iou)
    int64_t cyc_cost, cyc_all;      // shader-clock cycles since creation: the appearance pass of the fused cost (dot products) / the whole kernel
};
constexpr size_t BS_HDR_BYTES = 128;
static_assert(sizeof(BsHdr) <= BS_HDR_BYTES, "header area");

struct BsParams {                   // every threshold rounded to fp32 once
    float high, low, new_thresh, match_thresh, second_thresh, unconf_thresh, dup_dist, proximity, appearance, alpha, one_minus_alpha;
    int32_t max_lost, fuse, reid, cap, dim, no_fast;
};

struct BsTable {                    // device pointers
    BsHdr* hdr;
    BtTrack* trk;                   // the per-slot scalars are ByteTrack's (bytetrack.hpp)
    int32_t* tl;
    int32_t* ll;
    float* mean;
    float* cov;
    int32_t* hasf;
    float* feat;                    // [cap, dim] smoothed unit features, its own allocation
};

static inline size_t bs_table_bytes(int cap) {
    return BS_HDR_BYTES + (size_t)cap * (sizeof(BtTrack) + 8 + 4 * 8 + 4 * 64 + 4);
}
__host__ __device__ static inline BsTable bs_table(char* base, int cap, float* feat) {
    BsTable t;
    t.hdr = reinterpret_cast<BsHdr*>(base);
    t.trk = reinterpret_cast<BtTrack*>(base + BS_HDR_BYTES);
    t.tl = reinterpret_cast<int32_t*>(base + BS_HDR_BYTES + (size_t)cap * sizeof(BtTrack));
    t.ll = t.tl + cap;
    t.mean = reinterpret_cast<float*>(t.ll + cap);
    t.cov = t.mean + (size_t)cap * 8;
    t.hasf = reinterpret_cast<int32_t*>(t.cov + (size_t)cap * 64);
    t.feat = feat;
    return t;
}

// one launch, one block per stream (EpochCall, trk_dev.hpp).  c.dets.feat_n (unit rows; NULL = no features) and c.dets.valid are read
// for the high band only, by detection row; smooth = the streams' smoothed features, smooth_stride floats apart; warps = [rows, 6] camera
// motion (r00 r01 t0 r10 r11 t1), rows as c.dets' frames, or NULL
void launch_botsort_epoch(const BsParams& prm, const EpochCall& c, float* smooth, size_t smooth_stride, const float* warps, hipStream_t s);
// out[r] = in[r] / |in[r]| in the order of kf8wh_math.hpp (one wavefront per row); out[r][0] = NaN marks a row that is not finite in
// every element, which the epoch kernel takes as a row without a feature
void launch_botsort_normalize(const float* in, float* out, int rows, int dim, hipStream_t s);

}  // namespace aic
