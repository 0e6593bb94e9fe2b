// ocsort.hpp -- OC-SORT on the device (OCSort.update of the OC-SORT authors, restated in tests/ocsort_oracle.py): the structures shared
// by kernels_ocsort.hip (the epoch kernel, one block per stream) and ocsort.cpp (tracker object, pipeline hook).
//
// The track table lives in HBM between launches, indexed by SLOT:
//   OcHdr | OcTrack[cap] | track list[cap] (slots, list order) | mean[cap][8] | cov[cap][64] | frozen mean[cap][8] | frozen cov[cap][64]
//   | ring age[cap][OC_DTMAX] | ring box[cap][OC_DTMAX][4]
// (7-state filter stored with a pitch of 8: lane (i, j) of a wavefront <-> P[i][j]).  A bank holds the tables of its streams
// `table_stride` bytes apart in one allocation.  An epoch launch (ONE block of 512 threads per stream) loads the
// scalars, the list and the means into LDS, walks k <= TRK_KMAX frames with no host round trip and writes them back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trk_dev.hpp"

namespace aic {

constexpr int OC_DTMAX = 8;         // largest delta_t: the observation ring of a track

struct OcHdr {
    int32_t n_tracks, next_id, frame;               // list length; the id the next new track takes; updates done (frame_count)
    int32_t err;                    // 0 ok; 1 track slots exhausted (max_tracks); 2 no finite assignment; 3 more than 512 detections in a frame
    int32_t err_frame;              // group frame index the error was raised at
    int32_t n_fast, n_lsap;         // assignment problems settled by upstream's read-off / by the LSAP, since creation
    int32_t max_side;               // largest side of a problem that went to the LSAP (> 128: lsap_wave; beyond the LDS arena: matrix in HBM)
    int32_t n_oru, max_gap;         // ORU replays and the longest gap replayed
    int32_t n_ocr, n_byte;          // pairs made by the OCR stage / the BYTE stage
};

struct OcTrack {                    // per slot, 64 bytes
    int32_t id, age, hits, streak, tsu, cls;
    int32_t kstate;                 // KF7_NEW / KF7_OBSERVED / KF7_FROZEN
    int32_t has_obs, has_vel;
    float score;
    float last[4];                  // last observation, xyxy (-1 x4 before the first)
    float vel[2];                   // unit (dy, dx)
};

struct OcParams {                   // every threshold rounded to fp32 once
    float det_thresh, iou_thresh, inertia, low_thresh;
    int32_t max_age, min_hits, delta_t, use_byte;
    int32_t cap;                    // slots (max_tracks <= TRK_DEV_TMAX)
    int32_t no_fast;                // 1: stage 1 never takes the read-off
};

struct OcTable {                    // device pointers into one allocation
    OcHdr* hdr;
    OcTrack* trk;
    int32_t* tl;
    float *mean, *cov, *fmean, *fcov;
    int32_t* ring_age;
    float* ring_box;
};

static inline size_t oc_table_bytes(int cap) {
    return 64 + (size_t)cap * (sizeof(OcTrack) + 4 + 2 * (4 * 8 + 4 * 64) + OC_DTMAX * 4 + OC_DTMAX * 16);
}
__host__ __device__ static inline OcTable oc_table(char* base, int cap) {
    OcTable t;
    t.hdr = reinterpret_cast<OcHdr*>(base);
    t.trk = reinterpret_cast<OcTrack*>(base + 64);
    t.tl = reinterpret_cast<int32_t*>(base + 64 + (size_t)cap * sizeof(OcTrack));
    t.mean = reinterpret_cast<float*>(t.tl + cap);
    t.cov = t.mean + (size_t)cap * 8;
    t.fmean = t.cov + (size_t)cap * 64;
    t.fcov = t.fmean + (size_t)cap * 8;
    t.ring_age = reinterpret_cast<int32_t*>(t.fcov + (size_t)cap * 64);
    t.ring_box = reinterpret_cast<float*>(t.ring_age + (size_t)cap * OC_DTMAX);
    return t;
}

// one launch, one block per stream of the bank (EpochCall, trk_dev.hpp)
void launch_ocsort_epoch(const OcParams& prm, const EpochCall& c, hipStream_t s);

}  // namespace aic
