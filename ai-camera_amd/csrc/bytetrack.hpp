// bytetrack.hpp -- ByteTrack on the device (BYTETracker.update of yolox/tracker/byte_tracker.py, restated in tests/bytetrack_oracle.py):
// the structures shared by kernels_bytetrack.hip (the epoch kernel, one block per stream) and bytetrack.cpp (tracker object, pipeline hook).
//
// The track table lives in HBM between launches, indexed by SLOT (a slot is a track's place in the mean / cov arrays):
//   BtHdr | BtTrack[cap] | tracked list[cap] | lost list[cap] (slots, list order) | mean[cap][8] | cov[cap][64]
// A bank holds the tables of its streams `table_stride` bytes apart in one allocation.  An epoch launch (ONE block of 512 threads per
// stream) loads the scalars, the lists and the means into LDS, walks k <= TRK_KMAX frames with no host
// round trip (covariances stay in HBM) and writes them back.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "trk_dev.hpp"

namespace aic {

constexpr int BT_TRACKED = 1, BT_LOST = 2, BT_REMOVED = 3;     // basetrack.py TrackState (New = 0 never reaches the table)

struct BtHdr {
    int32_t n_tracked, n_lost, next_id, frame_id;   // list lengths; the id the next new track takes; updates done (frame_id of the last one)
    int32_t err;                    // 0 ok; 1 track slots exhausted (max_tracks); 3 an assignment problem beyond the LSAPs (extended side > 512)
    int32_t err_frame;              // group frame index the error was raised at
    int32_t n_fast, n_lsap;         // assignment problems settled by the unique-optimum check / by the LSAP, since creation
    int32_t max_side;               // largest extended side since creation (> 128: lsap_wave; beyond the LDS arena: matrix in HBM scratch)
};

struct BtTrack {                    // per slot
    int32_t id, state, act, start, end, cls;       // end = STrack.frame_id (end_frame)
    float score;
    int32_t pad;
};

struct BtParams {                   // every threshold rounded to fp32 once
    float track_thresh, low_thresh, new_thresh, match_thresh, second_thresh, unconf_thresh, dup_dist;
    int32_t max_lost;               // int(frame_rate / 30 * track_buffer)
    int32_t fuse;                   // fuse_score (= not mot20)
    int32_t cap;                    // slots (max_tracks <= TRK_DEV_TMAX)
    int32_t no_fast;                // 1: every assignment problem goes through the LSAP
};

struct BtTable {                    // device pointers into one allocation
    BtHdr* hdr;
    BtTrack* trk;
    int32_t* tl;
    int32_t* ll;
    float* mean;
    float* cov;
};

static inline size_t bt_table_bytes(int cap) {
    return 64 + (size_t)cap * (sizeof(BtTrack) + 8 + 4 * 8 + 4 * 64);
}
__host__ __device__ static inline BtTable bt_table(char* base, int cap) {
    BtTable t;
    t.hdr = reinterpret_cast<BtHdr*>(base);
    t.trk = reinterpret_cast<BtTrack*>(base + 64);
    t.tl = reinterpret_cast<int32_t*>(base + 64 + (size_t)cap * sizeof(BtTrack));
    t.ll = t.tl + cap;
    t.mean = reinterpret_cast<float*>(t.ll + cap);
    t.cov = t.mean + (size_t)cap * 8;
    return t;
}

// one launch, one block per stream of the bank (EpochCall, trk_dev.hpp); c.ext holds the extended matrices that do not fit the LDS
void launch_bytetrack_epoch(const BtParams& prm, const EpochCall& c, hipStream_t s);

}  // namespace aic
