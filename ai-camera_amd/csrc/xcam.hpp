// xcam.hpp -- cross-camera identities for the cameras of one tracker bank (xcam.cpp, C ABI aic_xcam_*; kernels_xcam.hip; DESIGN.md
// section 25).  What the gallery exchange of configs[4] does between ranks -- shard, all-gather, nearest rows, global ids -- inside one
// process: a link call packs every stream's shard on the device, finds every live row's nearest row of another stream, reads the
// tables back once and applies the global-id policy of global_id.cpp with world = streams.  The bank's per-stream association never
// reads the result.
//
// Device memory, allocated at the first pass: shards streams * t_max * (2 + dim) * 4 bytes (67 MB at 256 x 128 x 512), tables 20 bytes a row.
#pragma once
#include "archive.hpp"
#include "botsort_host.hpp"
#include "common.hpp"
#include "deepsort_bank.hpp"
#include "global_id.hpp"
#include "kernels.hpp"

namespace aic {

constexpr int XCAM_TMAX = TRK_DEV_TMAX;

// the checks of aic_xcam_create: nothing is touched before they pass
void xcam_check_params(int streams, int t_max, int dim, double max_cosine_distance);

struct XCam {
    Device* dev;
    int n_streams, t_max, dim, n;            // n = streams * t_max rows
    double max_cos;
    int tile = 0;                            // 32 / 64: that tile of the nearest kernel; 0: by size (tests, measurements)
    GidTable gid;
    DevBuf<float> d_shards;                  // [streams, t_max, 2 + dim]
    DevBuf<int> d_tab;                       // ids[n] | near_row[n] | near_dist[n] (float bits) | n_valid[streams] | flags[streams]
    DevBuf<unsigned long long> d_best;       // [n] keys of the nearest kernel
    PinBuf<int> h_tab;                       // the read-back of d_tab: the last pass's tables
    bool has_pass = false;
    // the identity archive (archive.hpp), not owned.  With one attached a pass ends with archive_step()
    Archive* archive = nullptr;
    int min_gap = 1;                         // an archived row answers a new track only when its last deposit is more than min_gap passes old
    int64_t passes = 0;                      // completed passes with an archive attached = the next pass's tick
    struct Returning { int32_t stream, track_id; int64_t archived_key; float dist; };
    std::vector<Returning> returning;        // the last pass's winners, ascending shard row

    XCam(Device& d, int streams, int t_max_, int dim_, double max_cosine_distance);
    void ensure();
    int* d_nvalid() const { return d_tab.p + 3 * (size_t)n; }
    int* d_flags() const { return d_nvalid() + n_streams; }
    const int* ids() const { return h_tab.p; }
    const int* near_row() const { return h_tab.p + n; }
    const float* near_dist() const { return reinterpret_cast<const float*>(h_tab.p + 2 * (size_t)n); }
    // d_shards, n_valid and flags are on their way (stream s): nearest rows, ONE read-back, ONE sync, then the policy on the host.
    // expect (may be NULL): the caller's n_valid, held against the device's counts before the policy sees the tables
    int pass(hipStream_t s, const int32_t* expect = nullptr);
    // after the policy: the pass's new rows against the archive (k = 1; the queries are the shard rows on the device), one winner per
    // archived row, link_keys for the winners, then every valid row of the pass is deposited
    void archive_step();
    int link(DeepSortBank& b);
    int link(BotSortTracker& b);
    int link_shards(const float* shards, const int32_t* n_valid, int mem);
};

}  // namespace aic

struct aic_xcam {
    aic::XCam x;
    aic_xcam(aic::Device& d, int streams, int t_max, int dim, double thr) : x(d, streams, t_max, dim, thr) {}
};
