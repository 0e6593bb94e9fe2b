// gmc.hpp -- camera-motion estimation on the device (kernels_gmc.hip, gmc.cpp): integer block matching on a gray pyramid level and a
// robust similarity fit per frame.  The specification is tests/gmc_oracle.py; every constant below is named there.
#pragma once
#include "common.hpp"

namespace aic {

constexpr int GMC_R = 8;               // search radius and grid origin (gray pixels)
constexpr int GMC_B = 16;              // block side
constexpr int GMC_TEX_MIN = 256;
constexpr int GMC_START_GATE = 64;     // 1/16 gray pixel
constexpr int GMC_MAX_BLOCKS = 2048;   // per frame (the fit kernel keeps them in LDS): 1920 x 1080 at s = 2 has 1947
constexpr int GMC_SKIPPED = INT32_MIN; // dx of a block that did not enter the fit

struct GmcGeom {
    int h = 0, w = 0, s = 0;           // frame size, downscale (2 or 4)
    int gh = 0, gw = 0;                // gray level size
    int nbx = 0, nby = 0, nb = 0;      // block grid
    size_t level = 0;                  // bytes between the gray levels of consecutive frames (gh * gw rounded up to 16)
};

inline GmcGeom gmc_geom(int h, int w, int s) {
    GmcGeom g;
    g.h = h, g.w = w, g.s = s, g.gh = h / s, g.gw = w / s;
    g.nby = g.gh >= 2 * GMC_B ? (g.gh - 2 * GMC_B) / GMC_B + 1 : 0;
    g.nbx = g.gw >= 2 * GMC_B ? (g.gw - 2 * GMC_B) / GMC_B + 1 : 0;
    g.nb = g.nbx * g.nby;
    g.level = ((size_t)g.gh * g.gw + 15) / 16 * 16;
    return g;
}

// gray[f] = level of frames[f], f in [0, k)
void launch_gmc_gray(const uint8_t* frames, int k, const GmcGeom& g, uint8_t* gray, hipStream_t s);
// disp[f, b] = (dx, dy) of block b of frame f in 1/16 gray pixel, dx = GMC_SKIPPED for a block that is skipped or discarded.  The k
// frames are tick-major over `streams` streams (frame t * streams + q = tick t of stream q).  The predecessor of frame f is
// gray[f - streams]; of frame f < streams it is level f of `prev_bank` where have[f] != 0 (device memory, one byte per stream), and
// every block of that frame is skipped where it is 0.  boxes: rows frame_d0[f] .. + frame_n[f] of `boxes` (xyxy, or tlwh with
// x2 = x + w in fp32); frame_n NULL = no boxes.
void launch_gmc_match(const uint8_t* gray, const uint8_t* prev_bank, const uint8_t* have, int streams, int k, const GmcGeom& g,
                      const int32_t* frame_n, const int32_t* frame_d0, const float* boxes, bool tlwh, int32_t* disp, hipStream_t s);
// warps[f, 6], stats[f, 4] = ok, blocks, kept, inliers
void launch_gmc_fit(const int32_t* disp, int k, const GmcGeom& g, int min_inliers, float* warps, int32_t* stats, hipStream_t s);

// The estimator of `streams` video streams whose frames come tick-major: the results of a call and every stream's gray level carried
// over from the last tick of the call before.  One stream is the bank of one.
struct CameraMotionEstimator {
    Device* dev;
    GmcGeom g;
    int min_inliers;
    int streams;
    std::vector<uint8_t> have;     // host mirror of d_have
    DevBuf<uint8_t> d_prev, d_have, d_gray, d_frames;   // d_prev: [streams] levels; d_have: [streams] 1 = the stream has a carried level
    DevBuf<int32_t> d_disp, d_stats, d_cnt;
    DevBuf<float> d_warps, d_boxes;
    int cap_frames = 0;            // frames d_disp / d_warps / d_stats hold
    int last_frames = 0;           // frames of the last match_fit (rows of d_warps / d_stats that are current)

    CameraMotionEstimator(Device& d, int h, int w, int s, int min_inl, int streams = 1);
    void reset(int stream);        // the stream's next frame is its first (ordered on the tracker stream, where match_fit runs)
    void ensure(int k);
    // match + fit over k gray levels (launch_gmc_gray's output; whole ticks, tick-major) against the carried levels, results in d_warps /
    // d_stats; keeps the last tick's levels (contiguous: one copy).  The caller syncs s between calls (the buffers may grow).
    void match_fit(const uint8_t* levels, int k, const int32_t* frame_n, const int32_t* frame_d0, const float* boxes, bool tlwh, hipStream_t s);
    void estimate_batch(const uint8_t* frames, int k, int mem, const int32_t* counts, const float* boxes_xyxy, float* warps_out,
                        int32_t* stats_out);
};

}  // namespace aic

struct aic_gmc {
    aic::CameraMotionEstimator e;
    aic_gmc(aic::Device& d, int h, int w, int s, int min_inl) : e(d, h, w, s, min_inl) {}
};
struct aic_gmc_bank {
    aic::CameraMotionEstimator e;
    aic_gmc_bank(aic::Device& d, int h, int w, int s, int min_inl, int streams) : e(d, h, w, s, min_inl, streams) {}
};
