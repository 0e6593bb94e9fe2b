// gmc.cpp -- the camera-motion estimator object (buffers, the carried gray level, launches) and its C ABI.  There is no host
// implementation of the algorithm: it runs in kernels_gmc.hip or the call raises.
#include "gmc.hpp"

#include <algorithm>
#include <vector>

namespace aic {

CameraMotionEstimator::CameraMotionEstimator(Device& d, int h, int w, int s, int min_inl, int n_streams)
    : dev(&d), g(gmc_geom(h, w, s)), min_inliers(min_inl), streams(n_streams), have(n_streams, 0) {
    dev->use();
    d_prev.alloc(g.level * streams);
    d_have.alloc(streams);
    HIP_CHECK(hipMemsetAsync(d_have.p, 0, streams, dev->s_trk));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void CameraMotionEstimator::reset(int stream) {
    AIC_REQUIRE(stream >= 0 && stream < streams, AIC_ERR_INVALID, "stream outside the bank");
    dev->use();
    have[stream] = 0;
    HIP_CHECK(hipMemsetAsync(d_have.p + stream, 0, 1, dev->s_trk));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
}

void CameraMotionEstimator::ensure(int k) {
    if (k <= cap_frames) return;
    d_disp.alloc((size_t)k * g.nb * 2);
    d_warps.alloc((size_t)k * 6);
    d_stats.alloc((size_t)k * 4);
    cap_frames = k;
}

void CameraMotionEstimator::match_fit(const uint8_t* levels, int k, const int32_t* frame_n, const int32_t* frame_d0, const float* boxes,
                                      bool tlwh, hipStream_t s) {
    AIC_REQUIRE(k > 0 && k % streams == 0, AIC_ERR_INVALID, "camera motion takes whole ticks of every stream");
    ensure(k);
    launch_gmc_match(levels, d_prev.p, d_have.p, streams, k, g, frame_n, frame_d0, boxes, tlwh, d_disp.p, s);
    launch_gmc_fit(d_disp.p, k, g, min_inliers, d_warps.p, d_stats.p, s);
    HIP_CHECK(hipMemcpyAsync(d_prev.p, levels + (size_t)(k - streams) * g.level, g.level * streams, hipMemcpyDeviceToDevice, s));
    if (std::find(have.begin(), have.end(), 0) != have.end()) {   // a first tick only: every stream has a carried level from here on
        HIP_CHECK(hipMemsetAsync(d_have.p, 1, streams, s));
        std::fill(have.begin(), have.end(), 1);
    }
    last_frames = k;
}

void CameraMotionEstimator::estimate_batch(const uint8_t* frames, int k, int mem, const int32_t* counts, const float* boxes_xyxy,
                                           float* warps_out, int32_t* stats_out) {
    dev->use();
    if (k == 0) return;
    hipStream_t s = dev->s_trk;
    const size_t fb = (size_t)g.h * g.w * 3;
    HIP_CHECK(hipStreamSynchronize(s));           // buffers of the call before may be reallocated below
    d_gray.ensure((size_t)k * g.level);
    const uint8_t* src = frames;
    if (mem == AIC_HOST) {
        d_frames.ensure((size_t)k * fb);
        HIP_CHECK(hipMemcpyAsync(d_frames.p, frames, (size_t)k * fb, hipMemcpyHostToDevice, s));
        src = d_frames.p;
    }
    const int32_t* d_n = nullptr;
    if (counts && boxes_xyxy) {
        std::vector<int32_t> h(2 * (size_t)k);
        long total = 0;
        for (int f = 0; f < k; ++f) { h[f] = counts[f], h[k + f] = (int32_t)total; total += counts[f]; }
        d_cnt.ensure(2 * (size_t)k);
        d_boxes.ensure((size_t)std::max(total, 1L) * 4);
        HIP_CHECK(hipMemcpyAsync(d_cnt.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, s));
        if (total) HIP_CHECK(hipMemcpyAsync(d_boxes.p, boxes_xyxy, (size_t)total * 16, hipMemcpyHostToDevice, s));
        HIP_CHECK(hipStreamSynchronize(s));       // `h` is pageable and leaves scope
        d_n = d_cnt.p;
    }
    launch_gmc_gray(src, k, g, d_gray.p, s);
    match_fit(d_gray.p, k, d_n, d_n ? d_cnt.p + k : nullptr, d_boxes.p, false, s);
    if (warps_out) HIP_CHECK(hipMemcpyAsync(warps_out, d_warps.p, (size_t)k * 24, hipMemcpyDeviceToHost, s));
    if (stats_out) HIP_CHECK(hipMemcpyAsync(stats_out, d_stats.p, (size_t)k * 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
}

}  // namespace aic

using namespace aic;

extern "C" {

// Parameter checks of aic_gmc_create / aic_gmc_bank_create: nothing is touched before they pass.  Returns the downscale.
static int gmc_checked(int height, int width, const aic_gmc_params* p) {
    AIC_REQUIRE(p->downscale == 0 || p->downscale == 2 || p->downscale == 4, AIC_ERR_INVALID, "downscale must be 2 or 4 (0 = 4)");
    AIC_REQUIRE(p->min_inliers >= 0, AIC_ERR_INVALID, "min_inliers must be >= 0 (0 = 8)");
    AIC_REQUIRE(height > 0 && width > 0 && height <= 16384 && width <= 16384, AIC_ERR_INVALID, "bad frame size");
    const int s = p->downscale ? p->downscale : 4;
    const GmcGeom g = gmc_geom(height, width, s);
    AIC_REQUIRE(g.nb >= 1, AIC_ERR_INVALID, "frame smaller than one block plus its search margin (32 * downscale pixels a side)");
    AIC_REQUIRE(g.nb <= GMC_MAX_BLOCKS, AIC_ERR_INVALID, "more than 2048 blocks per frame: use downscale 4");
    return s;
}

static void gmc_estimate_checked(CameraMotionEstimator& e, const uint8_t* frames_bgr, int k, int mem, const int32_t* counts,
                                 const float* boxes_xyxy, float* warps_out, int32_t* stats_out) {
    AIC_REQUIRE(k >= 0 && (k == 0 || frames_bgr), AIC_ERR_INVALID, "NULL argument / negative frame count");
    AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(!boxes_xyxy || counts, AIC_ERR_INVALID, "boxes without counts");
    if (counts && boxes_xyxy)
        for (int f = 0; f < k; ++f) AIC_REQUIRE(counts[f] >= 0, AIC_ERR_INVALID, "negative box count");
    e.estimate_batch(frames_bgr, k, mem, counts, boxes_xyxy, warps_out, stats_out);
}

int aic_gmc_create(int device_id, int height, int width, const aic_gmc_params* p, aic_gmc** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        const int s = gmc_checked(height, width, p);
        *out = new aic_gmc(device(device_id), height, width, s, p->min_inliers ? p->min_inliers : 8);
    });
}

int aic_gmc_destroy(aic_gmc* g) {
    return guarded([&] {
        if (g) { g->e.dev->use(); (void)hipStreamSynchronize(g->e.dev->s_trk); }
        delete g;
    });
}

int aic_gmc_reset(aic_gmc* g) {
    return guarded([&] {
        AIC_REQUIRE(g, AIC_ERR_INVALID, "NULL estimator");
        g->e.reset(0);
    });
}

int aic_gmc_estimate_batch(aic_gmc* g, const uint8_t* frames_bgr, int k, int mem, const int32_t* counts, const float* boxes_xyxy,
                           float* warps_out, int32_t* stats_out) {
    return guarded([&] {
        AIC_REQUIRE(g, AIC_ERR_INVALID, "NULL argument / negative frame count");
        gmc_estimate_checked(g->e, frames_bgr, k, mem, counts, boxes_xyxy, warps_out, stats_out);
    });
}

// ---- banks
int aic_gmc_bank_create(int device_id, int height, int width, const aic_gmc_params* p, int streams, aic_gmc_bank** out) {
    return guarded([&] {
        AIC_REQUIRE(p && out, AIC_ERR_INVALID, "NULL argument");
        const int s = gmc_checked(height, width, p);
        AIC_REQUIRE(streams >= 1 && streams <= 256, AIC_ERR_INVALID, "streams must be in 1..256");
        *out = new aic_gmc_bank(device(device_id), height, width, s, p->min_inliers ? p->min_inliers : 8, streams);
    });
}

int aic_gmc_bank_destroy(aic_gmc_bank* b) {
    return guarded([&] {
        if (b) { b->e.dev->use(); (void)hipStreamSynchronize(b->e.dev->s_trk); }
        delete b;
    });
}

int aic_gmc_bank_reset(aic_gmc_bank* b, int stream) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL estimator");
        b->e.reset(stream);
    });
}

int aic_gmc_bank_estimate(aic_gmc_bank* b, const uint8_t* frames_bgr, int ticks, int mem, const int32_t* counts, const float* boxes_xyxy,
                          float* warps_out, int32_t* stats_out) {
    return guarded([&] {
        AIC_REQUIRE(b, AIC_ERR_INVALID, "NULL argument / negative frame count");
        AIC_REQUIRE(ticks >= 0 && ticks <= (1 << 24) / b->e.streams, AIC_ERR_INVALID, "NULL argument / negative frame count");
        gmc_estimate_checked(b->e, frames_bgr, ticks * b->e.streams, mem, counts, boxes_xyxy, warps_out, stats_out);
    });
}

}  // extern "C"
