// kernels_overlay.hip -- box / label / info-panel overlay on a frame resident in HBM.
//
// Reference: draw_tracks / draw_detections / draw_info_panel of src/utils/visualization.py:9-124,170-228, called per frame at
// src/aicamera_tracker.py:211-223 (outside its FPS span) -- cv2.rectangle(thickness 2), a filled label bar above the box,
// white cv2.putText in FONT_HERSHEY_SIMPLEX, drawn track after track (a later track paints over an earlier one).
// cv2's line and glyph rasterisers are not in /root/reference, so the PIXELS are this build's own integer spec (parity
// unpinned against cv2; oracle/overlay_oracle.py restates it and the kernel matches it bit for bit):
//   kind 0  outline, thickness 2: the two-pixel ring x in {x0-1, x0} u {x1, x1+1} or y in {y0-1, y0} u {y1, y1+1} of the box
//   kind 1  filled rectangle, corners inclusive
//   kind 2  text: 5x7 bitmap glyphs (ASCII 32..126) scaled by s, cell advance 6s, top-left corner (x0, y0)
// Painter's order = list order: a pixel takes the colour of the LAST primitive that covers it, else stays -- evaluated per
// pixel (one thread per pixel walks the list backwards), so the result does not depend on scheduling.  HBM-bound: 3 bytes
// read + 3 written per touched pixel; the primitive list (a few KB) sits in LDS.
#include "common.hpp"
#include "font5x7.hpp"

namespace aic {

struct Prim { int kind, x0, y0, x1, y1, color, toff, tlen_scale; };   // color = B | G << 8 | R << 16; tlen_scale = len | scale << 16

__global__ __launch_bounds__(256) void overlay_kernel(unsigned char* __restrict__ frame, int h, int w, const Prim* __restrict__ prims, int n,
                                                      const unsigned char* __restrict__ text) {
    extern __shared__ Prim sp[];
    for (int i = threadIdx.x; i < n; i += blockDim.x) sp[i] = prims[i];
    __syncthreads();
    const int x = blockIdx.x * 32 + (threadIdx.x & 31), y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= w || y >= h) return;
    for (int i = n - 1; i >= 0; --i) {
        const Prim p = sp[i];
        bool hit = false;
        if (p.kind == 1) {
            hit = x >= p.x0 && x <= p.x1 && y >= p.y0 && y <= p.y1;
        } else if (p.kind == 0) {
            const bool outer = x >= p.x0 - 1 && x <= p.x1 + 1 && y >= p.y0 - 1 && y <= p.y1 + 1;
            const bool inner = x > p.x0 && x < p.x1 && y > p.y0 && y < p.y1;
            hit = outer && !inner;
        } else {
            const int s = p.tlen_scale >> 16, len = p.tlen_scale & 0xffff;
            const int dx = x - p.x0, dy = y - p.y0;
            if (dx >= 0 && dy >= 0 && dy < 7 * s && dx < 6 * s * len) {
                const int ci = dx / (6 * s), gx = (dx - ci * 6 * s) / s, gy = dy / s;
                const int ch = text[p.toff + ci];
                if (gx < 5 && ch >= 32 && ch <= 126) hit = (kFont5x7[(ch - 32) * 5 + gx] >> gy) & 1;
            }
        }
        if (hit) {
            unsigned char* o = frame + ((size_t)y * w + x) * 3;
            o[0] = (unsigned char)(p.color & 255), o[1] = (unsigned char)((p.color >> 8) & 255), o[2] = (unsigned char)((p.color >> 16) & 255);
            return;
        }
    }
}

void launch_overlay(unsigned char* frame, int h, int w, const int* prims, int n, const unsigned char* text, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(overlay_kernel, dim3(ceil_div(w, 32), ceil_div(h, 8)), dim3(256), (size_t)n * sizeof(Prim), s, frame, h, w,
                       reinterpret_cast<const Prim*>(prims), n, text);
    KCHECK();
}

}  // namespace aic

using namespace aic;

extern "C" int aic_overlay(int device_id, uint8_t* frame_bgr, int h, int w, int mem, const int32_t* prims, int n, const uint8_t* text,
                           int text_bytes) {
    return guarded([&] {
        AIC_REQUIRE(frame_bgr && h > 0 && w > 0 && n >= 0 && n <= 1500, AIC_ERR_INVALID, "bad argument (at most 1500 primitives per call)");
        if (n == 0) return;
        AIC_REQUIRE(prims && (text || text_bytes == 0), AIC_ERR_INVALID, "NULL argument");
        for (int i = 0; i < n; ++i) {
            const int32_t* p = prims + (size_t)i * 8;
            AIC_REQUIRE(p[0] >= 0 && p[0] <= 2, AIC_ERR_INVALID, "unknown primitive kind");
            if (p[0] == 2) AIC_REQUIRE(p[6] >= 0 && (p[7] >> 16) >= 1 && p[6] + (p[7] & 0xffff) <= text_bytes, AIC_ERR_INVALID, "text range outside the buffer");
        }
        Device& d = device(device_id);
        d.use();
        hipStream_t s = d.s_main;
        DevBuf<int> dp((size_t)n * 8);
        DevBuf<uint8_t> dt((size_t)std::max(text_bytes, 1));
        HIP_CHECK(hipMemcpyAsync(dp.p, prims, (size_t)n * 32, hipMemcpyHostToDevice, s));
        if (text_bytes) HIP_CHECK(hipMemcpyAsync(dt.p, text, (size_t)text_bytes, hipMemcpyHostToDevice, s));
        const size_t fb = (size_t)h * w * 3;
        if (mem == AIC_DEVICE) {
            launch_overlay(frame_bgr, h, w, dp.p, n, dt.p, s);
        } else {
            DevBuf<uint8_t> df(fb);
            HIP_CHECK(hipMemcpyAsync(df.p, frame_bgr, fb, hipMemcpyHostToDevice, s));
            launch_overlay(df.p, h, w, dp.p, n, dt.p, s);
            HIP_CHECK(hipMemcpyAsync(frame_bgr, df.p, fb, hipMemcpyDeviceToHost, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}
