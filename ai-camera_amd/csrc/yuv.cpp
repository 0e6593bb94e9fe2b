// yuv.cpp -- the argument checks of the pixel-format conversions (yuv.hpp) and their C ABI.  Every argument is checked before the device is
// touched; the pixels are written by kernels_yuv.hip or the call raises.
#include "yuv.hpp"

#include <algorithm>

namespace aic {

YuvLayout yuv_layout(int n_frames, int h, int w, int format, int64_t pitch, int64_t frame_stride) {
    AIC_REQUIRE(format == AIC_PIX_NV12 || format == AIC_PIX_I420, AIC_ERR_INVALID, "format must be AIC_PIX_NV12 or AIC_PIX_I420");
    AIC_REQUIRE(n_frames >= 0, AIC_ERR_INVALID, "n_frames is negative");
    AIC_REQUIRE(h >= 2 && h <= YUV_MAX_SIDE && w >= 2 && w <= YUV_MAX_SIDE, AIC_ERR_INVALID, "h and w must be in 2..16384");
    AIC_REQUIRE(h % 2 == 0 && w % 2 == 0, AIC_ERR_INVALID, "4:2:0 frames have an even h and w");
    AIC_REQUIRE(pitch >= 0 && frame_stride >= 0, AIC_ERR_INVALID, "pitch and frame_stride must not be negative (0 = tight)");
    if (pitch == 0) pitch = w;
    AIC_REQUIRE(pitch >= w, AIC_ERR_INVALID, "pitch is smaller than w");
    AIC_REQUIRE(format != AIC_PIX_I420 || pitch % 2 == 0, AIC_ERR_INVALID, "an I420 pitch must be even (the chroma rows are pitch / 2 bytes)");
    YuvLayout L{format, h, w, (size_t)pitch, 0};
    L.frame_stride = frame_stride ? (size_t)frame_stride : L.frame_bytes();
    AIC_REQUIRE(L.frame_stride >= L.frame_bytes(), AIC_ERR_INVALID, "frame_stride is shorter than pitch * h * 3 / 2");
    return L;
}

const YuvCoeffs& yuv_coeffs(int matrix, int range) {
    AIC_REQUIRE(matrix == AIC_YUV_BT601 || matrix == AIC_YUV_BT709, AIC_ERR_INVALID, "matrix must be AIC_YUV_BT601 or AIC_YUV_BT709");
    AIC_REQUIRE(range == AIC_YUV_LIMITED || range == AIC_YUV_FULL, AIC_ERR_INVALID, "range must be AIC_YUV_LIMITED or AIC_YUV_FULL");
    return YUV_TABLES[matrix][range];
}

namespace {

// to_bgr: the YUV bank is the source, else the destination
void convert(int device_id, bool to_bgr, const uint8_t* src, uint8_t* dst, int n, int h, int w, int format, int64_t pitch, int64_t frame_stride,
             int matrix, int range, int mem) {
    AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(device_id >= 0, AIC_ERR_INVALID, "device id out of range");
    const YuvLayout L = yuv_layout(n, h, w, format, pitch, frame_stride);
    const YuvCoeffs& c = yuv_coeffs(matrix, range);
    AIC_REQUIRE(n == 0 || (src && dst), AIC_ERR_INVALID, "NULL argument");
    if (n == 0) return;
    Device& dev = device(device_id);
    dev.use();
    hipStream_t st = dev.s_main;
    const size_t yb = L.bank_bytes(n), bb = (size_t)n * h * w * 3;
    DevBuf<uint8_t> d_yuv, d_bgr;                  // host memory: staged through these
    if (mem == AIC_DEVICE) {
        Prof pr(dev, PROF_MISC, st, 0.0, (double)n * h * w * 4.5);       // aic_prof_enable: the kernel alone, timed with events (tools/ingest_bench.py)
        if (to_bgr) launch_yuv_to_bgr(src, n, L, c, dst, st);
        else launch_bgr_to_yuv(src, n, L, c, dst, st);
    } else if (to_bgr) {
        d_yuv.alloc(yb), d_bgr.alloc(bb);
        HIP_CHECK(hipMemcpyAsync(d_yuv.p, src, yb, hipMemcpyHostToDevice, st));
        launch_yuv_to_bgr(d_yuv.p, n, L, c, d_bgr.p, st);
        HIP_CHECK(hipMemcpyAsync(dst, d_bgr.p, bb, hipMemcpyDeviceToHost, st));
    } else {
        d_yuv.alloc(yb), d_bgr.alloc(bb);
        HIP_CHECK(hipMemcpyAsync(d_bgr.p, src, bb, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_yuv.p, dst, yb, hipMemcpyHostToDevice, st));      // the pitch padding comes back as it was
        launch_bgr_to_yuv(d_bgr.p, n, L, c, d_yuv.p, st);
        HIP_CHECK(hipMemcpyAsync(dst, d_yuv.p, yb, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace

}  // namespace aic

using namespace aic;

extern "C" {

int aic_yuv_coeffs(int matrix, int range, int32_t dec[5], int32_t enc[9], int32_t* y_offset) {
    return guarded([&] {
        const YuvCoeffs& c = yuv_coeffs(matrix, range);
        AIC_REQUIRE(dec && enc && y_offset, AIC_ERR_INVALID, "NULL argument");
        std::copy(c.dec, c.dec + 5, dec);
        std::copy(c.enc, c.enc + 9, enc);
        *y_offset = c.y_offset;
    });
}

int aic_frames_to_bgr(int device, const uint8_t* src, int n_frames, int h, int w, int format, int64_t pitch, int64_t frame_stride, int matrix,
                      int range, int mem, uint8_t* dst_bgr) {
    return guarded([&] { convert(device, true, src, dst_bgr, n_frames, h, w, format, pitch, frame_stride, matrix, range, mem); });
}

int aic_frames_from_bgr(int device, const uint8_t* src_bgr, int n_frames, int h, int w, int format, int64_t pitch, int64_t frame_stride,
                        int matrix, int range, int mem, uint8_t* dst) {
    return guarded([&] { convert(device, false, src_bgr, dst, n_frames, h, w, format, pitch, frame_stride, matrix, range, mem); });
}

}  // extern "C"
