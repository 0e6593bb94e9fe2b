// yuv.hpp -- 4:2:0 YUV (NV12, I420) <-> BGR24 over a bank of frames.  tests/yuv_oracle.py is the specification:
// integer arithmetic on 2^20-scaled coefficients, chroma replicated on decode and taken from the 2x2 block's sums on encode; the kernels
// (kernels_yuv.hip) equal it bit for bit.  The four coefficient tables live here, once.
#pragma once
#include "common.hpp"

namespace aic {

constexpr int YUV_SHIFT = 20;
constexpr int YUV_MAX_SIDE = 16384;

// decode: cy cvr cvg cug cub; encode: yr yg yb ur ug ub vr vg vb; y_offset: 16 (limited range) or 0 (full).  Passed to the kernels by value.
struct YuvCoeffs {
    int32_t dec[5];
    int32_t enc[9];
    int32_t y_offset;
};

// [matrix][range]: the standards' exact fractions times 2^20, rounded half away from zero (tests/test_yuv_oracle.py derives them again)
constexpr YuvCoeffs YUV_TABLES[2][2] = {
    {{{1220945, 1673555, -852458, -410793, 2115221}, {269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897}, 16},
     {{1048576, 1470104, -748826, -360853, 1858077}, {313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262}, 0}},
    {{{1220945, 1879825, -558796, -223607, 2215014}, {191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230}, 16},
     {{1048576, 1651297, -490864, -196424, 1945738}, {222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074}, 0}},
};

// A bank of 4:2:0 frames in memory: pitch and frame_stride resolved (never 0).
struct YuvLayout {
    int format, h, w;
    size_t pitch, frame_stride;
    size_t frame_bytes() const { return pitch * h * 3 / 2; }                                     // one frame without the stride's tail
    size_t bank_bytes(int n) const { return n <= 0 ? 0 : (size_t)(n - 1) * frame_stride + frame_bytes(); }
};

// Every rejection of aic_frames_to_bgr / aic_frames_from_bgr but the NULL pointers, before the device is touched (throws AIC_ERR_INVALID).
YuvLayout yuv_layout(int n_frames, int h, int w, int format, int64_t pitch, int64_t frame_stride);
const YuvCoeffs& yuv_coeffs(int matrix, int range);

// n frames: src (layout L) -> dst BGR [n, h, w, 3] tight, and back (only the bytes inside w are written).  Device pointers of any alignment:
// the launchers pick 8-byte, 4-byte or byte accesses from the pointers, w and the strides; every path writes the same bytes.
void launch_yuv_to_bgr(const uint8_t* src, int n, const YuvLayout& L, const YuvCoeffs& c, uint8_t* dst_bgr, hipStream_t s);
void launch_bgr_to_yuv(const uint8_t* src_bgr, int n, const YuvLayout& L, const YuvCoeffs& c, uint8_t* dst, hipStream_t s);

}  // namespace aic
