// kf7_math.hpp -- arithmetic of OC-SORT's tracker (kernels_ocsort.hip; specification: tests/ocsort_oracle.py): SORT's 7-state constant
// velocity filter on [x, y, s, r, vx, vy, vs], the box conversions, the IoU and the fp32 asin of the OCM term.  fp32, -ffp-contract=off:
// every function is a fixed sequence of correctly rounded operations, the same sequence the oracle states.  The scalar part compiles
// for the host as well; the wave part (one wavefront = one track, the covariance in registers) is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "trk_math.hpp"

namespace aic {

constexpr int KF7_NEW = 0, KF7_OBSERVED = 1, KF7_FROZEN = 2;   // never updated / last update was an observation / frozen at the first miss

__host__ __device__ inline float kf7_q(int i) { return i < 4 ? 1.0f : i < 6 ? 0.01f : 1e-4f; }        // Q = diag(1, 1, 1, 1, .01, .01, 1e-4)
__host__ __device__ inline float kf7_r(int a) { return a < 2 ? 1.0f : 10.0f; }                        // R = diag(1, 1, 10, 10)
__host__ __device__ inline float kf7_p0(int i) { return i < 4 ? 10.0f : 1e4f; }                       // P0 = diag(10 x4, 1e4 x3)

// asin on [-1, 1] (Cephes asinf): the one transcendental of the tracker.  Max error against fp64 asin 1.64e-7, odd, non-decreasing.
__host__ __device__ inline float asin32(float x) {
    const float a = fabsf(x);
    const bool big = a > 0.5f;
    const float z = big ? 0.5f * (1.0f - a) : a * a;
    const float t = big ? sqrtf(z) : a;
    float p = 4.2163199048e-2f * z + 2.4181311049e-2f;
    p = p * z + 4.5470025998e-2f;
    p = p * z + 7.4953002686e-2f;
    p = p * z + 1.6666752422e-1f;
    p = (p * z) * t + t;
    if (big) p = 1.5707963267948966f - (p + p);
    return x < 0.f ? -p : p;
}

// convert_bbox_to_z: xyxy -> [x, y, s, r], r = w / (h + 1e-6)
__host__ __device__ inline void bbox_to_z(const float* b, float z[4]) {
    const float w = b[2] - b[0], h = b[3] - b[1];
    z[0] = b[0] + w / 2.0f, z[1] = b[1] + h / 2.0f, z[2] = w * h, z[3] = w / (h + 1e-6f);
}
// convert_x_to_bbox: w = sqrt(s r), h = s / w
__host__ __device__ inline void x_to_bbox(float x, float y, float s, float r, float b[4]) {
    const float w = sqrtf(s * r), h = s / w;
    b[0] = x - w / 2.0f, b[1] = y - h / 2.0f, b[2] = x + w / 2.0f, b[3] = y + h / 2.0f;
}
__host__ __device__ inline float iou_xyxy(const float* a, const float* b) {
    const float iw = fmaxf(0.f, fminf(a[2], b[2]) - fmaxf(a[0], b[0]));
    const float ih = fmaxf(0.f, fminf(a[3], b[3]) - fmaxf(a[1], b[1]));
    const float inter = iw * ih;
    const float uni = (a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter;
    return inter / fmaxf(uni, 1e-7f);
}
// speed_direction: unit (dy, dx) from the centre of a to the centre of b
__host__ __device__ inline void speed_direction(const float* a, const float* b, float v[2]) {
    const float cx1 = (a[0] + a[2]) / 2.0f, cy1 = (a[1] + a[3]) / 2.0f;
    const float cx2 = (b[0] + b[2]) / 2.0f, cy2 = (b[1] + b[3]) / 2.0f;
    const float dy = cy2 - cy1, dx = cx2 - cx1;
    const float norm = sqrtf(dx * dx + dy * dy) + 1e-6f;
    v[0] = dy / norm, v[1] = dx / norm;
}

#if defined(__HIPCC__)
// One wavefront = one track.  Lane (i, j) = (lane >> 3, lane & 7) holds p = P[i][j] (0 where i or j is 7) and m = x[i]; what a lane needs of
// the others comes by __shfl, so a chain of predicts and updates (the ORU replay) never leaves the registers.  All 64 lanes active.

// x = F x, P = F (P F^T) + Q
__device__ __forceinline__ void kf7_predict_wave(float& p, float& m, int lane) {
    const int i = lane >> 3, j = lane & 7;
    const float a = __shfl(p, (i << 3) + ((j + 4) & 7));
    const float t1 = j < 3 ? p + a : p;
    const float b = __shfl(t1, (((i + 4) & 7) << 3) + j);
    float t2 = i < 3 ? t1 + b : t1;
    if (i == j && i < 7) t2 = t2 + kf7_q(i);
    const float mv = __shfl(m, ((i + 4) & 7) << 3);
    if (i < 3) m = m + mv;
    p = i < 7 && j < 7 ? t2 : 0.f;
}

// Joseph-form update with z = [x, y, s, r]: K_i = S^-1 P[i, :4] by Cholesky, x += K y, P = (I - KH) P (I - KH)^T + K R K^T, each product an
// ordered sum over the four measured states
__device__ __forceinline__ void kf7_update_wave(float& p, float& m, const float z[4], int lane) {
    const int i = lane >> 3, j = lane & 7;
    float Pab[4][4], S[4][4], L[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            Pab[a][b] = __shfl(p, a * 8 + b);
            S[a][b] = a == b ? Pab[a][b] + kf7_r(a) : Pab[a][b];
        }
    cholesky<4>(S, L);
    float bi[4], bj[4], paj[4], y[4], Ki[4], Kj[4], t[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        bi[a] = __shfl(p, i * 8 + a);
        bj[a] = __shfl(p, j * 8 + a);
        paj[a] = __shfl(p, a * 8 + j);
        y[a] = z[a] - __shfl(m, a * 8);
    }
    fwd_solve<4>(L, bi, t); bwd_solve(L, t, Ki);
    fwd_solve<4>(L, bj, t); bwd_solve(L, t, Kj);
    float dot = Ki[0] * y[0] + Ki[1] * y[1];
    dot = dot + Ki[2] * y[2];
    dot = dot + Ki[3] * y[3];
    m = m + dot;
    float acc = Ki[0] * paj[0] + Ki[1] * paj[1];                  // (I - KH) P, element (i, j) ...
    acc = acc + Ki[2] * paj[2];
    acc = acc + Ki[3] * paj[3];
    const float Bij = p - acc;
    float Bib[4];                                                 // ... and elements (i, 0..3)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        float s = Ki[0] * Pab[0][b] + Ki[1] * Pab[1][b];
        s = s + Ki[2] * Pab[2][b];
        s = s + Ki[3] * Pab[3][b];
        Bib[b] = bi[b] - s;
    }
    float c = Bib[0] * Kj[0] + Bib[1] * Kj[1];
    c = c + Bib[2] * Kj[2];
    c = c + Bib[3] * Kj[3];
    float k = (Ki[0] * kf7_r(0)) * Kj[0] + (Ki[1] * kf7_r(1)) * Kj[1];
    k = k + (Ki[2] * kf7_r(2)) * Kj[2];
    k = k + (Ki[3] * kf7_r(3)) * Kj[3];
    const float pn = (Bij - c) + k;
    p = i < 7 && j < 7 ? pn : 0.f;
}
#endif

}  // namespace aic
