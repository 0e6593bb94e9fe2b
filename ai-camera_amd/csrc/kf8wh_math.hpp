// kf8wh_math.hpp -- arithmetic of BoT-SORT's tracker (kernels_botsort.hip; specification: tests/botsort_oracle.py): the 8-state constant
// velocity filter on [cx, cy, w, h, vcx, vcy, vw, vh] with noise scaled by w (x / w components) and h (y / h components), the camera-motion
// warp, and the ordered 64-lane sums of the appearance term.  fp32, -ffp-contract=off: every function is a fixed sequence of correctly
// rounded operations, the same sequence the oracle states.  This is NOT the xyah filter of trk_math.hpp (only its 4x4 Cholesky is shared).
//
// One wavefront = one track.  Lane (i, j) = (lane >> 3, lane & 7) holds p = P[i][j] and m = x[i]; what a lane needs of the others comes
// by __shfl, so predict -> warp -> update never leaves the registers.  All 64 lanes active.
#pragma once
#include <hip/hip_runtime.h>

#include "trk_math.hpp"

namespace aic {

constexpr float KF8_W_POS = 0.05f, KF8_W_VEL = 0.00625f;      // fp32(1 / 20), fp32(1 / 160)
constexpr float KF8_W_POS0 = 0.1f, KF8_W_VEL0 = 0.0625f;      // initiate: 2 / 20, 10 / 160

// KalmanFilter.initiate for the measurement z = [cx, cy, w, h]
__device__ __forceinline__ void kf8_initiate_wave(float& p, float& m, const float* z, int lane) {
    const int i = lane >> 3, j = lane & 7;
    const float side = (i & 1) ? z[3] : z[2];
    const float s = (i < 4 ? KF8_W_POS0 : KF8_W_VEL0) * side;
    p = i == j ? s * s : 0.f;
    m = i < 4 ? z[i] : 0.f;
}

// x = F x, P = F (P F^T) + Q, Q from the sides before the step
__device__ __forceinline__ void kf8_predict_wave(float& p, float& m, int lane) {
    const int i = lane >> 3, j = lane & 7;
    const float w = __shfl(m, 2 * 8), h = __shfl(m, 3 * 8);
    const float a = __shfl(p, (i << 3) + ((j + 4) & 7));
    const float t1 = j < 4 ? p + a : p;
    const float b = __shfl(t1, (((i + 4) & 7) << 3) + j);
    float t2 = i < 4 ? t1 + b : t1;
    const float s = (i < 4 ? KF8_W_POS : KF8_W_VEL) * ((i & 1) ? h : w);
    if (i == j) t2 = t2 + s * s;
    const float mv = __shfl(m, ((i + 4) & 7) << 3);
    if (i < 4) m = m + mv;
    p = t2;
}

// KalmanFilter.update with z = [cx, cy, w, h]: S = P[:4, :4] + R, K_i = S^-1 P[i, :4] by Cholesky, x += K y, P -= K (S K^T)
__device__ __forceinline__ void kf8_update_wave(float& p, float& m, const float* z, int lane) {
    const int i = lane >> 3, j = lane & 7;
    const float w = __shfl(m, 2 * 8), h = __shfl(m, 3 * 8);
    float S[4][4], L[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const float pab = __shfl(p, a * 8 + b);
            const float s = KF8_W_POS * ((a & 1) ? h : w);
            S[a][b] = a == b ? pab + s * s : pab;
        }
    cholesky<4>(S, L);
    float bi[4], bj[4], y[4], Ki[4], Kj[4], t[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        bi[a] = __shfl(p, i * 8 + a);
        bj[a] = __shfl(p, j * 8 + a);
        y[a] = z[a] - __shfl(m, a * 8);
    }
    fwd_solve<4>(L, bi, t); bwd_solve(L, t, Ki);
    fwd_solve<4>(L, bj, t); bwd_solve(L, t, Kj);
    float acc = 0.f, dot = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float u = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) u = u + S[a][c] * Kj[c];
        acc = acc + Ki[a] * u;
        dot = dot + Ki[a] * y[a];
    }
    p = p - acc;
    m = m + dot;
}

// Camera motion [R | t] (wp = r00 r01 t0 r10 r11 t1): x <- A x (+ t on cx, cy), P <- (A P) A^T with A = kron(I4, R), two-term sums
__device__ __forceinline__ void kf8_warp_wave(float& p, float& m, const float* wp, int lane) {
    const int i = lane >> 3, j = lane & 7;
    const float ra = wp[(i & 1) * 3], rb = wp[(i & 1) * 3 + 1];
    const float ca = wp[(j & 1) * 3], cb = wp[(j & 1) * 3 + 1];
    const float me = __shfl(m, (i & ~1) << 3), mo = __shfl(m, (i | 1) << 3);
    float mn = ra * me + rb * mo;
    if (i == 0) mn = mn + wp[2];
    if (i == 1) mn = mn + wp[5];
    const float pe = __shfl(p, ((i & ~1) << 3) + j), po = __shfl(p, ((i | 1) << 3) + j);
    const float T = ra * pe + rb * po;
    const float te = __shfl(T, (i << 3) + (j & ~1)), to = __shfl(T, (i << 3) + (j | 1));
    p = te * ca + to * cb;
    m = mn;
}

// ---- ordered sums over a feature vector (dim a multiple of 4, rows 16-byte aligned): lane l takes elements 256 c + 4 l + q in the order
// c, q; the 64 partial sums fold by a butterfly (32, 16, 8, 4, 2, 1), so every lane returns the same value
__device__ __forceinline__ float wave_fold(float acc) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
    return acc;
}
__device__ __forceinline__ float wave_dot(const float* a, const float* b, int dim, int lane) {
    float acc = 0.f;
    for (int e = lane * 4; e < dim; e += 256) {
        const float4 x = *reinterpret_cast<const float4*>(a + e), y = *reinterpret_cast<const float4*>(b + e);
        acc = acc + x.x * y.x;
        acc = acc + x.y * y.y;
        acc = acc + x.z * y.z;
        acc = acc + x.w * y.w;
    }
    return wave_fold(acc);
}

// STrack.update_features for a unit feature f: the first one is copied, later ones smooth <- alpha smooth + (1 - alpha) f, renormalised
__device__ __forceinline__ void feat_update_wave(float* smooth, const float* f, int dim, bool first, float alpha, float oma, int lane) {
    if (first) {
        for (int e = lane * 4; e < dim; e += 256) *reinterpret_cast<float4*>(smooth + e) = *reinterpret_cast<const float4*>(f + e);
        return;
    }
    float acc = 0.f;
    for (int e = lane * 4; e < dim; e += 256) {
        const float4 s = *reinterpret_cast<const float4*>(smooth + e), x = *reinterpret_cast<const float4*>(f + e);
        float4 r;
        r.x = alpha * s.x + oma * x.x, r.y = alpha * s.y + oma * x.y, r.z = alpha * s.z + oma * x.z, r.w = alpha * s.w + oma * x.w;
        acc = acc + r.x * r.x;
        acc = acc + r.y * r.y;
        acc = acc + r.z * r.z;
        acc = acc + r.w * r.w;
        *reinterpret_cast<float4*>(smooth + e) = r;
    }
    const float nrm = sqrtf(wave_fold(acc));
    for (int e = lane * 4; e < dim; e += 256) {                  // every lane re-reads what it wrote itself
        float4 r = *reinterpret_cast<const float4*>(smooth + e);
        r.x = r.x / nrm, r.y = r.y / nrm, r.z = r.z / nrm, r.w = r.w / nrm;
        *reinterpret_cast<float4*>(smooth + e) = r;
    }
}

}  // namespace aic
