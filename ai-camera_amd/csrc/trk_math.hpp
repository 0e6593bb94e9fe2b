// trk_math.hpp -- the arithmetic of the DeepSORT-family tracker kernels, once (kernels_trk.hip: one launch per frame; kernels_trk_dev.hip:
// association on the device, k frames per launch; kernels_bytetrack.hip): the xyah Kalman filter, the Mahalanobis gate, the box of a mean,
// 1 - IoU and the 16 x 32 cosine tile.  fp32, -ffp-contract=off.
//   src/tracker/core/kalman_filter.py:55-83 (initiate), :85-120 (predict), :122-151 (project), :153-204 (update), :206-249 (gating)
//   src/tracker/core/track.py:133-151 (to_tlwh), src/tracker/core/matching.py:13-106 (iou), :136-141 (cosine distance)
// Noise terms follow NumPy 2.x scalar promotion: std = fp32(weight) * h in fp32, squared in fp64, rounded once.
// The scalar pieces (TRK_HD) need nothing but <cmath>, so a stand-alone program builds them with the system compiler
// (tests/trk_math_probe.cpp); the wave wrappers and the MFMA tile are device code.
#pragma once
#if defined(__HIPCC__)
#include "kernels.hpp"
#define TRK_HD __host__ __device__ __forceinline__
#else
#include <cmath>
#define TRK_HD inline
#endif

namespace aic {

TRK_HD float sq64(float s) { return (float)((double)s * (double)s); }

#define W_POS 0.05f       /* fp32(1/20)   kalman_filter.py:52  */
#define W_VEL 0.00625f    /* fp32(1/160)  kalman_filter.py:53  */

TRK_HD float q_diag(int i, float h) {   // process noise, kalman_filter.py:99-112
    if (i == 2) return (float)(1e-2 * 1e-2);
    if (i == 6) return (float)(1e-5 * 1e-5);
    return sq64((i < 4 ? W_POS : W_VEL) * h);
}
TRK_HD float r_diag(int i, float h) {   // measurement noise, kalman_filter.py:136-143
    if (i == 2) return (float)(1e-1 * 1e-1);
    return sq64(W_POS * h);
}

// S = H P H^T + R (4x4, symmetric) and its lower Cholesky factor. Returns false if not PD.
TRK_HD void innovation_cov(const float* P, float h, float S[4][4]) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) S[a][b] = P[a * 8 + b] + (a == b ? r_diag(a, h) : 0.f);
}
template <int N>
TRK_HD bool cholesky(const float S[4][4], float L[4][4]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float d = S[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        if (!(d > 0.f)) ok = false;
        const float ljj = sqrtf(d);
        L[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            float s = S[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            L[i][j] = s / ljj;
        }
    }
    return ok;
}
template <int N>
TRK_HD void fwd_solve(const float L[4][4], const float b[4], float y[4]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float s = b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s / L[i][i];
    }
}
TRK_HD void bwd_solve(const float L[4][4], const float y[4], float x[4]) {   // L^T x = y
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        float s = y[i];
#pragma unroll
        for (int k = i + 1; k < 4; ++k) s = s - L[k][i] * x[k];
        x[i] = s / L[i][i];
    }
}

// ---- the update's pieces (kalman_filter.py:185-202), shared by the wave form (kf_update_lane: every lane works out rows i and j) and the
// thread-per-row form of trk_epoch_kernel (gain row, S K and the mean element once per (track, row), then kf_cov_elem per element)
// row i of K = (S^-1 (P H^T)^T)^T: the two triangular solves on row i of P H^T
TRK_HD void kf_gain_row(const float L[4][4], const float* P, int i, float Ki[4]) {
    float b[4], y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) b[a] = P[i * 8 + a];
    fwd_solve<4>(L, b, y);
    bwd_solve(L, y, Ki);
}
TRK_HD void kf_s_gain(const float S[4][4], const float K[4], float u[4]) {   // S K[j]^T
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) s = s + S[a][c] * K[c];
        u[a] = s;
    }
}
TRK_HD float kf_cov_elem(float pij, const float Ki[4], const float SKj[4]) {   // (P - K (S K^T))[i][j]
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) acc = acc + Ki[a] * SKj[a];
    return pij - acc;
}
TRK_HD float kf_mean_elem(const float* m, const float* zz, const float Ki[4], int i) {   // (mean + K (z - H mean))[i]
    float dot = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) dot = dot + Ki[a] * (zz[a] - m[a]);
    return m[i] + dot;
}

// ---- one lane (i, j) = element P[i][j] of the 8x8 covariance: what the lane will hold, without writing.  mi = mean element i.
// (They take i and j, not the lane: trk_epoch_kernel sits at its 256 VGPRs, and with the lane split inside them its allocation spills one.)
// Predict (kalman_filter.py:85-120): bit-exact with the reference (F P F^T has at most two non-zero terms per element and multi_dot
// evaluates F (P F^T)).  dt: KalmanFilter(dt) (kalman_filter.py:34-44), fp32 like the reference's motion matrix; x * 1.0f == x, so dt = 1
// keeps its bits.  mi is worked out by the lanes j == 0 only.
TRK_HD void kf_predict_lane(const float* P, const float* m, int i, int j, float dt, float& pij, float& mi) {
    const float h = m[3];
    float t1 = P[i * 8 + j];                       // T1 = P F^T ; T2 = F T1
    if (j < 4) t1 = t1 + P[i * 8 + j + 4] * dt;
    float t2 = t1;
    if (i < 4) {
        float u = P[(i + 4) * 8 + j];
        if (j < 4) u = u + P[(i + 4) * 8 + j + 4] * dt;
        t2 = t1 + u * dt;
    }
    if (i == j) t2 = t2 + q_diag(i, h);
    pij = t2;
    mi = 0.f;
    if (j == 0) { mi = m[i]; if (i < 4) mi = mi + m[i + 4] * dt; }
}
// Update with measurement zz (xyah) (kalman_filter.py:153-204)
TRK_HD void kf_update_lane(const float* P, const float* m, const float* zz, int i, int j, float& pij, float& mi) {
    float S[4][4], L[4][4], Ki[4], Kj[4], u[4];
    innovation_cov(P, m[3], S);
    cholesky<4>(S, L);
    kf_gain_row(L, P, i, Ki);
    kf_gain_row(L, P, j, Kj);
    kf_s_gain(S, Kj, u);
    pij = kf_cov_elem(P[i * 8 + j], Ki, u);
    mi = kf_mean_elem(m, zz, Ki, i);
}
// KalmanFilter.initiate (kalman_filter.py:55-83) for measurement zz (xyah)
TRK_HD void kf_initiate_lane(const float* zz, int i, int j, float& pij, float& mi) {
    const float h = zz[3];
    float v = 0.f;
    if (i == j) {   // kalman_filter.py:72-82
        if (i == 2) v = (float)(1e-2 * 1e-2);
        else if (i == 6) v = (float)(1e-5 * 1e-5);
        else v = sq64((i < 4 ? 0.1f : 0.0625f) * h);
    }
    pij = v;
    mi = i < 4 ? zz[i] : 0.f;
}

// Track.to_tlwh of a mean (track.py:133-151): w = a h while h > 0, else 0 with h clamped at 0
TRK_HD void mean_box(const float* m, float b[4]) {
    const float cx = m[0], cy = m[1], ar = m[2];       // (all loads first: b may alias m for all the compiler knows)
    float bw = 0.f, bh = m[3];
    if (bh > 0.f) bw = ar * bh; else bh = fmaxf(0.f, bh);
    b[0] = cx - bw / 2.0f, b[1] = cy - bh / 2.0f, b[2] = bw, b[3] = bh;
}

// 1 - IoU of box b against candidate c (tlwh), matching.py:13-106 (union floored at 1e-7)
TRK_HD float iou_dist(const float* b, const float* c) {
    const float brx = b[0] + b[2], bry = b[1] + b[3];
    const float crx = c[0] + c[2], cry = c[1] + c[3];
    const float iw = fmaxf(0.f, fminf(brx, crx) - fmaxf(b[0], c[0]));
    const float ih = fmaxf(0.f, fminf(bry, cry) - fmaxf(b[1], c[1]));
    const float inter = iw * ih;
    const float uni = b[2] * b[3] + c[2] * c[3] - inter;
    return 1.0f - inter / fmaxf(uni, 1e-7f);
}

// squared Mahalanobis distance of measurement z (xyah) to the mean m, all four components, through the Cholesky factor L of S;
// +inf when S is not positive definite (pd = what cholesky<4> returned), kalman_filter.py:206-249
TRK_HD float maha4(const float L[4][4], bool pd, const float* m, const float* z) {
    float d[4], y[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) d[a] = z[a] - m[a];
    fwd_solve<4>(L, d, y);
    float acc = y[0] * y[0];
    acc = acc + y[1] * y[1];
    acc = acc + y[2] * y[2];
    acc = acc + y[3] * y[3];
    return pd ? acc : __builtin_inff();
}

TRK_HD float cos_dist(float dot) {       // matching.py:136-141
    const float x = 1.0f - dot;
    return x > 0.f ? x : 0.f;
}

#if defined(__HIPCC__)
// ---- one wavefront = one track, lane (i, j) = element P[i][j] (state in global or LDS memory), in place.
// The fence is synchronisation, not arithmetic: a lane reads elements of P and m that OTHER lanes overwrite, the wave runs in lock-step but
// its loads are asynchronous, so every lane must hold its operands before anyone stores.  It lives here so that every caller gets it.
__device__ __forceinline__ void kf_store_wave(float* P, float* m, int lane, float pij, float mi) {
    __builtin_amdgcn_s_waitcnt(0);
    P[lane] = pij;
    if ((lane & 7) == 0) m[lane >> 3] = mi;
}
__device__ __forceinline__ void kf_predict_wave(float* P, float* m, int lane, float dt = 1.0f) {
    float pij, mi;
    kf_predict_lane(P, m, lane >> 3, lane & 7, dt, pij, mi);
    kf_store_wave(P, m, lane, pij, mi);
}
// returns the updated mean element i of lane (i, *)
__device__ __forceinline__ float kf_update_wave(float* P, float* m, const float* zz, int lane) {
    float pij, mi;
    kf_update_lane(P, m, zz, lane >> 3, lane & 7, pij, mi);
    kf_store_wave(P, m, lane, pij, mi);
    return mi;
}
// the update and, from lane 0, the tlwh of the updated mean to box[4]
__device__ __forceinline__ void kf_update_box_wave(float* P, float* m, const float* zz, int lane, float* box) {
    const float mi = kf_update_wave(P, m, zz, lane);
    const float mu[4] = {__shfl(mi, 0), __shfl(mi, 8), __shfl(mi, 16), __shfl(mi, 24)};
    if (lane == 0) mean_box(mu, box);
}
__device__ __forceinline__ void kf_initiate_wave(float* P, float* m, const float* zz, int lane) {   // reads neither P nor m: no fence
    float pij, mi;
    kf_initiate_lane(zz, lane >> 3, lane & 7, pij, mi);
    P[lane] = pij;
    if ((lane & 7) == 0) m[lane >> 3] = mi;
}

// ---- cosine distances on the matrix cores.  v_mfma_f32_16x16x4_f32: exact fp32 fmaf chain.  One wave = 16 gallery rows x 32 detections
// (rows pa: detections d0 + r, pb: d0 + 16 + r), both operands ALREADY normalised; lane (r, q) streams 16 bytes of its row per 16-deep K
// slice and MFMA e consumes element e of both operands (k = 16 kb + 4 q + e on both sides, so the contraction index matches).  K runs over
// [k_lo, k_hi), k ascending.  vec (wave-uniform): rows are 16-byte aligned (dim % 4 == 0) and the first loop may take 64 elements per step
// with 12 independent 16-byte loads in flight per lane; the element-guarded loop then takes the tail, or all of K, in the same order.
typedef float floatx4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void cos_tile(const float* __restrict__ grow, const float* __restrict__ pa, const float* __restrict__ pb,
                                         int k_lo, int k_hi, bool vec, int q, floatx4& acc0, floatx4& acc1) {
    acc0 = floatx4{0.f, 0.f, 0.f, 0.f};
    acc1 = acc0;
    int k0 = k_lo;
    for (; vec && k0 + 64 <= k_hi; k0 += 64) {
        floatx4 a[4], b0[4], b1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 16 * u + 4 * q;
            a[u] = *reinterpret_cast<const floatx4*>(grow + k);
            b0[u] = *reinterpret_cast<const floatx4*>(pa + k);
            b1[u] = *reinterpret_cast<const floatx4*>(pb + k);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b0[u][e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][e], b1[u][e], acc1, 0, 0, 0);
            }
    }
    for (; k0 < k_hi; k0 += 16) {                // tail: any dimension, element-guarded
        const int k = k0 + 4 * q;
        floatx4 a = {0.f, 0.f, 0.f, 0.f}, b0 = a, b1 = a;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (k + e < k_hi) { a[e] = grow[k + e]; b0[e] = pa[k + e]; b1[e] = pb[k + e]; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b0[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b1[e], acc1, 0, 0, 0);
        }
    }
}

// D[row = gallery g0 + 4q + e][col = detection r] of a tile: the distance of each of its two detections to the nearest of the tile's
// live gallery rows (< len), the same value in the four lanes (r, *)
__device__ __forceinline__ void cos_tile_min(const floatx4& acc0, const floatx4& acc1, int g0, int q, int len, float& m0, float& m1) {
    m0 = 3.0e38f, m1 = 3.0e38f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (g0 + 4 * q + e < len) {
            m0 = fminf(m0, cos_dist(acc0[e]));
            m1 = fminf(m1, cos_dist(acc1[e]));
        }
    }
    m0 = fminf(m0, __shfl_xor(m0, 16)); m0 = fminf(m0, __shfl_xor(m0, 32));
    m1 = fminf(m1, __shfl_xor(m1, 16)); m1 = fminf(m1, __shfl_xor(m1, 32));
}
#endif  // __HIPCC__

}  // namespace aic
