// kernels_trk.hip -- batched Kalman filter (K7, K8, K12), IoU cost (K10), cosine-min over the
// per-track feature galleries (K9).  fp32 throughout, -ffp-contract=off.
//
// Reference arithmetic (all fp32, per track / per pair in Python loops):
//   KalmanFilter.initiate/predict/project/update/gating_distance
//       src/tracker/core/kalman_filter.py:55-83, 85-120, 122-151, 153-204, 206-249
//   iou / iou_cost                      src/tracker/core/matching.py:13-106
//   cosine_distance / appearance_cost   src/tracker/core/matching.py:109-217
//
// The arithmetic itself is trk_math.hpp's, the one copy every DeepSORT-family kernel calls: kf_*_wave (one wavefront = the 8x8
// covariance of a track, in place), mean_box, iou_dist, maha4, cos_tile / cos_tile_min.  predict is bit-exact with the reference;
// project/update/gating go through a 4x4 Cholesky like LAPACK's potrf + trtrs / potrs and agree to fp32 rounding.  This file holds
// the kernels around it: which track, measurement or tile a wave or thread takes, and where the result goes.
//
// Layout: state SoA in HBM, mean[slot][8], cov[slot][64]; one wavefront (64 lanes = the 8x8
// covariance) per track for predict/update, one thread per (track, detection) pair for gating/IoU.
#include "kernels.hpp"
#include "trk_math.hpp"

namespace aic {

__global__ void kf_initiate_kernel(const float* __restrict__ z, int n, float* mean, float* cov) {
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= n) return;
    kf_initiate_wave(cov + (size_t)k * 64, mean + (size_t)k * 8, z + (size_t)k * 4, threadIdx.x & 63);
}

__global__ void kf_predict_kernel(float* mean, float* cov, const int* slots, int n, float dt) {
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= n) return;
    const int slot = slots ? slots[k] : k;
    kf_predict_wave(cov + (size_t)slot * 64, mean + (size_t)slot * 8, threadIdx.x & 63, dt);
}

__global__ void kf_project_kernel(const float* __restrict__ mean, const float* __restrict__ cov, int n, float* pmean, float* pcov) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float* P = cov + (size_t)k * 64;
    const float* m = mean + (size_t)k * 8;
    float S[4][4];
    innovation_cov(P, m[3], S);
    for (int a = 0; a < 4; ++a) {
        pmean[(size_t)k * 4 + a] = m[a];
        for (int b = 0; b < 4; ++b) pcov[(size_t)k * 16 + a * 4 + b] = S[a][b];
    }
}

// grid.x = tracks, threads over measurements.
__global__ void kf_gating_kernel(const float* __restrict__ mean, const float* __restrict__ cov, const int* __restrict__ slots,
                                 int n, const float* __restrict__ zs, int m, int shared_z, int only_position, float* d2) {
    const int t = blockIdx.x;
    if (t >= n) return;
    const int slot = slots ? slots[t] : t;
    const float* P = cov + (size_t)slot * 64;
    const float* mu = mean + (size_t)slot * 8;
    float S[4][4], L[4][4];
    innovation_cov(P, mu[3], S);
    const bool ok = only_position ? cholesky<2>(S, L) : cholesky<4>(S, L);
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        const float* z = zs + (size_t)(shared_z ? j : (size_t)t * m + j) * 4;
        float acc;
        if (only_position) {   // the position block alone: this kernel is its only user
            float d[4], y[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) d[a] = z[a] - mu[a];
            fwd_solve<2>(L, d, y);
            acc = y[0] * y[0] + y[1] * y[1];
            if (!ok) acc = __builtin_inff();   // kalman_filter.py:241-247
        } else {
            acc = maha4(L, ok, mu, z);
        }
        d2[(size_t)t * m + j] = acc;
    }
}

// One wavefront per (track, measurement) pair: lane (i,j) owns P[i][j].
__global__ void kf_update_kernel(float* mean, float* cov, const float* __restrict__ z, int n) {
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= n) return;
    kf_update_wave(cov + (size_t)k * 64, mean + (size_t)k * 8, z + (size_t)k * 4, threadIdx.x & 63);
}

// 1 - IoU in tlwh (matching.py:13-106). Track boxes either given or derived from the state means.
__global__ void iou_cost_kernel(const float* __restrict__ trk_tlwh, const float* __restrict__ mean, const int* __restrict__ slots,
                                int t, const float* __restrict__ det, int n, float* cost) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= t * n) return;
    const int ti = idx / n, di = idx - ti * n;
    float b[4];
    if (trk_tlwh) {
        b[0] = trk_tlwh[ti * 4], b[1] = trk_tlwh[ti * 4 + 1], b[2] = trk_tlwh[ti * 4 + 2], b[3] = trk_tlwh[ti * 4 + 3];
    } else {
        mean_box(mean + (size_t)(slots ? slots[ti] : ti) * 8, b);
    }
    cost[idx] = iou_dist(b, det + (size_t)di * 4);
}

__global__ void fill_kernel(float* p, float v, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// rows / max(||row||, 1e-7)  (matching.py:126-130); one wavefront per row.
__global__ void normalize_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int n, int dim, const int* __restrict__ n_dev) {
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= (n_dev ? min(n, n_dev[0]) : n)) return;
    const int lane = threadIdx.x & 63;
    const float* s = src + (size_t)row * dim;
    float ss = 0.f;
    for (int c = lane; c < dim; c += 64) ss = ss + s[c] * s[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ss = ss + __shfl_xor(ss, o);
    const float nrm = fmaxf(sqrtf(ss), 1e-7f);
    for (int c = lane; c < dim; c += 64) dst[(size_t)row * dim + c] = s[c] / nrm;
}

// ------------------------------------------------------------------------------------------------
// Fused per-frame kernels of the tracker (one stream).

// cosine_min on the matrix cores: cost[t][n] = min_g max(0, 1 - <gal_n[t][g], det_n[n]>) with both
// operands ALREADY normalised (gallery rows at append time, detections once per launch group).
// One wave = 16 gallery rows x up to 32 detections (cos_tile); atomicMin on the fp32 bit pattern is
// order-preserving because every value is >= +0.
__global__ __launch_bounds__(256) void cosine_min_mfma_kernel(const float* __restrict__ gal_n, const int* __restrict__ slots,
                                                              const int* __restrict__ glen, int gmax, int dim,
                                                              const float* __restrict__ det_n, const unsigned char* __restrict__ has_feat,
                                                              int n, float* cost) {
    const int t = blockIdx.x;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int g0 = (blockIdx.y * 4 + wv) * 16;
    const int len = glen[t];
    if (g0 >= len) return;
    // rows / detections past the end are CLAMPED to a valid row instead of zero-filled: their products
    // are never read (the min below and the atomics are guarded), and the loads stay branch-free
    const float* grow = gal_n + ((size_t)slots[t] * gmax + min(g0 + r, len - 1)) * dim;
    unsigned int* out = reinterpret_cast<unsigned int*>(cost) + (size_t)t * n;
    // rows start at row * dim floats: 16-byte aligned only when dim % 4 == 0.  Otherwise (block-uniform) the element-guarded loop
    // walks all of K, k in the same order
    const bool vec = (dim & 3) == 0;
    for (int d0 = 0; d0 < n; d0 += 32) {
        const int da = d0 + r, db = d0 + 16 + r;
        const float* pa = det_n + (size_t)min(da, n - 1) * dim;
        const float* pb = det_n + (size_t)min(db, n - 1) * dim;
        const bool oka = da < n, okb = db < n;
        floatx4 acc0, acc1;
        cos_tile(grow, pa, pb, 0, dim, vec, q, acc0, acc1);
        float m0, m1;
        cos_tile_min(acc0, acc1, g0, q, len, m0, m1);
        if (q == 0) {
            if (oka && (!has_feat || has_feat[da])) atomicMin(out + da, __float_as_uint(m0));
            if (okb && (!has_feat || has_feat[db])) atomicMin(out + db, __float_as_uint(m1));
        }
    }
}

struct TrkCommit {   // per-track commit of the previous frame, folded into the next frame's association launch (kind == nullptr: none)
    const int* kind;      // 0 none, 1 Kalman update, 2 initiate
    const int* det;       // detection row (previous frame) for kind 1 / 2
    const int* kout;      // row of out_tlwh for kind 1
    const int* appos;     // gallery ring position to write, or -1
    const int* apdet;     // detection row whose feature is appended
    const float* xyah;    // previous frame's detections
    const float* feat; const float* feat_n;
    float* out_tlwh; float* gal_raw; float* gal_w;
};

// trk_assoc_all_kernel: ONE launch per frame for everything the host association needs about track t (one 1024-thread
// block per track): the lazy Kalman predict in place (kalman_filter.py:85-120), the squared Mahalanobis (kalman_filter.py:206-249) and
// 1-IoU (matching.py:13-106) rows (waves 0..1) and the
// appearance row of cosine_min_mfma_kernel -- wave pair w>>1 takes the 16-row gallery slices, each wave half of K, and the per-slice minima
// meet in LDS instead of atomicMin, so the three rows are plain stores and may go STRAIGHT to pinned host memory: no
// init pass, no second launch, no device-to-host blit on the per-frame chain.  Same products; the dot product is summed as
// two K halves (fp32 rounding differs from the one-pass kernel in the last bit).
__global__ __launch_bounds__(1024) void trk_assoc_all_kernel(float* mean, float* cov, const int* __restrict__ slots,
                                                             const int* __restrict__ glen, int do_predict,
                                                             const float* __restrict__ det_tlwh, const float* __restrict__ det_xyah,
                                                             const float* gal_n, int gmax, int dim,
                                                             const float* __restrict__ det_n, const unsigned char* __restrict__ has_feat,
                                                             int n, float* app, float* d2, float* iouc, TrkCommit cm) {
    // 16 waves: wave w = (gallery slice lane w>>1, K half w&1).  The two K halves of a slice meet in LDS (the chain is
    // latency-bound: half the dependent load batches per wave), then the per-slice minima meet in red[].
    extern __shared__ float red[];                     // [8][n] per-slice minima, then [8][64][8] partial sums
    float* part = red + 8 * n;
    const int t = blockIdx.x;
    const int slot = slots[t];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const bool two = blockDim.x == 1024;                // 16 waves: K split in halves; 8 waves: one wave per slice
    const int sl = two ? wv >> 1 : wv, ks = two ? wv & 1 : 0;
    float* P = cov + (size_t)slot * 64;
    float* m = mean + (size_t)slot * 8;
    // ---- commit of the PREVIOUS frame for this track (pipelined form: one launch per frame): Kalman update or initiate on
    // wave 0, the gallery row on the other waves; then the block continues with the next frame's rows
    if (cm.kind != nullptr) {
        const int kind = cm.kind[t];
        if (threadIdx.x < 64) {
            if (kind == 1) kf_update_box_wave(P, m, cm.xyah + (size_t)cm.det[t] * 4, lane, cm.out_tlwh + (size_t)cm.kout[t] * 4);
            else if (kind == 2) kf_initiate_wave(P, m, cm.xyah + (size_t)cm.det[t] * 4, lane);
        } else if (cm.appos[t] >= 0) {
            const size_t dst = ((size_t)slot * gmax + cm.appos[t]) * dim;
            const size_t src = (size_t)cm.apdet[t] * dim;
            for (int c = threadIdx.x - 64; c < dim; c += blockDim.x - 64) {
                cm.gal_raw[dst + c] = cm.feat[src + c];
                cm.gal_w[dst + c] = cm.feat_n[src + c];
            }
        }
        __syncthreads();                            // the block's own global writes are visible to all its waves from here on
        if (n <= 0) return;                         // (block-uniform) commit only: no next frame to prepare
    }
    if (do_predict && threadIdx.x < 64) kf_predict_wave(P, m, lane);
    // ---- appearance
    const int len = (gal_n != nullptr && dim > 0) ? glen[t] : 0;
    if (ks == 0)
        for (int j = lane; j < n; j += 64) red[sl * n + j] = 3.0e38f;
    const int kmid = two ? (dim / 2) / 64 * 64 : dim;   // K split on a 64-element boundary (the tail stays in the upper half)
    const int k_lo = ks ? kmid : 0, k_hi = ks ? dim : kmid;
    const bool vec = (dim & 3) == 0;                    // 16-byte row loads need dim % 4 == 0; else the element-guarded loop walks all of K
    for (int gb = 0; gb < len; gb += 128) {             // block-uniform trip counts: the barriers below are safe
        const int g0 = gb + sl * 16;
        const bool live = g0 < len;
        const float* grow = gal_n + ((size_t)slot * gmax + min(g0 + r, max(len - 1, 0))) * dim;
        for (int d0 = 0; d0 < n; d0 += 32) {
            const int da = d0 + r, db = d0 + 16 + r;
            floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
            if (live) cos_tile(grow, det_n + (size_t)min(da, n - 1) * dim, det_n + (size_t)min(db, n - 1) * dim, k_lo, k_hi, vec, q, acc0, acc1);
            float* ps = part + ((size_t)sl * 64 + lane) * 8;
            if (two) {
                if (ks == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ps[e] = acc0[e]; ps[4 + e] = acc1[e]; }
                }
                __syncthreads();
                if (ks == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { acc0[e] += ps[e]; acc1[e] += ps[4 + e]; }
                }
            }
            if (ks == 0 && live) {
                float m0, m1;
                cos_tile_min(acc0, acc1, g0, q, len, m0, m1);
                if (q == 0) {                       // this wave owns red[sl][*]
                    if (da < n) red[sl * n + da] = fminf(red[sl * n + da], m0);
                    if (db < n) red[sl * n + db] = fminf(red[sl * n + db], m1);
                }
            }
            if (two) __syncthreads();               // part[] is reused by the next tile
        }
    }
    __syncthreads();   // predict's global writes and every wave's minima are visible to the whole block
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        float v = 1e5f;                              // INFTY_COST (matching.py:148,175): empty gallery / featureless detection
        if (len > 0 && (!has_feat || has_feat[j])) {
            float mn = red[j];
#pragma unroll
            for (int w = 1; w < 8; ++w) mn = fminf(mn, red[w * n + j]);
            v = mn;
        }
        app[(size_t)t * n + j] = v;
    }
    // ---- gating distance + IoU rows (threads 0..127)
    if (threadIdx.x < 128) {
        float S[4][4], L[4][4], b[4];
        innovation_cov(P, m[3], S);
        const bool ok = cholesky<4>(S, L);
        mean_box(m, b);
        for (int j = threadIdx.x; j < n; j += 128) {
            const size_t o = (size_t)t * n + j;
            d2[o] = maha4(L, ok, m, det_xyah + (size_t)j * 4);
            iouc[o] = iou_dist(b, det_tlwh + (size_t)j * 4);
        }
    }
}

// trk_commit_kernel: one wavefront-sized block per work item, three roles by block index:
//   [0, M)        Kalman update of a matched track (kalman_filter.py:153-204) + its new tlwh
//   [M, M+U)      initiate a new track (kalman_filter.py:55-83)
//   [M+U, M+U+A)  append a feature to a gallery ring (track.py:70-74): raw row + normalised row
__global__ __launch_bounds__(64) void trk_commit_kernel(float* mean, float* cov, const int* __restrict__ lists, int M, int U, int A,
                                                        const float* __restrict__ xyah, float* out_tlwh, float* gal_raw, float* gal_n,
                                                        int gmax, int dim, const float* __restrict__ feat, const float* __restrict__ feat_n) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int* upd_slot = lists;
    const int* upd_det = lists + M;
    const int* ini_slot = lists + 2 * M;
    const int* ini_det = lists + 2 * M + U;
    const int* ap_slot = lists + 2 * M + 2 * U;
    const int* ap_pos = ap_slot + A;
    const int* ap_det = ap_pos + A;
    if (b < M) {
        kf_update_box_wave(cov + (size_t)upd_slot[b] * 64, mean + (size_t)upd_slot[b] * 8, xyah + (size_t)upd_det[b] * 4, lane, out_tlwh + (size_t)b * 4);
    } else if (b < M + U) {
        const int k = b - M;
        kf_initiate_wave(cov + (size_t)ini_slot[k] * 64, mean + (size_t)ini_slot[k] * 8, xyah + (size_t)ini_det[k] * 4, lane);
    } else {
        const int k = b - M - U;
        const size_t dst = ((size_t)ap_slot[k] * gmax + ap_pos[k]) * dim;
        const size_t src = (size_t)ap_det[k] * dim;
        for (int c = lane; c < dim; c += 64) {
            gal_raw[dst + c] = feat[src + c];
            gal_n[dst + c] = feat_n[src + c];
        }
    }
}

// ------------------------------------------------------------------------------------------------
void launch_kf_initiate(const float* z, int n, float* mean, float* cov, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(kf_initiate_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, z, n, mean, cov);
    KCHECK();
}
void launch_kf_predict(float* mean, float* cov, const int* slots, int n, hipStream_t s, float dt) {
    if (n <= 0) return;
    hipLaunchKernelGGL(kf_predict_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, mean, cov, slots, n, dt);
    KCHECK();
}
void launch_kf_project(const float* mean, const float* cov, int n, float* pmean, float* pcov, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(kf_project_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, s, mean, cov, n, pmean, pcov);
    KCHECK();
}
void launch_kf_update(float* mean, float* cov, const float* z, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(kf_update_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, mean, cov, z, n);
    KCHECK();
}
void launch_kf_gating(const float* mean, const float* cov, const int* slots, int n, const float* zs, int m, int shared_z,
                      int only_position, float* d2, hipStream_t s) {
    if (n <= 0 || m <= 0) return;
    hipLaunchKernelGGL(kf_gating_kernel, dim3(n), dim3(64), 0, s, mean, cov, slots, n, zs, m, shared_z, only_position, d2);
    KCHECK();
}
void launch_iou_cost(const float* trk_tlwh, const float* mean, const int* slots, int t, const float* det_tlwh, int n, float* cost, hipStream_t s) {
    if (t <= 0 || n <= 0) return;
    hipLaunchKernelGGL(iou_cost_kernel, dim3(ceil_div((long)t * n, 256)), dim3(256), 0, s, trk_tlwh, mean, slots, t, det_tlwh, n, cost);
    KCHECK();
}
void launch_fill(float* p, float v, size_t n, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(fill_kernel, dim3(ceil_div((long)n, 256)), dim3(256), 0, s, p, v, n);
    KCHECK();
}
void launch_normalize_rows(const float* src, float* dst, int n, int dim, hipStream_t s, const int* n_dev) {
    if (n <= 0) return;
    hipLaunchKernelGGL(normalize_rows_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, src, dst, n, dim, n_dev);
    KCHECK();
}

void launch_cosine_min_mfma(const float* gal_n, const int* slots, const int* glen, int t, int gmax, int dim, const float* det_n,
                            const unsigned char* has_feat, int n, float* cost, hipStream_t s) {
    if (t <= 0 || n <= 0 || gmax <= 0) return;
    hipLaunchKernelGGL(cosine_min_mfma_kernel, dim3(t, ceil_div(gmax, 64)), dim3(256), 0, s, gal_n, slots, glen, gmax, dim, det_n, has_feat, n, cost);
    KCHECK();
}
void launch_trk_assoc_all(float* mean, float* cov, const int* slots, const int* glen, int t, int do_predict, const float* det_tlwh,
                          const float* det_xyah, const float* gal_n, int gmax, int dim, const float* det_n,
                          const unsigned char* has_feat, int n, float* app, float* d2, float* iouc, hipStream_t s) {
    launch_trk_step(mean, cov, slots, glen, t, do_predict, det_tlwh, det_xyah, gal_n, gmax, dim, det_n, has_feat, n, app, d2, iouc,
                    nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, s);
}
void launch_trk_step(float* mean, float* cov, const int* slots, const int* glen, int t, int do_predict, const float* det_tlwh,
                     const float* det_xyah, const float* gal_n, int gmax, int dim, const float* det_n,
                     const unsigned char* has_feat, int n, float* app, float* d2, float* iouc,
                     const int* c_kind, const int* c_det, const int* c_kout, const int* c_appos, const int* c_apdet,
                     const float* c_xyah, const float* c_feat, const float* c_feat_n, float* c_out_tlwh, float* c_gal_raw, float* c_gal_w,
                     hipStream_t s) {
    if (t <= 0 || (n <= 0 && c_kind == nullptr)) return;
    const TrkCommit cm{c_kind, c_det, c_kout, c_appos, c_apdet, c_xyah, c_feat, c_feat_n, c_out_tlwh, c_gal_raw, c_gal_w};
    // (a K split over wave pairs -- 1024-thread blocks -- waited longer for a CU: 88 against 83 us of chain)
    hipLaunchKernelGGL(trk_assoc_all_kernel, dim3(t), dim3(512), ((size_t)8 * std::max(n, 0) + 8 * 64 * 8) * sizeof(float), s, mean, cov, slots, glen, do_predict,
                       det_tlwh, det_xyah, gal_n, gmax, dim, det_n, has_feat, n, app, d2, iouc, cm);
    KCHECK();
}
void launch_trk_commit(float* mean, float* cov, const int* lists, int M, int U, int A, const float* xyah, float* out_tlwh,
                       float* gal_raw, float* gal_n, int gmax, int dim, const float* feat, const float* feat_n, hipStream_t s) {
    if (M + U + A <= 0) return;
    hipLaunchKernelGGL(trk_commit_kernel, dim3(M + U + A), dim3(64), 0, s, mean, cov, lists, M, U, A, xyah, out_tlwh, gal_raw, gal_n, gmax, dim, feat, feat_n);
    KCHECK();
}

}  // namespace aic
