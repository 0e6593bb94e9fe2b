// kernels_botsort.hip -- BoT-SORT with ReID on the device, k frames per launch (structures: botsort.hpp).
//
// Specification: BoTSORT.update() of the BoT-SORT authors (tracker/bot_sort.py, matching.py, kalman_filter.py) as restated in
// tests/botsort_oracle.py, with the deliberate changes listed there.  The life cycle and the assignment are byte_epoch.hpp's (shared with
// ByteTrack); this file is the BoT-SORT variant of it: the xywh measurement and box, the filter, the warp and the ordered feature sums of
// kf8wh_math.hpp through the registers of a wavefront, the appearance pass over the cost matrix of stages 1 and 3
// (cost = min(fused IoU distance, gated appearance distance)), the camera-motion warp of pool and unconfirmed tracks, and every track of
// the tracked list as output.  A committed match of stages 1 and 3 and a new track take the detection's feature into the slot's
// smoothed vector in HBM.
#include "kernels.hpp"
#include "trk_dev.hpp"
#include "kf8wh_math.hpp"
#include "trk_wave.hpp"
#include "botsort.hpp"
#include "byte_epoch.hpp"

namespace aic {

struct BsArgs {
    EpochCall c;                    // stream s: bs_table(c.bank + s * c.table_stride, cap, smooth + s * smooth_stride)
    float* smooth;                  // [streams][cap][dim] smoothed unit features
    size_t smooth_stride;           // floats between two streams' features
    const float* warps;             // [rows, 6], indexed like c.dets.frame_n / c.out
    BsParams prm;
    int lds_bytes;
};

namespace {

struct BsLds : ByteLds {
    int *hasf, *dhas;               // a slot / a detection of the frame has a feature
};

struct BsVariant {
    using Args = BsArgs;
    using Lds = BsLds;
    using Table = BsTable;
    struct Ctx {
        bool reid;                  // the call has features and the tracker reads them
        long long* cyc;             // shader clocks of the appearance passes (__shared__)
        long long t_all;            // clock at the kernel's start
    };
    static constexpr size_t EXTRA_LDS_BYTES = 2 * 4 * (size_t)TRK_DEV_NMAX;
    static __device__ __forceinline__ void carve_extra(Lds& L, LdsTake& take) {
        L.hasf = (int*)take(4 * (size_t)TRK_DEV_NMAX);
        L.dhas = (int*)take(4 * (size_t)TRK_DEV_NMAX);
    }
    static __device__ __forceinline__ Table table(const Args& a, int sid) {
        return bs_table(a.c.bank + (size_t)sid * a.c.table_stride, a.prm.cap, a.smooth + (size_t)sid * a.smooth_stride);
    }
    static __device__ __forceinline__ float high(const BsParams& P) { return P.high; }
    static __device__ __forceinline__ float low(const BsParams& P) { return P.low; }
    static __device__ __forceinline__ void detection(const Lds& L, const Args& a, Ctx& x, int i, int row, float bx, float by, float w, float h) {
        L.meas[i * 4 + 0] = bx + w / 2.0f, L.meas[i * 4 + 1] = by + h / 2.0f, L.meas[i * 4 + 2] = w, L.meas[i * 4 + 3] = h;
        // a row that did not normalise to finite values is no feature: botsort_normalize_kernel leaves a NaN in its element 0
        L.dhas[i] = x.reid && (a.c.dets.valid == nullptr || a.c.dets.valid[row] != 0) && !isnan(a.c.dets.feat_n[(size_t)row * a.prm.dim]);
    }
    // track box: [cx - w / 2, cy - h / 2, w, h]
    static __device__ __forceinline__ void mean_box(const float* m, float b[4]) {
        b[0] = m[0] - m[2] / 2.0f, b[1] = m[1] - m[3] / 2.0f, b[2] = m[2], b[3] = m[3];
    }
    static __device__ __forceinline__ void zero_velocity(float* m) { m[6] = 0.f, m[7] = 0.f; }

    // the filter of slot sl through the registers of one wavefront (mean in LDS, covariance in HBM)
    template <class F>
    static __device__ __forceinline__ void kf_slot(const Lds& L, float* cov, int sl, int lane, F f) {
        float p = cov[(size_t)sl * 64 + lane], m = L.mean[sl * 8 + (lane >> 3)];
        f(p, m);
        cov[(size_t)sl * 64 + lane] = p;
        if ((lane & 7) == 0) L.mean[sl * 8 + (lane >> 3)] = m;
    }
    // predict the pool, then the camera-motion warp of pool and unconfirmed (which are not predicted)
    static __device__ __forceinline__ void predict(const Lds& L, const Args& a, const Table& tbl, int f, int np, int nun) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const float* wp = a.warps ? a.warps + (size_t)f * 6 : nullptr;
        for (int r = wv; r < np; r += NW)
            kf_slot(L, tbl.cov, L.pool[r], lane, [&](float& p, float& m) {
                kf8_predict_wave(p, m, lane);
                if (wp) kf8_warp_wave(p, m, wp, lane);
            });
        if (wp)
            for (int r = wv; r < nun; r += NW) kf_slot(L, tbl.cov, L.unc[r], lane, [&](float& p, float& m) { kf8_warp_wave(p, m, wp, lane); });
    }
    // The appearance term, for the pairs that pass the proximity veto (taken on the IoU distance before score fusion) and have a feature on
    // both sides: a wavefront takes 64 pairs, finds the ones that need a dot product and walks them, 16-byte loads straight from HBM / L2.
    // Non-finite features (tests/botsort_oracle.py, change 7): a detection whose normalised row is not finite in every element has no
    // feature (detection() above), so it is never compared, never enters a smoothed vector and does not set has_feat; it still matches
    // by IoU.  No NaN therefore reaches a dot product from a detection's side, where fmaxf would turn it into a distance of 0.
    static __device__ __forceinline__ void cost_pass(const Lds& L, const Args& a, const Table& tbl, Ctx& x, float* ext, int S, const int* rows, int nr,
                                                     const int* cols, int nc, int d0, bool app) {
        if (!(app && x.reid)) return;
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const long long t_cost = threadIdx.x == 0 ? clock64() : 0;
        const int dim = a.prm.dim;
        for (int base = wv * 64; base < nr * nc; base += NW * 64) {
            const int q = base + lane;
            bool need = false;
            int r = 0, c = 0;
            if (q < nr * nc) {
                r = q / nc, c = q - r * nc;
                const int j = cols[c];
                if (L.hasf[rows[r]] && L.dhas[j]) {
                    float b[4];
                    mean_box(L.mean + rows[r] * 8, b);
                    need = !(iou_dist(b, L.tlwh + j * 4) > a.prm.proximity);
                }
            }
            unsigned long long todo = __ballot(need);
            float mine = 0.f;
            while (todo) {
                const int bit = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int q2 = base + bit, r2 = q2 / nc, c2 = q2 - r2 * nc;
                const float d = wave_dot(tbl.feat + (size_t)rows[r2] * dim, a.c.dets.feat_n + (size_t)(d0 + cols[c2]) * dim, dim, lane);
                if (lane == bit) mine = d;
            }
            if (need) {
                const float e = fmaxf(0.f, 1.0f - mine) / 2.0f;
                if (e <= a.prm.appearance) ext[r * S + c] = fminf(ext[r * S + c], e);
            }
        }
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x == 0) *x.cyc += clock64() - t_cost;       // the pass as the block sees it: thread 0's share and its wait at the barrier
    }
    // count the pairs of the assignment whose cost is the appearance distance (cost < fused IoU distance)
    static __device__ __forceinline__ void post_solve(const Lds& L, Ctx& x, const float* ext, int S, const int* rows, int nr, const int* cols, bool fuse,
                                                      bool app) {
        const int tid = threadIdx.x;
        if (app && x.reid && tid < nr && L.mrow[tid] >= 0) {
            const int c = L.mrow[tid];
            if (ext[tid * S + c] < byte_cost<BsVariant>(L, rows[tid], cols[c], fuse)) atomicAdd(&L.wcnt[NW + BW_APP], 1);
        }
        __syncthreads();
    }
    // Kalman update and feature update of the matched rows: one wavefront per row
    static __device__ __forceinline__ void commit(const Lds& L, const Args& a, const Table& tbl, Ctx& x, const int* rows, int nr, const int* cols, int d0,
                                                  bool app) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const bool feats = app && x.reid;
        for (int r = wv; r < nr; r += NW) {
            const int c = L.mrow[r];
            if (c < 0) continue;
            const int sl = rows[r], j = cols[c];
            kf_slot(L, tbl.cov, sl, lane, [&](float& p, float& m) { kf8_update_wave(p, m, L.meas + j * 4, lane); });
            if (feats && L.dhas[j])
                feat_update_wave(tbl.feat + (size_t)sl * a.prm.dim, a.c.dets.feat_n + (size_t)(d0 + j) * a.prm.dim, a.prm.dim, !L.hasf[sl],
                                 a.prm.alpha, a.prm.one_minus_alpha, lane);
        }
        __threadfence_block();
        __syncthreads();
        if (feats && threadIdx.x < nr && L.mrow[threadIdx.x] >= 0 && L.dhas[cols[L.mrow[threadIdx.x]]]) L.hasf[rows[threadIdx.x]] = 1;
        __syncthreads();
    }
    static __device__ __forceinline__ void activate(const Lds& L, int sl, int j) { L.hasf[sl] = L.dhas[j]; }
    static __device__ __forceinline__ void initiate(const Lds& L, const Args& a, const Table& tbl, int nnew, int d0) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, dim = a.prm.dim;
        for (int r = wv; r < nnew; r += NW) {
            const int sl = L.fre[r], j = L.newd[r];
            kf_slot(L, tbl.cov, sl, lane, [&](float& p, float& m) { kf8_initiate_wave(p, m, L.meas + j * 4, lane); });
            if (L.dhas[j]) feat_update_wave(tbl.feat + (size_t)sl * dim, a.c.dets.feat_n + (size_t)(d0 + j) * dim, dim, true, 0.f, 0.f, lane);
        }
    }
    // every track of the tracked list
    static __device__ __forceinline__ int outputs(const Lds& L, int ntl, const int*& list) {
        list = L.tl;
        return ntl;
    }
    static __device__ __forceinline__ void load_slot(const Lds& L, const Table& tbl, int i) { L.hasf[i] = tbl.hasf[i]; }
    static __device__ __forceinline__ void store_slot(const Lds& L, const Table& tbl, int i) { tbl.hasf[i] = L.hasf[i]; }
    static __device__ __forceinline__ void begin(const Lds& L, Ctx& x) { *x.cyc = 0; L.wcnt[NW + BW_APP] = 0; }
    static __device__ __forceinline__ void finish(BsHdr* h, const Lds& L, Ctx& x) {
        h->n_app += L.wcnt[NW + BW_APP];
        h->cyc_cost += *x.cyc, h->cyc_all += clock64() - x.t_all;
    }
};
static_assert(byte_arena_floats<BsVariant>() == 11504, "the LDS arena of the BoT-SORT kernel: extended sides up to 107");

}  // namespace

__global__ __launch_bounds__(TRK_DEV_TMAX) void botsort_epoch_kernel(BsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ BsLds s_lds;
    __shared__ long long s_cyc;
    BsVariant::Ctx x{a.prm.reid && a.c.dets.feat_n != nullptr, &s_cyc, clock64()};
    byte_epoch<BsVariant>(a, smem, s_lds, x);
}

// out[r] = in[r] / |in[r]|: one wavefront per row, four rows per block.  A row with an element that is not finite after the division (a
// zero row: 0 / 0; an overflowed element: inf / inf beside zeros) is marked by a NaN in its element 0, the flag BsVariant::detection reads
__global__ __launch_bounds__(256) void botsort_normalize_kernel(const float* in, float* out, int rows, int dim) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* x = in + (size_t)r * dim;
    const float nrm = sqrtf(wave_dot(x, x, dim, lane));
    bool finite = true;
    for (int e = lane * 4; e < dim; e += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + e);
        v.x = v.x / nrm, v.y = v.y / nrm, v.z = v.z / nrm, v.w = v.w / nrm;
        finite = finite && isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
        *reinterpret_cast<float4*>(out + (size_t)r * dim + e) = v;
    }
    if (__any(!finite) && lane == 0) out[(size_t)r * dim] = __builtin_nanf("");      // lane 0 wrote element 0 above: program order
}

void launch_botsort_epoch(const BsParams& prm, const EpochCall& c, float* smooth, size_t smooth_stride, const float* warps, hipStream_t s) {
    set_lds_limit(botsort_epoch_kernel, BYTE_LDS_BYTES);
    BsArgs a{c, smooth, smooth_stride, warps, prm, BYTE_LDS_BYTES};
    // one block per stream; 512 threads (__launch_bounds__) and 159 KB of dynamic LDS keep it at one block per CU
    hipLaunchKernelGGL(botsort_epoch_kernel, dim3(c.streams), dim3(TRK_DEV_TMAX), BYTE_LDS_BYTES, s, a);
    KCHECK();
}

void launch_botsort_normalize(const float* in, float* out, int rows, int dim, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(botsort_normalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, out, rows, dim);
    KCHECK();
}

}  // namespace aic
