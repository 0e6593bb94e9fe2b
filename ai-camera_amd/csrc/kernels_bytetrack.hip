// kernels_bytetrack.hip -- ByteTrack on the device, k frames per launch (structures: bytetrack.hpp).
//
// Specification: BYTETracker.update() of the ByteTrack authors (yolox/tracker/byte_tracker.py, matching.py) as restated in
// tests/bytetrack_oracle.py, with its four deliberate changes (this project's IoU, the reference DeepSORT fp32 Kalman filter,
// per-tracker ids, SciPy's tie rules on lap's extended matrix).  The life cycle and the assignment are byte_epoch.hpp's (shared with
// BoT-SORT); this file is the ByteTrack variant of it: the xyah measurement, mean_to_tlwh, the DeepSORT filter of trk_math.hpp run in
// place (covariance in HBM, mean in LDS), the fused IoU cost alone, and the activated tracks as output.
#include "kernels.hpp"
#include "trk_dev.hpp"
#include "trk_math.hpp"
#include "trk_wave.hpp"
#include "bytetrack.hpp"
#include "byte_epoch.hpp"

namespace aic {

struct BtArgs {
    EpochCall c;                    // stream s: bt_table(c.bank + s * c.table_stride, cap); c.ext: extended matrices beyond the LDS arena
    BtParams prm;
    int lds_bytes;
};

namespace {

struct BtVariant {
    using Args = BtArgs;
    using Lds = ByteLds;
    using Table = BtTable;
    struct Ctx {};
    static constexpr size_t EXTRA_LDS_BYTES = 0;
    static __device__ __forceinline__ void carve_extra(Lds&, LdsTake&) {}
    static __device__ __forceinline__ Table table(const Args& a, int sid) { return bt_table(a.c.bank + (size_t)sid * a.c.table_stride, a.prm.cap); }
    static __device__ __forceinline__ float high(const BtParams& P) { return P.track_thresh; }
    static __device__ __forceinline__ float low(const BtParams& P) { return P.low_thresh; }
    // tlwh_to_xyah (detection.py:36-47)
    static __device__ __forceinline__ void detection(const Lds& L, const Args&, Ctx&, int i, int, float x, float y, float w, float h) {
        L.meas[i * 4 + 0] = x + w / 2.0f, L.meas[i * 4 + 1] = y + h / 2.0f, L.meas[i * 4 + 2] = h > 0.f ? w / h : 0.f, L.meas[i * 4 + 3] = h;
    }
    // track box (mean_to_tlwh of deepsort_oracle.py / track.py:133-151)
    static __device__ __forceinline__ void mean_box(const float* m, float b[4]) { aic::mean_box(m, b); }
    static __device__ __forceinline__ void zero_velocity(float* m) { m[7] = 0.f; }
    static __device__ __forceinline__ void predict(const Lds& L, const Args&, const Table& tbl, int, int np, int) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int r = wv; r < np; r += NW) {
            const int sl = L.pool[r];
            kf_predict_wave(tbl.cov + (size_t)sl * 64, L.mean + sl * 8, lane);
        }
    }
    static __device__ __forceinline__ void cost_pass(const Lds&, const Args&, const Table&, Ctx&, float*, int, const int*, int, const int*, int, int, bool) {}
    static __device__ __forceinline__ void post_solve(const Lds&, Ctx&, const float*, int, const int*, int, const int*, bool, bool) {}
    static __device__ __forceinline__ void commit(const Lds& L, const Args&, const Table& tbl, Ctx&, const int* rows, int nr, const int* cols, int, bool) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int r = wv; r < nr; r += NW) {
            const int c = L.mrow[r];
            if (c >= 0) kf_update_wave(tbl.cov + (size_t)rows[r] * 64, L.mean + rows[r] * 8, L.meas + cols[c] * 4, lane);
        }
        __threadfence_block();
        __syncthreads();
    }
    static __device__ __forceinline__ void activate(const Lds&, int, int) {}
    static __device__ __forceinline__ void initiate(const Lds& L, const Args&, const Table& tbl, int nnew, int) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        for (int r = wv; r < nnew; r += NW) kf_initiate_wave(tbl.cov + (size_t)L.fre[r] * 64, L.mean + L.fre[r] * 8, L.meas + L.newd[r] * 4, lane);
    }
    // the activated tracks of the tracked list, compacted into L.rows
    static __device__ __forceinline__ int outputs(const Lds& L, int ntl, const int*& list) {
        const int tid = threadIdx.x, osl = tid < ntl ? L.tl[tid] : 0;
        list = L.rows;
        return block_compact(tid < ntl && L.act[osl], osl, L.rows, L.wcnt);
    }
    static __device__ __forceinline__ void load_slot(const Lds&, const Table&, int) {}
    static __device__ __forceinline__ void store_slot(const Lds&, const Table&, int) {}
    static __device__ __forceinline__ void begin(const Lds&, Ctx&) {}
    static __device__ __forceinline__ void finish(BtHdr*, const Lds&, Ctx&) {}
};
static_assert(byte_arena_floats<BtVariant>() == 12528, "the LDS arena of the ByteTrack kernel: extended sides up to 111");

}  // namespace

__global__ __launch_bounds__(TRK_DEV_TMAX) void bytetrack_epoch_kernel(BtArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ ByteLds s_lds;
    BtVariant::Ctx x;
    byte_epoch<BtVariant>(a, smem, s_lds, x);
}

void launch_bytetrack_epoch(const BtParams& prm, const EpochCall& c, hipStream_t s) {
    set_lds_limit(bytetrack_epoch_kernel, BYTE_LDS_BYTES);
    BtArgs a{c, prm, BYTE_LDS_BYTES};
    hipLaunchKernelGGL(bytetrack_epoch_kernel, dim3(c.streams), dim3(TRK_DEV_TMAX), BYTE_LDS_BYTES, s, a);
    KCHECK();
}

}  // namespace aic
