// kernels_archive.hip -- the identity archive's device side (archive.hpp, C ABI aic_archive_*).
//
//   archive_put_kernel      one wave per fp32 row: max |v| by shuffles, one correctly rounded division, int8 codes (round half to even),
//                           the row's scale and metadata into the slot the uploaded slot list names.  Also the queries' prologue
//                           (no slot list: row i -> row i) and, with mode 0, the check that runs before anything is stored.
//   archive_search_kernel   int8 MFMA (v_mfma_i32_16x16x64_i8) over the slots below the high-water mark; per-wave top-k lists in LDS
//   archive_merge_kernel    one block per query: the partial lists -> [Q, k] slots, distances and keys
//
// Arithmetic (tests/archive_oracle.py restates it; the int32 dot product is exact whatever order the hardware sums in):
//   inv = 127 / m, q_i = rint(v_i * inv), scale = m / 127; sim = (float(dot) * scale_row) * scale_query; dist = max(+0, 1 - sim);
//   rank by (dist bits << 32 | slot).  -ffp-contract=off keeps the two products and the subtraction apart.
//
// Operands of the MFMA: lane l carries 16 consecutive bytes of row (l & 15) at byte 64 ks + 16 (l >> 4) of K-step ks -- for the archive
// rows (A) and the query rows (B) alike, so whatever order the hardware gives the 64 k of a step, both sides share it and the dot
// product is that of the rows.  C/D: col = lane & 15 (query), row = (lane >> 4) * 4 + reg (slot within the group of 16).
#include "kernels.hpp"

#include <cfloat>

namespace aic {

namespace {

constexpr float kInfty = 1e5f;                               // linear_assignment.py:9
constexpr unsigned long long kNoKey = ~0ull;
constexpr int ARCHIVE_THR_COPIES = 32;                       // copies of the search's shared k-th keys (a block polls copy blockIdx.x % 32)

typedef int v4i __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned long long shfl64(unsigned long long v, int src) {
    const unsigned lo = __shfl((unsigned)v, src), hi = __shfl((unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long shfl64_up1(unsigned long long v) {
    const unsigned lo = __shfl_up((unsigned)v, 1), hi = __shfl_up((unsigned)(v >> 32), 1);
    return ((unsigned long long)hi << 32) | lo;
}

// the split of a sweep of nq <= 64 queries over the block's 4 waves: nt column tiles of 16 queries, sp waves per tile (each takes
// every sp-th group of 16 slots).  Shared by the search kernel, the merge kernel and the host's buffer size.
__host__ __device__ __forceinline__ int sweep_split(int nq) {
    const int nt = (nq + 15) >> 4;
    return nt == 1 ? 4 : nt == 2 ? 2 : 1;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ put / query prologue
// Wave i = row src_index[i] (NULL: i) of src (fp32, row_stride floats apart, the payload `offset` floats into the row).  Skipped: keys[i] < 0 or slots[i] < 0
// (either list may be NULL; no slot list = row i goes to row i).  A row with m == 0, a non-finite element or no finite 127 / m sets
// *flag and stores nothing.  mode 0 checks only.  Bytes [dim, pitch) of the stored row are zero.
__global__ __launch_bounds__(256) void archive_put_kernel(const float* __restrict__ src, const int* __restrict__ src_index, long row_stride, int offset,
                                                          int dim, int pitch, int n, const int* __restrict__ slots, const long long* __restrict__ keys,
                                                          const int* __restrict__ cams, long long tick, int mode, signed char* __restrict__ rows,
                                                          float* __restrict__ scale, int* __restrict__ camera, long long* __restrict__ t_last,
                                                          long long* __restrict__ key, int* __restrict__ flag) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;                                      // wave-uniform
    if (keys && keys[i] < 0) return;
    const int slot = slots ? slots[i] : i;
    if (slot < 0) return;
    const float* v = src + (size_t)(src_index ? src_index[i] : i) * row_stride + offset;
    float m = 0.f;
    bool bad = false;
    for (int c = lane; c < dim; c += 64) {
        const float a = fabsf(v[c]);
        bad |= !(a <= FLT_MAX);
        m = fmaxf(m, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float inv = __fdiv_rn(127.0f, m);
    bad |= !(m > 0.f) || !(inv <= FLT_MAX);
    if (__ballot(bad)) {
        if (lane == 0) atomicOr(flag, 1);
        return;
    }
    if (!mode) return;
    unsigned* o = reinterpret_cast<unsigned*>(rows + (size_t)slot * pitch);
    for (int c = 4 * lane; c < pitch; c += 256) {
        unsigned w = 0;
        if (c < dim) {                                       // dim % 4 == 0: a word is inside or outside as a whole
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= ((unsigned)(int)rintf(v[c + e] * inv) & 0xffu) << (8 * e);
        }
        o[c >> 2] = w;
    }
    if (lane == 0) {
        scale[slot] = __fdiv_rn(m, 127.0f);
        if (key) { camera[slot] = cams[i]; t_last[slot] = tick; key[slot] = keys[i]; }
    }
}

// ------------------------------------------------------------------------------------------------ search
// Block (bx, sweep): slots [bx R, min(hw, bx R + R)) against queries [64 sweep, 64 sweep + nq).  Wave w holds column tile ct = w % (4 / sp)
// of 16 queries as the B operand in registers (NKS K-steps of 64 bytes: zero beyond the pitch and beyond Q) and streams the groups of
// 16 slots sub, sub + sp, ... of the range as the A operand, 16 bytes per lane straight from global memory, the loads of 4 or 8
// K-steps (neighbouring steps share a 128-byte line) issued before their MFMAs.  After the K loop a lane has 4 (slot, query) cells: it
// forms the distances, drops what cannot enter its query's list (the k-th key so far, kept in a register) or lies beyond max_distance,
// and only for the rest reads the slot's metadata and applies the filters.  Survivors go into the wave's own sorted list of the query
// in LDS, the (at most one) candidate of each of the 16 queries in a lane group at once: the four lanes of a column each shift a
// quarter of its list.  No barrier, the waves never meet -- but a wave publishes a full list's k-th key (gthr, atomic min) and reads
// the others' every fourth group: a key above any wave's k-th key is not among the k smallest, so the lists stop growing early.
// part: per sweep [gridDim.x * sp][nq][k] keys ascending, ~0 in the empty places; sweep s starts at s * gridDim.x * 64 * k.
template <int NKS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void archive_search_kernel(
    const signed char* __restrict__ rows, const float* __restrict__ scale, const int* __restrict__ camera, const long long* __restrict__ t_last,
    const long long* __restrict__ key, int hw, int pitch, int R, const signed char* __restrict__ qrows, const float* __restrict__ qscale,
    const aic_archive_filter* __restrict__ flt, int Q, int k, unsigned long long* __restrict__ part, unsigned long long* gthr) {
    constexpr int CH = NKS == 8 ? 8 : NKS == 16 ? 2 : 4;                    // K-steps whose loads are in flight together (16 steps of B leave room for 4)
    __shared__ unsigned long long s_list[4][16][32];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, grp = lane >> 4;
    const int sweep = blockIdx.y, q0 = sweep * 64, nq = min(64, Q - q0);
    const int nt = (nq + 15) >> 4, sp = sweep_split(nq), ntw = 4 / sp;
    const int ct = w % ntw, sub = w / ntw;
    if (ct >= nt) return;                                    // 3 tiles: the fourth wave has none (no barrier follows)
    const int nks = pitch >> 6;
    const int q = q0 + ct * 16 + col;
    const bool qok = q < Q;

    v4i b[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        b[ks] = v4i{0, 0, 0, 0};
        if (qok && ks < nks) b[ks] = *reinterpret_cast<const v4i*>(qrows + (size_t)q * pitch + ks * 64 + grp * 16);
    }
    const float qs = qok ? qscale[q] : 0.f;
    const float maxd = qok ? flt[q].max_distance : 0.f;
    for (int i = lane; i < 16 * 32; i += 64) (&s_list[w][0][0])[i] = kNoKey;
    __builtin_amdgcn_wave_barrier();
    unsigned long long thr = kNoKey;                         // the k-th key of this lane's query so far, here or in any other wave
    const int seg = (k + 3) >> 2;                            // entries of a query's list per lane: lane (grp, col) holds [grp seg, grp seg + seg)

    // the shared keys: ARCHIVE_THR_COPIES copies of [max(Q, 16)] (a copy per 128-byte line at least), block bx uses copy bx % copies, so
    // that the blocks do not all poll one L2 channel
    unsigned long long* gq = gthr + (size_t)(blockIdx.x % ARCHIVE_THR_COPIES) * max(Q, 16) + (qok ? q : 0);
    unsigned long long seen = kNoKey;
    int gi = 0;
    const int r0 = blockIdx.x * R, r1 = min(hw, r0 + R);    // R % 64 == 0
    for (int g0 = r0 + 16 * sub; g0 < r1; g0 += 16 * sp) {
        const signed char* pa = rows + (size_t)(g0 + col) * pitch + grp * 16;
        // another wave's k-th key bounds this query's k-th key from above, and a stale one is only looser: read every fourth group
        if (qok && !(gi++ & 3)) seen = __hip_atomic_load(gq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        thr = seen < thr ? seen : thr;
        v4i acc = {0, 0, 0, 0};
#pragma unroll
        for (int c0 = 0; c0 < NKS; c0 += CH) {
            v4i a[CH];
#pragma unroll
            for (int p = 0; p < CH; p += 2)
                if (c0 + p < nks) {                          // an odd step count: the pair's second load reads into the next row (B is zero there)
                    a[p] = *reinterpret_cast<const v4i*>(pa + (c0 + p) * 64);
                    a[p + 1] = *reinterpret_cast<const v4i*>(pa + (c0 + p + 1) * 64);
                }
#pragma unroll
            for (int p = 0; p < CH; p += 2)
                if (c0 + p < nks) {
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p], b[c0 + p], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[p + 1], b[c0 + p + 1], acc, 0, 0, 0);
                }
        }
        const int s0 = g0 + grp * 4;
        const float4 sc = *reinterpret_cast<const float4*>(scale + s0);
        const float scr[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int slot = s0 + r;
            const float sim = ((float)acc[r] * scr[r]) * qs;
            const float d1 = 1.0f - sim;
            const float dist = d1 > 0.f ? d1 : 0.f;
            const unsigned long long ck = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned)slot;
            bool cand = qok && slot < r1 && dist <= maxd && ck < thr;
            if (cand) {                                      // rare once the lists are warm: only now the slot's metadata
                const aic_archive_filter f = flt[q];
                const long long kk = key[slot], tl = t_last[slot];
                cand = kk >= 0 && kk != f.exclude_key && tl >= f.t_lo && tl <= f.t_hi && (f.exclude_camera < 0 || camera[slot] != f.exclude_camera);
            }
            const unsigned long long any = __ballot(cand);
            if (!any) continue;                              // wave-uniform
#pragma unroll 1
            for (int g = 0; g < 4; ++g) {                    // the candidates of lane group g: at most one per query, all 16 queries at once
                if (!((any >> (16 * g)) & 0xffffull)) continue;
                const int srcl = 16 * g + col;
                const unsigned long long nk = shfl64(ck, srcl);
                const bool has = __shfl((int)cand, srcl) != 0 && nk < thr;   // thr may have tightened earlier in this round
                unsigned long long* list = &s_list[w][col][0];
                const int lo = grp * seg, hi = min(k, lo + seg);
                // the four lanes of a column shift their segments of its list; the entry below a segment is read before anyone writes
                const unsigned long long below = lo > 0 && lo < hi ? list[lo - 1] : 0;
                __builtin_amdgcn_wave_barrier();
                if (has && lo < hi) {
                    unsigned long long cur = list[hi - 1];
                    for (int idx = hi - 1; idx >= lo; --idx) {
                        const unsigned long long pred = idx > lo ? list[idx - 1] : below;
                        const unsigned long long neu = cur < nk ? cur : (idx == 0 || pred < nk) ? nk : pred;
                        list[idx] = neu;
                        cur = pred;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                const unsigned long long kth = list[k - 1];
                thr = kth < thr ? kth : thr;
            }
        }
        // published at most once a group, and only a key below what was last read or written
        if (qok && thr < seen) {
            if (grp == 0) atomicMin(gq, thr);
            seen = thr;
        }
    }
    unsigned long long* out = part + (size_t)sweep * gridDim.x * 64 * k + ((size_t)(blockIdx.x * sp + sub) * nq) * k;
    for (int i = lane; i < 16 * k; i += 64) {
        const int c = i / k, j = i - c * k, ql = ct * 16 + c;
        if (ql < nq) out[(size_t)ql * k + j] = s_list[w][c][j];
    }
}

// ------------------------------------------------------------------------------------------------ merge
// Block q: the blocks * sp sorted partial lists of query q -> its k smallest keys.  Keys are unique (the slot is part of the key), so round
// r takes the smallest key above round r - 1's; a list's candidate is among its first r + 1 entries.
__global__ __launch_bounds__(256) void archive_merge_kernel(const unsigned long long* __restrict__ part, int blocks, int Q, int k,
                                                            const long long* __restrict__ key, int* __restrict__ out_slot, float* __restrict__ out_dist,
                                                            long long* __restrict__ out_key) {
    __shared__ unsigned long long s_min[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int sweep = q >> 6, ql = q & 63, nq = min(64, Q - sweep * 64);
    const int P = blocks * sweep_split(nq);
    const unsigned long long* base = part + (size_t)sweep * blocks * 64 * k + (size_t)ql * k;
    unsigned long long prev = 0;
    bool done = false;
    for (int r = 0; r < k; ++r) {
        unsigned long long best = kNoKey;
        if (!done)
            for (int p = tid; p < P; p += 256) {
                const unsigned long long* l = base + (size_t)p * nq * k;
                for (int j = 0; j <= r; ++j) {
                    const unsigned long long v = l[j];
                    if (r == 0 || v > prev) { best = v < best ? v : best; break; }
                }
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = shfl64(best, (tid & 63) ^ o);
            best = other < best ? other : best;
        }
        __syncthreads();                                     // the previous round's readers of s_min are done
        if ((tid & 63) == 0) s_min[tid >> 6] = best;
        __syncthreads();
        best = s_min[0];
#pragma unroll
        for (int x = 1; x < 4; ++x) best = s_min[x] < best ? s_min[x] : best;
        if (best == kNoKey) done = true;                     // block-uniform: the rest of the places are empty
        prev = best;
        if (tid == 0) {
            const int slot = done ? -1 : (int)(unsigned)best;
            out_slot[(size_t)q * k + r] = slot;
            out_dist[(size_t)q * k + r] = done ? kInfty : __uint_as_float((unsigned)(best >> 32));
            out_key[(size_t)q * k + r] = done ? -1 : key[slot];
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_archive_put(const float* src, const int* src_index, long row_stride, int offset, int dim, int pitch, int n, const int* slots, const long long* keys,
                        const int* cams, long long tick, int mode, signed char* rows, float* scale, int* camera, long long* t_last, long long* key,
                        int* flag, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(archive_put_kernel, dim3((n + 3) / 4), dim3(256), 0, s, src, src_index, row_stride, offset, dim, pitch, n,
                       slots, keys, cams, tick, mode,
                       rows, scale, camera, t_last, key, flag);
    KCHECK();
}

int archive_block_rows(int hw, int n_queries) {
    const int sweeps = std::max(1, (n_queries + 63) / 64);
    const int max_blocks = std::max(64, std::min(1024, 4096 / sweeps));
    const int per = (std::max(hw, 1) + max_blocks - 1) / max_blocks;
    return std::max(ARCHIVE_MIN_BLOCK_ROWS, (per + 63) / 64 * 64);
}

size_t archive_partial_keys(int hw, int n_queries, int k) {   // the partial lists, then one shared k-th key a query
    const int R = archive_block_rows(hw, n_queries), blocks = std::max(1, (hw + R - 1) / R);
    return (size_t)((n_queries + 63) / 64) * blocks * 64 * k + (size_t)ARCHIVE_THR_COPIES * std::max(n_queries, 16);
}

void launch_archive_search(const signed char* rows, const float* scale, const int* camera, const long long* t_last, const long long* key, int hw,
                           int pitch, const signed char* qrows, const float* qscale, const aic_archive_filter* flt, int n_queries, int k,
                           unsigned long long* part, int* out_slot, float* out_dist, long long* out_key, hipStream_t s) {
    if (n_queries <= 0) return;
    const int R = archive_block_rows(hw, n_queries), blocks = std::max(1, (hw + R - 1) / R);
    const dim3 grid(blocks, (n_queries + 63) / 64);
    const size_t n_thr = (size_t)ARCHIVE_THR_COPIES * std::max(n_queries, 16);
    unsigned long long* gthr = part + archive_partial_keys(hw, n_queries, k) - n_thr;
    HIP_CHECK(hipMemsetAsync(gthr, 0xff, n_thr * 8, s));
#define AIC_ARCHIVE_SEARCH(NKS)                                                                                                              \
    hipLaunchKernelGGL(archive_search_kernel<NKS>, grid, dim3(256), 0, s, rows, scale, camera, t_last, key, hw, pitch, R, qrows, qscale, flt, \
                       n_queries, k, part, gthr)
    if (pitch <= 256) AIC_ARCHIVE_SEARCH(4);
    else if (pitch <= 512) AIC_ARCHIVE_SEARCH(8);
    else AIC_ARCHIVE_SEARCH(16);
#undef AIC_ARCHIVE_SEARCH
    KCHECK();
    hipLaunchKernelGGL(archive_merge_kernel, dim3(n_queries), dim3(256), 0, s, part, blocks, n_queries, k, key, out_slot, out_dist, out_key);
    KCHECK();
}

}  // namespace aic
