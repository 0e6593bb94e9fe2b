// kernels_xcam.hip -- cross-camera identities inside a tracker bank (xcam.hpp, C ABI aic_xcam_*).
//
// What configs[4] does between ranks (kernels_trk_dev.hip: gallery_shard_kernel, gallery_nearest_kernel; global_id.cpp), for the S
// cameras of one bank in one device pass:
//   xcam_pack_deepsort_kernel / xcam_pack_botsort_kernel   block s packs stream s's shard, fp32 [t_max, 2 + dim] = (valid, track id,
//                                                          unit embedding); valid rows are a prefix, their number goes to n_valid[s]
//   xcam_count_kernel                                       the same n_valid for shards the caller made (aic_xcam_link_shards)
//   xcam_nearest_kernel                                     the table of gallery_nearest_kernel as a tiled all-pairs pass over the LIVE rows
//   xcam_finalize_kernel                                    keys -> near_row / near_dist, ids, the -1 rows of the invalid tails
//
// Arithmetic of a distance: max(0, 1 - <e_i, e_j>) (matching.py:136-141), the products summed k ascending in fp32 with separate
// multiply and add (-ffp-contract=off; no MFMA: its internal accumulation is not that arithmetic), which is bit for bit what
// gallery_nearest_kernel and oracle/xcam_oracle.py compute; d(i, j) == d(j, i) because a * b == b * a.
#include "kernels.hpp"
#include "botsort.hpp"
#include "trk_dev.hpp"
#include "trk_wave.hpp"

namespace aic {

namespace {

constexpr float kInfty = 1e5f;                               // linear_assignment.py:9
constexpr unsigned long long kNoKey = ~0ull;

__device__ __forceinline__ float cos_dist(float dot) {       // matching.py:136-141
    const float x = 1.0f - dot;
    return x > 0.f ? x : 0.f;
}

// rows [0, t_max) of one stream's shard from the selected tracks: wave w copies rows w, w + NW, ... 8 bytes per lane (a shard row is
// 8-byte aligned: 2 + dim floats with dim % 4 == 0, payload at + 2 floats; the source rows are 16-byte aligned)
template <class Src>
__device__ __forceinline__ void pack_rows(float* __restrict__ out, int t_max, int dim, int cnt, Src src) {
    const int tid = threadIdx.x, w = 2 + dim;
    for (int r = tid >> 6; r < t_max; r += NW) {
        float* o = out + (size_t)r * w;
        if (r < cnt) {
            int id;
            const float* g = src(r, &id);
            for (int c = 2 * (tid & 63); c < dim; c += 128) *reinterpret_cast<float2*>(o + 2 + c) = *reinterpret_cast<const float2*>(g + c);
            if ((tid & 63) == 0) { o[0] = 1.0f; o[1] = (float)id; }
        } else if ((tid & 63) == 0) {
            o[0] = 0.0f; o[1] = 0.0f;
        }
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ pack: DeepSORT bank
// Block s = stream s of a DeepSortBank (table DevTrkHdr | DevTrack[cap] | ..., tbl_stride bytes apart; unit galleries gal_stride floats
// apart): gallery_shard_kernel's rows -- the first t_max tracks in list order with state == 2 && glen > 0, the newest gallery entry.
// A stream whose header carries err packs nothing.  flags[s]: bit 1 = a packed track id does not fit fp32 (>= 2^24).
__global__ __launch_bounds__(TRK_DEV_TMAX) void xcam_pack_deepsort_kernel(const char* __restrict__ tbl, size_t tbl_stride, const float* __restrict__ gal_n,
                                                                         size_t gal_stride, int gmax, int dim, float* __restrict__ out, int t_max,
                                                                         int* __restrict__ n_valid, int* __restrict__ flags) {
    __shared__ int wcnt[NW + 8];
    __shared__ int sel[TRK_DEV_TMAX];
    __shared__ int s_big;
    const int s = blockIdx.x, tid = threadIdx.x;
    const DevTrkHdr* hdr = reinterpret_cast<const DevTrkHdr*>(tbl + (size_t)s * tbl_stride);
    const DevTrack* trk = reinterpret_cast<const DevTrack*>(hdr + 1);
    const float* gal = gal_n + (size_t)s * gal_stride;
    if (tid == 0) s_big = 0;
    const int T = hdr->err ? 0 : min(hdr->n_tracks, TRK_DEV_TMAX);
    const bool ok = tid < T && trk[tid].state == 2 && trk[tid].glen > 0;
    const int cnt = min(block_compact(ok, tid, sel, wcnt), t_max);
    if (tid < cnt && trk[sel[tid]].id >= (1 << 24)) s_big = 1;
    pack_rows(out + (size_t)s * t_max * (2 + dim), t_max, dim, cnt, [&](int r, int* id) {
        const DevTrack t = trk[sel[r]];
        int pos = t.ghead + t.glen - 1;
        if (pos >= gmax) pos -= gmax;
        *id = t.id;
        return gal + ((size_t)t.slot * gmax + pos) * dim;
    });
    __syncthreads();
    if (tid == 0) { n_valid[s] = cnt; flags[s] = s_big ? 2 : 0; }
}

// ------------------------------------------------------------------------------------------------ pack: BoT-SORT bank
// Block s = stream s of a BoT-SORT bank (botsort.hpp: table_stride bytes / smooth_stride floats apart): the first t_max tracks of the
// tracked list, in its order, that are activated and have a feature; the row is the slot's smoothed unit feature.
__global__ __launch_bounds__(TRK_DEV_TMAX) void xcam_pack_botsort_kernel(char* __restrict__ bank, size_t table_stride, float* __restrict__ smooth,
                                                                        size_t smooth_stride, int cap, int dim, float* __restrict__ out, int t_max,
                                                                        int* __restrict__ n_valid, int* __restrict__ flags) {
    __shared__ int wcnt[NW + 8];
    __shared__ int sel[TRK_DEV_TMAX];
    __shared__ int s_big;
    const int s = blockIdx.x, tid = threadIdx.x;
    const BsTable t = bs_table(bank + (size_t)s * table_stride, cap, smooth + (size_t)s * smooth_stride);
    if (tid == 0) s_big = 0;
    const int T = t.hdr->err ? 0 : min(t.hdr->n_tracked, cap);
    const int sl = tid < T ? t.tl[tid] : 0;
    const bool ok = tid < T && t.trk[sl].act != 0 && t.hasf[sl] != 0;
    const int cnt = min(block_compact(ok, sl, sel, wcnt), t_max);
    if (tid < cnt && t.trk[sel[tid]].id >= (1 << 24)) s_big = 1;
    pack_rows(out + (size_t)s * t_max * (2 + dim), t_max, dim, cnt, [&](int r, int* id) {
        *id = t.trk[sel[r]].id;
        return t.feat + (size_t)sel[r] * dim;
    });
    __syncthreads();
    if (tid == 0) { n_valid[s] = cnt; flags[s] = s_big ? 2 : 0; }
}

// ------------------------------------------------------------------------------------------------ count: caller-made shards
// n_valid[s] = valid rows of stream s; flags[s] bit 0 = they are not a prefix of the stream's slice.
__global__ __launch_bounds__(TRK_DEV_TMAX) void xcam_count_kernel(const float* __restrict__ g, int t_max, int dim, int* __restrict__ n_valid,
                                                                 int* __restrict__ flags) {
    __shared__ int s_cnt, s_last;
    const int s = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) s_cnt = 0, s_last = -1;
    __syncthreads();
    const bool v = tid < t_max && g[((size_t)s * t_max + tid) * (2 + dim)] > 0.5f;
    const unsigned long long bal = __ballot(v);
    if ((tid & 63) == 0 && bal) {
        atomicAdd(&s_cnt, __popcll(bal));
        atomicMax(&s_last, (tid & ~63) + 63 - __clzll(bal));
    }
    __syncthreads();
    if (tid == 0) { n_valid[s] = s_cnt; flags[s] = s_last + 1 != s_cnt ? 1 : 0; }
}

// ------------------------------------------------------------------------------------------------ nearest: tiled all pairs
// The LIVE rows -- the n_valid[s] first rows of every stream, stream-major: L of them -- are the index space.  Block (bi, by) owns the
// T = 16 R live rows [bi T, bi T + T) and walks the column tiles jt = by, by + gridDim.y, ... of T live rows each.  Per tile pair the K
// range goes through LDS in chunks of XCAM_KC, both operands transposed ([k][row]: a row of the image is what one k contributes, so a
// lane reads its R rows and its R columns with one wide read each, conflict-free); thread (ty, tx) keeps the R x R dot products of rows
// R ty.. and columns R tx.. in registers and adds one product per k to each, k ascending.  The next chunk's global loads are issued
// before the current chunk's arithmetic.  A pair of tiles that lies inside one stream is skipped.
// Result: best[raw row i] = min over the valid rows j of other streams of (distance bits << 32 | raw row j), merged across the column
// splits with a 64-bit atomic min (distances are >= +0: the bit pattern orders like the value; ties go to the lowest row).
// Blocks beyond the live rows return at once: the cost follows L, not S * t_max.
template <int R>
__global__ __launch_bounds__(256) void xcam_nearest_kernel(const float* __restrict__ g, const int* __restrict__ n_valid, int S, int t_max, int dim,
                                                          unsigned long long* __restrict__ best) {
    constexpr int T = 16 * R, KC = XCAM_KC, NQ = 256 / T, NLD = KC / 2 / NQ;
    typedef float vecr __attribute__((ext_vector_type(R)));
    __shared__ __attribute__((aligned(16))) float sA[KC][T];
    __shared__ __attribute__((aligned(16))) float sB[KC][T];
    __shared__ int s_pre[BANK_STREAMS_MAX_XCAM + 1];      // exclusive prefix of the clamped n_valid
    __shared__ int s_irow[T], s_istr[T], s_jrow[T], s_jstr[T];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int w = 2 + dim;

    // ---- prefix of n_valid over the streams (S <= 256 = the block)
    s_pre[tid + 1] = tid < S ? min(max(n_valid[tid], 0), t_max) : 0;
    if (tid == 0) s_pre[0] = 0;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = tid + 1 > o ? s_pre[tid + 1 - o] : 0;
        __syncthreads();
        s_pre[tid + 1] += v;
        __syncthreads();
    }
    const int L = s_pre[S];
    const int i0 = blockIdx.x * T;
    if (i0 >= L) return;                                   // block-uniform

    auto locate = [&](int c, int* row, int* str) {        // live index -> raw row, stream (-1 beyond the live rows)
        if (c >= L) { *row = -1; *str = -1; return; }
        int lo = 0, hi = S - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_pre[mid + 1] > c) hi = mid; else lo = mid + 1;
        }
        *row = lo * t_max + (c - s_pre[lo]);
        *str = lo;
    };
    if (tid < T) locate(i0 + tid, &s_irow[tid], &s_istr[tid]);
    __syncthreads();
    const int ni = min(T, L - i0);
    const int i_first = s_istr[0], i_last = s_istr[ni - 1];

    // the loader's row of both tiles: thread -> (row lr, k pairs kq + NQ u)
    const int lr = tid % T, kq = tid / T;
    const float* pa = s_irow[lr] >= 0 ? g + (size_t)s_irow[lr] * w + 2 : nullptr;
    int irow[R], istr[R];
#pragma unroll
    for (int x = 0; x < R; ++x) irow[x] = s_irow[R * ty + x], istr[x] = s_istr[R * ty + x];
    unsigned long long bst[R];
#pragma unroll
    for (int x = 0; x < R; ++x) bst[x] = kNoKey;

    const int n_jt = (L + T - 1) / T;
    for (int jt = blockIdx.y; jt < n_jt; jt += gridDim.y) {
        const int j0 = jt * T;
        __syncthreads();                                   // the previous tile's readers of s_jrow / s_jstr are done
        if (tid < T) locate(j0 + tid, &s_jrow[tid], &s_jstr[tid]);
        __syncthreads();
        const int nj = min(T, L - j0);
        if (i_first == i_last && s_jstr[0] == i_first && s_jstr[nj - 1] == i_first) continue;   // block-uniform: one stream on both sides
        const float* pb = s_jrow[lr] >= 0 ? g + (size_t)s_jrow[lr] * w + 2 : nullptr;

        float acc[R][R];
#pragma unroll
        for (int x = 0; x < R; ++x)
#pragma unroll
            for (int y = 0; y < R; ++y) acc[x][y] = 0.f;

        float2 ra[NLD], rb[NLD];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int k = k0 + 2 * (kq + NQ * u);
                const bool in = k < dim;                  // dim is even: a pair is inside or outside as a whole
                ra[u] = pa && in ? *reinterpret_cast<const float2*>(pa + k) : float2{0.f, 0.f};
                rb[u] = pb && in ? *reinterpret_cast<const float2*>(pb + k) : float2{0.f, 0.f};
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < dim; k0 += KC) {
#pragma unroll
            for (int u = 0; u < NLD; ++u) {
                const int k = 2 * (kq + NQ * u);
                sA[k][lr] = ra[u].x, sA[k + 1][lr] = ra[u].y;
                sB[k][lr] = rb[u].x, sB[k + 1][lr] = rb[u].y;
            }
            __syncthreads();
            if (k0 + KC < dim) fetch(k0 + KC);
            const int kc = min(KC, dim - k0);              // a multiple of 4
            for (int kk = 0; kk < kc; kk += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const vecr a = *reinterpret_cast<const vecr*>(&sA[kk + q][R * ty]);
                    const vecr b = *reinterpret_cast<const vecr*>(&sB[kk + q][R * tx]);
#pragma unroll
                    for (int x = 0; x < R; ++x)
#pragma unroll
                        for (int y = 0; y < R; ++y) acc[x][y] = acc[x][y] + a[x] * b[y];
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int y = 0; y < R; ++y) {
            const int jr = s_jrow[R * tx + y], js = s_jstr[R * tx + y];
#pragma unroll
            for (int x = 0; x < R; ++x) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(cos_dist(acc[x][y])) << 32) | (unsigned)jr;
                if (jr >= 0 && irow[x] >= 0 && js != istr[x] && key < bst[x]) bst[x] = key;
            }
        }
    }
#pragma unroll
    for (int x = 0; x < R; ++x) {
        unsigned long long b = bst[x];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) {                  // the 16 lanes of one ty are consecutive
            const unsigned long long other = __shfl_xor(b, o);
            b = other < b ? other : b;
        }
        if (tx == 0 && irow[x] >= 0 && b != kNoKey) atomicMin(&best[irow[x]], b);
    }
}

// ------------------------------------------------------------------------------------------------ finalize
// Every raw row: its track id (or -1), its nearest row and distance (or -1 / kInfty: an invalid row, or no valid row of another stream).
__global__ __launch_bounds__(256) void xcam_finalize_kernel(const float* __restrict__ g, const int* __restrict__ n_valid, int n, int t_max, int dim,
                                                           const unsigned long long* __restrict__ best, int* __restrict__ ids,
                                                           int* __restrict__ near_row, float* __restrict__ near_dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int s = i / t_max, r = i - s * t_max;
    const bool valid = r < min(max(n_valid[s], 0), t_max);
    const unsigned long long b = valid ? best[i] : kNoKey;
    ids[i] = valid ? (int)g[(size_t)i * (2 + dim) + 1] : -1;
    near_row[i] = b == kNoKey ? -1 : (int)(unsigned)b;
    near_dist[i] = b == kNoKey ? kInfty : __uint_as_float((unsigned)(b >> 32));
}

// ------------------------------------------------------------------------------------------------ launchers
void launch_xcam_pack_deepsort(const char* tbl, size_t tbl_stride, const float* gal_n, size_t gal_stride, int gmax, int dim, int streams, int t_max,
                               float* shards, int* n_valid, int* flags, hipStream_t s) {
    hipLaunchKernelGGL(xcam_pack_deepsort_kernel, dim3(streams), dim3(TRK_DEV_TMAX), 0, s, tbl, tbl_stride, gal_n, gal_stride, gmax, dim, shards, t_max,
                       n_valid, flags);
    KCHECK();
}

void launch_xcam_pack_botsort(char* bank, size_t table_stride, float* smooth, size_t smooth_stride, int cap, int dim, int streams, int t_max,
                              float* shards, int* n_valid, int* flags, hipStream_t s) {
    hipLaunchKernelGGL(xcam_pack_botsort_kernel, dim3(streams), dim3(TRK_DEV_TMAX), 0, s, bank, table_stride, smooth, smooth_stride, cap, dim, shards,
                       t_max, n_valid, flags);
    KCHECK();
}

void launch_xcam_count(const float* shards, int streams, int t_max, int dim, int* n_valid, int* flags, hipStream_t s) {
    hipLaunchKernelGGL(xcam_count_kernel, dim3(streams), dim3(TRK_DEV_TMAX), 0, s, shards, t_max, dim, n_valid, flags);
    KCHECK();
}

int xcam_tile_rows(int streams, int t_max, int tile) {
    if (tile == 32 || tile == 64) return tile;
    return (long)streams * t_max < XCAM_SMALL_ROWS ? 32 : 64;
}

void launch_xcam_nearest(const float* shards, const int* n_valid, int streams, int t_max, int dim, int tile, unsigned long long* best, int* ids,
                         int* near_row, float* near_dist, hipStream_t s) {
    const int n = streams * t_max;
    if (n <= 0) return;
    const int T = xcam_tile_rows(streams, t_max, tile), nt = (n + T - 1) / T;
    // column splits: enough blocks to fill the chip when few row tiles are live (the grid is sized for n, the live rows may be far fewer)
    const int splits = std::max(1, std::min(nt, (4096 + nt - 1) / nt));
    HIP_CHECK(hipMemsetAsync(best, 0xff, (size_t)n * 8, s));
    if (T == 32) hipLaunchKernelGGL(xcam_nearest_kernel<2>, dim3(nt, splits), dim3(256), 0, s, shards, n_valid, streams, t_max, dim, best);
    else hipLaunchKernelGGL(xcam_nearest_kernel<4>, dim3(nt, splits), dim3(256), 0, s, shards, n_valid, streams, t_max, dim, best);
    KCHECK();
    hipLaunchKernelGGL(xcam_finalize_kernel, dim3((n + 255) / 256), dim3(256), 0, s, shards, n_valid, n, t_max, dim, best, ids, near_row, near_dist);
    KCHECK();
}

}  // namespace aic
