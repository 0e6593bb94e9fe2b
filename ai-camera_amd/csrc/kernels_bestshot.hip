// kernels_bestshot.hip -- the two kernels of the best-shot stage (bestshot.hpp).  Integer arithmetic only;
// tests/bestshot_oracle.py is the specification.  No global atomics, no scratch.
//
// bestshot_score_kernel  stateless, one block of 256 threads per row of the launch.  Rows that are not candidates leave after their
//                        flags.  The block builds the TH x TW x 3 thumbnail in dynamic LDS (24 KiB at 64 x 128: five blocks per CU
//                        beside each other; 96 KiB at 128 x 256: one block per CU): thread = thumbnail pixel, so with TW = 64 a wave
//                        is one thumbnail row, a lane one column, and the lanes of a wave read neighbouring windows of the same
//                        source rows -- every cache line fetched is used whole.  Sharpness is a 5-point Laplacian on the gray level
//                        recomputed from LDS, reduced per wave then over the four waves; the occluder loop strides the frame's rows.
//                        The thumbnail goes to the per-row candidate buffer only when the row could still win: its id is not in a live
//                        slot that is certain to survive up to this tick, or that slot has no shot, or the score beats the slot's best
//                        as it stood when the launch began (a best score only rises while a slot lives).
// bestshot_walk_kernel   one block of 512 threads per stream, the launch's ticks in order.  The slot table lives in LDS for the launch.
//                        A thread is slot t of the table AND row t of the frame.  Thumbnails move with 16-byte copies by the whole block:
//                        ENDED slots to the output list, winning candidates to their slots.
#include "bestshot.hpp"

namespace aic {

namespace {

constexpr int T = BS_TRACKS_MAX;

struct Rect { int x0, y0, x1, y1; };

__device__ __forceinline__ bool coord_ok(int v) { return v >= -BS_COORD_MAX && v <= BS_COORD_MAX; }
__device__ __forceinline__ bool row_valid(int x1, int y1, int x2, int y2) {
    return coord_ok(x1) && coord_ok(y1) && coord_ok(x2) && coord_ok(y2) && x2 >= x1 && y2 >= y1;
}
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = imax(v, __shfl_xor(v, d));
    return v;
}

__device__ __forceinline__ int gray_at(const uint8_t* th, int idx) {
    return (29 * th[3 * idx] + 150 * th[3 * idx + 1] + 77 * th[3 * idx + 2] + 128) >> 8;
}

__global__ __launch_bounds__(256) void bestshot_score_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ frame_off,
                                                             const int* __restrict__ rows6, const int* __restrict__ state_all,
                                                             const int* __restrict__ reset, int first, BsGeom g, int cand_base,
                                                             int4* __restrict__ info, uint8_t* __restrict__ cand) {
    extern __shared__ __align__(16) uint8_t s_thumb[];                       // [TH][TW][3]
    __shared__ int s_red[4];
    __shared__ int s_flag;
    const int x = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int off = frame_off[x], n = frame_off[x + 1] - off;
    if (r >= n) return;
    const int s = x % g.streams, kk = x / g.streams;
    const int* st = state_all + (size_t)s * BS_ST_INTS;
    const bool fresh = first && reset[s];
    int4* out = info + (size_t)(off + r) * 2;
    if (!fresh && st[1] != 0) {                                              // a stopped stream commits nothing
        if (tid == 0) out[0] = make_int4(0, 0, 0, 0), out[1] = make_int4(0, 0, 0, 0);
        return;
    }
    const int* row = rows6 + (size_t)(off + r) * 6;
    const int x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3], rid = row[4];
    if (!row_valid(x1, y1, x2, y2)) {
        if (tid == 0) out[0] = make_int4(0, 0, 0, 0), out[1] = make_int4(0, 0, 0, 0);
        return;
    }
    // ---- the first valid row of its id?
    if (tid == 0) s_flag = 0;
    __syncthreads();
    bool dup = false;
    for (int j = tid; j < r; j += 256) {
        const int* q = rows6 + (size_t)(off + j) * 6;
        dup = dup || (q[4] == rid && row_valid(q[0], q[1], q[2], q[3]));
    }
    if (dup) s_flag = 1;
    __syncthreads();
    int flags = BS_F_VALID | (s_flag ? 0 : BS_F_FIRST);
    // ---- region, clipped
    Rect reg;
    reg.x0 = x1 - g.pad, reg.y0 = y1 - g.pad, reg.x1 = x2 + g.pad;
    reg.y1 = g.region == BS_REGION_BOX ? y2 + g.pad : y1 + (int)(((long long)(y2 - y1) * g.head_q8) >> 8);
    Rect c;
    c.x0 = imax(reg.x0, 0), c.y0 = imax(reg.y0, 0), c.x1 = imin(reg.x1, g.w - 1), c.y1 = imin(reg.y1, g.h - 1);
    const bool nonempty = c.x1 >= c.x0 && c.y1 >= c.y0;
    const int cw = c.x1 - c.x0 + 1, ch = c.y1 - c.y0 + 1;
    const bool is_cand = (flags & BS_F_FIRST) && nonempty && cw >= g.min_w && ch >= g.min_h;
    if (nonempty) flags |= BS_F_NONEMPTY;
    const int trunc = nonempty && (c.x0 != reg.x0 || c.y0 != reg.y0 || c.x1 != reg.x1 || c.y1 != reg.y1);
    if (trunc) flags |= BS_F_TRUNC;
    if (!is_cand) {
        if (tid == 0) {
            out[0] = make_int4(flags, 0, nonempty ? c.x0 : 0, nonempty ? c.y0 : 0);
            out[1] = make_int4(nonempty ? c.x1 : 0, nonempty ? c.y1 : 0, 0, 0);
        }
        return;
    }
    flags |= BS_F_CAND;
    // ---- the thumbnail: thread = thumbnail pixel, its window summed along the source rows
    const int TW = g.tw, TH = g.th, npix = TW * TH;
    const uint8_t* frame = frames + (size_t)x * g.h * g.w * 3;
    for (int idx = tid; idx < npix; idx += 256) {
        const int u = idx % TW, v = idx / TW;
        const int xa = c.x0 + (int)(((long long)u * cw) / TW);
        int xb = c.x0 + (int)(((long long)(u + 1) * cw) / TW);
        const int ya = c.y0 + (int)(((long long)v * ch) / TH);
        int yb = c.y0 + (int)(((long long)(v + 1) * ch) / TH);
        if (xb == xa) xb = xa + 1;
        if (yb == ya) yb = ya + 1;
        unsigned sb = 0, sg = 0, sr = 0;
        for (int y = ya; y < yb; ++y) {
            const uint8_t* p = frame + ((size_t)y * g.w + xa) * 3;
            for (int xx = xa; xx < xb; ++xx, p += 3) sb += p[0], sg += p[1], sr += p[2];
        }
        const unsigned cnt = (unsigned)(xb - xa) * (unsigned)(yb - ya);      // <= 2^20, the sums <= 255 * 2^20
        s_thumb[3 * idx] = (uint8_t)((sb + cnt / 2) / cnt);
        s_thumb[3 * idx + 1] = (uint8_t)((sg + cnt / 2) / cnt);
        s_thumb[3 * idx + 2] = (uint8_t)((sr + cnt / 2) / cnt);
    }
    __syncthreads();
    // ---- sharpness over the interior
    int part = 0;
    for (int idx = tid; idx < npix; idx += 256) {
        const int u = idx % TW, v = idx / TW;
        if (u >= 1 && u <= TW - 2 && v >= 1 && v <= TH - 2) {
            const int d = 4 * gray_at(s_thumb, idx) - gray_at(s_thumb, idx - 1) - gray_at(s_thumb, idx + 1) - gray_at(s_thumb, idx - TW) -
                          gray_at(s_thumb, idx + TW);
            part += d < 0 ? -d : d;
        }
    }
    part = wave_sum(part);
    if (lane == 0) s_red[wv] = part;
    __syncthreads();
    const int sharp = s_red[0] + s_red[1] + s_red[2] + s_red[3];             // <= 126 * 254 * 1020 < 2^25
    __syncthreads();
    // ---- the largest share of C one occluder covers
    const long long area = (long long)cw * ch;
    int cover = 0;
    for (int j = tid; j < n; j += 256) {
        const int* q = rows6 + (size_t)(off + j) * 6;
        const int qx1 = q[0], qy1 = q[1], qx2 = q[2], qy2 = q[3];
        if (q[4] == rid || !row_valid(qx1, qy1, qx2, qy2)) continue;
        if (!(qy2 > y2 || (qy2 == y2 && j < r))) continue;
        const int bx0 = imax(qx1, 0), by0 = imax(qy1, 0), bx1 = imin(qx2, g.w - 1), by1 = imin(qy2, g.h - 1);
        const int iw = imin(c.x1, bx1) - imax(c.x0, bx0) + 1, ih = imin(c.y1, by1) - imax(c.y0, by0) + 1;
        if (iw > 0 && ih > 0) cover = imax(cover, (int)(((long long)iw * ih * 256) / area));
    }
    cover = wave_max(cover);
    if (lane == 0) s_red[wv] = cover;
    __syncthreads();
    cover = imax(imax(s_red[0], s_red[1]), imax(s_red[2], s_red[3]));
    const long long fill_ll = (area * 256) / ((long long)TW * TH);
    const int fill = fill_ll > 256 ? 256 : (int)fill_ll;
    const int score = (int)(((long long)sharp * fill * (256 - cover)) >> (16 + trunc));
    // ---- could the row still win?  The table as the launch found it
    if (tid == 0) s_flag = 0;
    __syncthreads();
    if (!fresh) {
        const int f = st[0] + kk;                                            // the tick's frame number unless the stream stops before it
        for (int t = tid; t < g.max_tracks; t += 256) {
            const int* a = st + BS_ST_SLOTS + t;
            if (a[BS_A_STATE * T] == 1 && a[BS_A_ID * T] == rid && a[BS_A_HAS * T] && score <= a[BS_A_SCORE * T] &&
                f - a[BS_A_LAST * T] <= g.forget_after)
                s_flag = 1;                                                  // live up to this tick whatever happens, and no worse
        }
    }
    __syncthreads();
    const bool store = !s_flag;
    if (store) {
        uint4* dst = reinterpret_cast<uint4*>(cand + (size_t)(off + r - cand_base) * npix * 3);
        const uint4* src = reinterpret_cast<const uint4*>(s_thumb);
        for (int q = tid; q < npix * 3 / 16; q += 256) dst[q] = src[q];
        flags |= BS_F_STORED;
    }
    if (tid == 0) out[0] = make_int4(flags, score, c.x0, c.y0), out[1] = make_int4(c.x1, c.y1, 0, 0);
}

// exclusive prefix sum over the 512 threads of the block; total = the block's sum.  s_w: 8 ints of LDS, free again on return
__device__ __forceinline__ int block_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int t = s_w[i];
        base += i < w ? t : 0;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(512) void bestshot_walk_kernel(const int* __restrict__ frame_off, int n_ticks, const int* __restrict__ rows6,
                                                            const int4* __restrict__ info, const uint8_t* __restrict__ cand, int cand_base,
                                                            const int* __restrict__ reset, const int* __restrict__ mode, int first, BsGeom g,
                                                            int* __restrict__ state_all, uint8_t* __restrict__ slot_thumbs, int cap,
                                                            int* __restrict__ n_final, int* __restrict__ pending, int* __restrict__ status,
                                                            int* __restrict__ events, uint8_t* __restrict__ out_thumbs) {
    __shared__ int s_tab[BS_ARRAYS][T];
    __shared__ int s_live[T], s_list[T], s_list2[T];
    __shared__ int s_w[8];
    int* s_id = s_tab[BS_A_ID];
    int* s_state = s_tab[BS_A_STATE];
    int* s_last = s_tab[BS_A_LAST];
    int* s_has = s_tab[BS_A_HAS];
    int* s_score = s_tab[BS_A_SCORE];
    const int s = blockIdx.x, tid = threadIdx.x, S = g.streams;
    int* st = state_all + (size_t)s * BS_ST_INTS;
    const bool fresh = first && reset[s];
    int frame = fresh ? 0 : st[0];
    int stopped = fresh ? 0 : st[1];
#pragma unroll
    for (int a = 0; a < BS_ARRAYS; ++a) s_tab[a][tid] = fresh ? 0 : st[BS_ST_SLOTS + a * T + tid];
    int n_out = first ? 0 : n_final[s];
    const int tq = g.tw * g.th * 3 / 16;                                     // 16-byte words of a thumbnail
    uint4* slots16 = reinterpret_cast<uint4*>(slot_thumbs) + (size_t)s * g.max_tracks * tq;
    uint4* outs16 = reinterpret_cast<uint4*>(out_thumbs) + (size_t)s * cap * tq;
    const uint4* cand16 = reinterpret_cast<const uint4*>(cand);
    __syncthreads();

    // ENDED slots (E, ranked e_rank in slot order) leave for the output list while it has room; they become free
    auto emit = [&](bool E, int e_rank, int n_E) {
        const int room = cap - n_out;
        const bool em = E && e_rank < room;
        if (em) {
            s_list[e_rank] = tid;
            int4* ev = reinterpret_cast<int4*>(events + ((size_t)s * cap + n_out + e_rank) * BS_EVENT_INTS);
            const int has = s_tab[BS_A_HAS][tid];
            ev[0] = make_int4(s_state[tid] == 3 ? BS_FLUSHED : BS_EXPIRED, s, s_id[tid], s_tab[BS_A_CLS][tid]);
            ev[1] = make_int4(s_tab[BS_A_FIRST][tid], s_last[tid], s_tab[BS_A_SIGHT][tid], has);
            ev[2] = make_int4(has ? s_tab[BS_A_BFRAME][tid] : 0, has ? s_score[tid] : 0, has ? s_tab[BS_A_C0][tid] : 0, has ? s_tab[BS_A_C1][tid] : 0);
            ev[3] = make_int4(has ? s_tab[BS_A_C2][tid] : 0, has ? s_tab[BS_A_C3][tid] : 0, tid, 0);
        }
        __syncthreads();
        const int n_emit = n_E < room ? n_E : (room > 0 ? room : 0);
        for (int i = 0; i < n_emit; ++i) {
            const int slot = s_list[i];
            const bool has = s_has[slot] != 0;
            const uint4* src = slots16 + (size_t)slot * tq;
            uint4* dst = outs16 + (size_t)(n_out + i) * tq;
            for (int q = tid; q < tq; q += T) dst[q] = has ? src[q] : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();                                                     // the copies are done before a row may take the slot
        if (em) s_state[tid] = 0;
        n_out += n_emit;
        __syncthreads();
    };

    if (n_ticks == 0) {
        const int m = mode[s];
        if (m == BS_MODE_FLUSH && s_state[tid] == 1) s_state[tid] = 3;
        if (m != BS_MODE_NONE) {
            const bool E = tid < g.max_tracks && s_state[tid] >= 2;
            int n_E;
            const int e_rank = block_scan(E, s_w, n_E);
            emit(E, e_rank, n_E);
        }
    }
    for (int kk = 0; kk < n_ticks && !stopped; ++kk) {
        const int x = kk * S + s;
        const int off = frame_off[x], n = frame_off[x + 1] - off;            // 0..512, checked by the host
        // ---- this thread as row tid
        int flags = 0, score = 0, c0 = 0, c1 = 0, c2 = 0, c3 = 0, rid = 0, rcls = 0;
        if (tid < n) {
            const int4 a = info[(size_t)(off + tid) * 2], b = info[(size_t)(off + tid) * 2 + 1];
            flags = a.x, score = a.y, c0 = a.z, c1 = a.w, c2 = b.x, c3 = b.y;
            rid = rows6[(size_t)(off + tid) * 6 + 4], rcls = rows6[(size_t)(off + tid) * 6 + 5];
        }
        const int need = BS_F_VALID | BS_F_FIRST | BS_F_NONEMPTY;
        const bool counted = (flags & need) == need;
        // ---- this thread as slot tid
        const int state = tid < g.max_tracks ? s_state[tid] : 0;
        const bool expiring = state == 1 && frame - s_last[tid] > g.forget_after;
        const bool E = state >= 2 || expiring;
        s_live[tid] = state == 1 && !expiring;
        __syncthreads();
        int slot = -1;
        if (counted)
            for (int t = 0; t < g.max_tracks; ++t)
                if (s_live[t] && s_id[t] == rid) slot = t;
        const bool is_new = counted && slot < 0;
        int n_new, n_E, n_live, n_old, n_unfit;
        const int new_rank = block_scan(is_new, s_w, n_new);
        const int e_rank = block_scan(E, s_w, n_E);
        block_scan(s_live[tid], s_w, n_live);
        block_scan(state >= 2, s_w, n_old);
        block_scan(expiring && e_rank >= cap - n_out, s_w, n_unfit);         // ENDED now, no room in the list: the slot stays taken
        if (n_live + n_old + n_unfit + n_new > g.max_tracks) {               // nothing of this tick is committed
            stopped = AIC_ERR_CAPACITY;
            break;
        }
        if (expiring) s_state[tid] = 2;
        emit(E, e_rank, n_E);
        const bool is_free = tid < g.max_tracks && s_state[tid] == 0;
        int n_free;
        const int free_rank = block_scan(is_free, s_w, n_free);
        if (is_free) s_list[free_rank] = tid;
        __syncthreads();
        bool win = false;
        if (counted) {
            if (slot < 0) {                                                  // the k-th new row takes the k-th lowest free slot
                slot = s_list[new_rank];
                s_id[slot] = rid, s_state[slot] = 1, s_tab[BS_A_FIRST][slot] = frame, s_tab[BS_A_SIGHT][slot] = 0, s_has[slot] = 0;
                s_tab[BS_A_BFRAME][slot] = 0, s_score[slot] = 0;
                s_tab[BS_A_C0][slot] = 0, s_tab[BS_A_C1][slot] = 0, s_tab[BS_A_C2][slot] = 0, s_tab[BS_A_C3][slot] = 0;
            }
            s_last[slot] = frame, s_tab[BS_A_CLS][slot] = rcls, s_tab[BS_A_SIGHT][slot] += 1;
            win = (flags & BS_F_CAND) && (!s_has[slot] || score > s_score[slot]);
            if (win) {
                s_has[slot] = 1, s_score[slot] = score, s_tab[BS_A_BFRAME][slot] = frame;
                s_tab[BS_A_C0][slot] = c0, s_tab[BS_A_C1][slot] = c1, s_tab[BS_A_C2][slot] = c2, s_tab[BS_A_C3][slot] = c3;
            }
        }
        int n_win, n_lost;
        const int win_rank = block_scan(win, s_w, n_win);
        block_scan(win && !(flags & BS_F_STORED), s_w, n_lost);
        if (win) s_live[win_rank] = off + tid - cand_base, s_list2[win_rank] = slot;
        __syncthreads();
        for (int i = 0; i < n_win; ++i) {
            const uint4* src = cand16 + (size_t)s_live[i] * tq;
            uint4* dst = slots16 + (size_t)s_list2[i] * tq;
            for (int q = tid; q < tq; q += T) dst[q] = src[q];
        }
        ++frame;
        if (n_lost) stopped = AIC_ERR_RUNTIME;                               // a winner whose thumbnail the score kernel withheld: never
        __syncthreads();
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < BS_ARRAYS; ++a) st[BS_ST_SLOTS + a * T + tid] = s_tab[a][tid];
    int n_pend;
    block_scan(tid < g.max_tracks && s_state[tid] >= 2, s_w, n_pend);
    if (tid == 0) st[0] = frame, st[1] = stopped, n_final[s] = n_out, pending[s] = n_pend, status[s] = stopped;
}

}  // namespace

void launch_bestshot_score(const uint8_t* frames, const int* frame_off, int n_frames, int max_rows, const int* rows6, const int* state, const int* reset,
                           int first, const BsGeom& g, int cand_base, int* info, uint8_t* cand, hipStream_t s) {
    if (n_frames <= 0 || max_rows <= 0) return;
    const size_t lds = (size_t)g.tw * g.th * 3;
    set_lds_limit(bestshot_score_kernel, 128 * 256 * 3);
    hipLaunchKernelGGL(bestshot_score_kernel, dim3(n_frames, max_rows), dim3(256), lds, s, frames, frame_off, rows6, state, reset, first, g, cand_base,
                       reinterpret_cast<int4*>(info), cand);
    KCHECK();
}

void launch_bestshot_walk(const int* frame_off, int n_ticks, const int* rows6, const int* info, const uint8_t* cand, int cand_base, const int* reset,
                          const int* mode, int first, const BsGeom& g, int* state, uint8_t* slot_thumbs, int cap, int* n_final, int* pending,
                          int* status, int* events, uint8_t* out_thumbs, hipStream_t s) {
    hipLaunchKernelGGL(bestshot_walk_kernel, dim3(g.streams), dim3(T), 0, s, frame_off, n_ticks, rows6, reinterpret_cast<const int4*>(info), cand,
                       cand_base, reset, mode, first, g, state, slot_thumbs, cap, n_final, pending, status, events, out_thumbs);
    KCHECK();
}

}  // namespace aic
