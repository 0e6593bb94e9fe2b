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
// bestshot_walk_kernel   one block of 512 threads per stream, the launch's ticks in order: the life cycle is slot_walk.hpp's, BestshotWalk
//                        states what is this stage's.  The slot table lives in LDS for the launch.
//                        A thread is slot t of the table AND row t of the frame.  Thumbnails move with 16-byte copies by the whole block:
//                        ENDED slots to the output list, winning candidates to their slots.
#include "bestshot.hpp"
#include "slot_walk.hpp"

namespace aic {

namespace {

constexpr int T = BS_TRACKS_MAX;

struct Rect { int x0, y0, x1, y1; };

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
    if (!row_valid(x1, y1, x2, y2, BS_COORD_MAX)) {
        if (tid == 0) out[0] = make_int4(0, 0, 0, 0), out[1] = make_int4(0, 0, 0, 0);
        return;
    }
    // ---- the first valid row of its id?
    if (tid == 0) s_flag = 0;
    __syncthreads();
    bool dup = false;
    for (int j = tid; j < r; j += 256) {
        const int* q = rows6 + (size_t)(off + j) * 6;
        dup = dup || (q[4] == rid && row_valid(q[0], q[1], q[2], q[3], BS_COORD_MAX));
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
        if (q[4] == rid || !row_valid(qx1, qy1, qx2, qy2, BS_COORD_MAX)) continue;
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

// what the best-shot stage states of the slot walk (slot_walk.hpp): a shot's seven ints a slot, the resident thumbnails, their copies
struct BestshotWalk {
    static constexpr int ARRAYS = BS_ARRAYS, ST_INTS = BS_ST_INTS, EVENT_INTS = BS_EVENT_INTS;
    struct Row {
        int flags, score, c0, c1, c2, c3;
        bool win;
    };
    const int4* info;
    const uint4* cand16;
    int cand_base, tq;                                                       // tq: 16-byte words of a thumbnail
    uint4 *slots16, *outs16;                                                 // the stream's resident thumbnails and its output list
    int* s_list2;

    __device__ __forceinline__ Row load_row(int r, bool in) const {
        Row x{0, 0, 0, 0, 0, 0, false};
        if (in) {
            const int4 a = info[(size_t)r * 2], b = info[(size_t)r * 2 + 1];
            x.flags = a.x, x.score = a.y, x.c0 = a.z, x.c1 = a.w, x.c2 = b.x, x.c3 = b.y;
        }
        return x;
    }
    __device__ __forceinline__ void fresh(const SlotLds& L, int slot) const {
        L.tab[BS_A_HAS][slot] = 0, L.tab[BS_A_BFRAME][slot] = 0, L.tab[BS_A_SCORE][slot] = 0;
        L.tab[BS_A_C0][slot] = 0, L.tab[BS_A_C1][slot] = 0, L.tab[BS_A_C2][slot] = 0, L.tab[BS_A_C3][slot] = 0;
    }
    __device__ __forceinline__ void commit(const SlotLds& L, Row& row, int slot, bool fresh_slot, int frame) const {
        row.win = (row.flags & BS_F_CAND) && (!L.tab[BS_A_HAS][slot] || row.score > L.tab[BS_A_SCORE][slot]);
        if (row.win) {
            L.tab[BS_A_HAS][slot] = 1, L.tab[BS_A_SCORE][slot] = row.score, L.tab[BS_A_BFRAME][slot] = frame;
            L.tab[BS_A_C0][slot] = row.c0, L.tab[BS_A_C1][slot] = row.c1, L.tab[BS_A_C2][slot] = row.c2, L.tab[BS_A_C3][slot] = row.c3;
        }
    }
    __device__ __forceinline__ void event(const SlotLds& L, int4* ev, int s, int e_rank) const {
        const int tid = threadIdx.x;
        L.list[e_rank] = tid;
        const int has = L.tab[BS_A_HAS][tid];
        slot_event_head(L, ev, s, has);
        ev[2] = make_int4(has ? L.tab[BS_A_BFRAME][tid] : 0, has ? L.tab[BS_A_SCORE][tid] : 0, has ? L.tab[BS_A_C0][tid] : 0, has ? L.tab[BS_A_C1][tid] : 0);
        ev[3] = make_int4(has ? L.tab[BS_A_C2][tid] : 0, has ? L.tab[BS_A_C3][tid] : 0, tid, 0);
    }
    __device__ __forceinline__ void post_emit(const SlotLds& L, bool em, int n_emit, int n_out) const {
        __syncthreads();
        for (int i = 0; i < n_emit; ++i) {
            const int slot = L.list[i];
            const bool has = L.tab[BS_A_HAS][slot] != 0;
            const uint4* src = slots16 + (size_t)slot * tq;
            uint4* dst = outs16 + (size_t)(n_out + i) * tq;
            for (int q = threadIdx.x; q < tq; q += T) dst[q] = has ? src[q] : make_uint4(0, 0, 0, 0);
        }
        __syncthreads();                                                     // the copies are done before a row may take the slot
        if (em) L.tab[BS_A_STATE][threadIdx.x] = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void post_tick(const SlotLds& L, const Row& row, int slot, int off, int n, int& stopped) const {
        int n_win, n_lost;
        const int win_rank = block_scan(row.win, L.w, n_win);
        block_scan(row.win && !(row.flags & BS_F_STORED), L.w, n_lost);
        if (row.win) L.live[win_rank] = off + threadIdx.x - cand_base, s_list2[win_rank] = slot;
        __syncthreads();
        for (int i = 0; i < n_win; ++i) {
            const uint4* src = cand16 + (size_t)L.live[i] * tq;
            uint4* dst = slots16 + (size_t)s_list2[i] * tq;
            for (int q = threadIdx.x; q < tq; q += T) dst[q] = src[q];
        }
        if (n_lost) stopped = AIC_ERR_RUNTIME;                               // a winner whose thumbnail the score kernel withheld: never
    }
    __device__ __forceinline__ void tail(const SlotCall& c, int kk) const {}
};

__global__ __launch_bounds__(512) void bestshot_walk_kernel(const int* __restrict__ frame_off, int n_ticks, const int* __restrict__ rows6,
                                                            const int4* __restrict__ info, const uint8_t* __restrict__ cand, int cand_base,
                                                            const int* __restrict__ reset, const int* __restrict__ mode, int first, BsGeom g,
                                                            int* __restrict__ state_all, uint8_t* __restrict__ slot_thumbs, int cap,
                                                            int* __restrict__ n_final, int* __restrict__ pending, int* __restrict__ status,
                                                            int* __restrict__ events, uint8_t* __restrict__ out_thumbs) {
    __shared__ int s_list2[T];
    const SlotCall c{frame_off, n_ticks, rows6, reset, mode, first, g.streams, g.max_tracks, g.forget_after, state_all, cap, n_final, pending, status,
                     events};
    const int s = blockIdx.x, tq = g.tw * g.th * 3 / 16;
    BestshotWalk v{info, reinterpret_cast<const uint4*>(cand), cand_base, tq, reinterpret_cast<uint4*>(slot_thumbs) + (size_t)s * g.max_tracks * tq,
                   reinterpret_cast<uint4*>(out_thumbs) + (size_t)s * cap * tq, s_list2};
    slot_walk(c, v);
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
