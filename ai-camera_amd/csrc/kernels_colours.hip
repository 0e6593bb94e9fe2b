// kernels_colours.hip -- the two kernels of the clothing-colour stage (colours.hpp).  Integer arithmetic only;
// tests/colours_oracle.py is the specification.  No global atomics, no scratch.
//
// colours_sample_kernel  stateless, one block of 256 threads per row of the launch.  Rows that are invalid, not the first of their id or
//                        empty leave after their flags.  Per part (torso, legs): the occluder loop strides the frame's rows and is
//                        reduced per wave, then over the four waves.  A lane then takes 4 pixels = 12 bytes of one pixel row of the
//                        part at a time: the three or four ALIGNED dwords that hold them and an alignbyte per dword, so a part may
//                        start at any byte (3 x0, a pitch 3 W that is no multiple of 4, a frame pointer of any alignment) and there is
//                        one path only; every aligned dword read holds at least one byte of the part, so no read leaves the frame's
//                        pages.  Neighbouring lanes read neighbouring 12 bytes.  Classification is per lane (cl_classify, the two
//                        divisions by a reciprocal from a 256-entry table the block computes into LDS).  The 12 counts are gathered
//                        WITHOUT atomics and without LDS histograms: a ballot per bin and a popcount -- the counts are wave-uniform
//                        scalars, 36 scalar instructions per 64 pixels beside some 60 vector instructions per pixel of classification,
//                        where an LDS histogram would serialise on the few colours clothing really has (one bin takes most pixels).
// colours_walk_kernel    one block of 512 threads per stream, the launch's ticks in order: the life cycle is slot_walk.hpp's, ColoursWalk
//                        states what is this stage's.  A thread is slot t of the table AND row t of the frame.  The eight small
//                        arrays of the table live in LDS for the launch (16 KiB); the accumulators (24 ints a slot, 48 KiB a stream) stay in HBM: a tick touches only the slots of its counted rows, some 30 of
//                        512, so loading and storing all of them per launch would move more bytes than it saves, and 64 KiB of LDS
//                        would leave one block per CU.  A slot's accumulators are written by the thread of its row and read by the
//                        thread of its slot only across a block barrier.
#include "colours.hpp"
#include "slot_walk.hpp"

namespace aic {

namespace {

constexpr int T = CL_TRACKS_MAX;

__global__ __launch_bounds__(256) void colours_sample_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ frame_off,
                                                             const int* __restrict__ rows6, const int* __restrict__ state_all,
                                                             const int* __restrict__ reset, int first, ColGeom g, int info_base,
                                                             int4* __restrict__ info) {
    __shared__ unsigned s_recip[256];
    __shared__ int s_red[4];
    __shared__ int s_cnt[4][CL_BINS];
    __shared__ int s_flag;
    const int x = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int off = frame_off[x], n = frame_off[x + 1] - off;
    if (r >= n) return;
    const int s = x % g.streams;
    const int* st = state_all + (size_t)s * CL_ST_INTS;
    const bool fresh = first && reset[s];
    int4* out = info + (size_t)(off + r - info_base) * (CL_INFO_INTS / 4);
    const int* row = rows6 + (size_t)(off + r) * 6;
    const int x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3], rid = row[4];
    int flags = 0;
    bool go = (fresh || st[1] == 0) && row_valid(x1, y1, x2, y2, CL_COORD_MAX);            // a stopped stream commits nothing
    if (go) {
        // ---- the first valid row of its id?
        if (tid == 0) s_flag = 0;
        __syncthreads();
        bool dup = false;
        for (int j = tid; j < r; j += 256) {
            const int* q = rows6 + (size_t)(off + j) * 6;
            dup = dup || (q[4] == rid && row_valid(q[0], q[1], q[2], q[3], CL_COORD_MAX));
        }
        if (dup) s_flag = 1;
        __syncthreads();
        const bool nonempty = imin(x2, g.w - 1) >= imax(x1, 0) && imin(y2, g.h - 1) >= imax(y1, 0);
        flags = CL_F_VALID | (s_flag ? 0 : CL_F_FIRST) | (nonempty ? CL_F_NONEMPTY : 0);
        go = !s_flag && nonempty;
    }
    if (!go) {
        if (tid < CL_INFO_INTS / 4) out[tid] = make_int4(tid == 0 ? flags : 0, 0, 0, 0);
        return;
    }
    s_recip[tid] = cl_recip((unsigned)tid);
    const uint8_t* frame = frames + (size_t)x * g.h * g.w * 3;
    const int bw = x2 - x1, bh = y2 - y1, inset = (bw * g.inset_q8) >> 8;
    int n_part[2] = {0, 0};
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        const int fa = part ? g.l0 : g.t0, fb = part ? g.l1 : g.t1;
        const int px0 = imax(x1 + inset, 0), px1 = imin(x2 - inset, g.w - 1);
        const int py0 = imax(y1 + ((bh * fa) >> 8), 0), py1 = imin(y1 + ((bh * fb) >> 8), g.h - 1);
        const int pw = px1 - px0 + 1, ph = py1 - py0 + 1;
        __syncthreads();                                                     // s_red, s_cnt and the table are free / filled
        if (pw < g.min_w || ph < g.min_h || pw <= 0 || ph <= 0) {            // (uniform over the block)
            if (tid < 3) out[1 + 3 * part + tid] = make_int4(0, 0, 0, 0);
            continue;
        }
        // ---- the largest share of P one occluder covers
        const long long area = (long long)pw * ph;
        int cover = 0;
        for (int j = tid; j < n; j += 256) {
            const int* q = rows6 + (size_t)(off + j) * 6;
            const int qx1 = q[0], qy1 = q[1], qx2 = q[2], qy2 = q[3];
            if (q[4] == rid || !row_valid(qx1, qy1, qx2, qy2, CL_COORD_MAX)) continue;
            if (!(qy2 > y2 || (qy2 == y2 && j < r))) continue;
            const int bx0 = imax(qx1, 0), by0 = imax(qy1, 0), bx1 = imin(qx2, g.w - 1), by1 = imin(qy2, g.h - 1);
            const int iw = imin(px1, bx1) - imax(px0, bx0) + 1, ih = imin(py1, by1) - imax(py0, by0) + 1;
            if (iw > 0 && ih > 0) cover = imax(cover, (int)(((long long)iw * ih * 256) / area));
        }
        cover = wave_max(cover);
        if (lane == 0) s_red[wv] = cover;
        __syncthreads();
        cover = imax(imax(s_red[0], s_red[1]), imax(s_red[2], s_red[3]));
        if (cover > g.max_cover_q8) {
            if (tid < 3) out[1 + 3 * part + tid] = make_int4(0, 0, 0, 0);
            continue;
        }
        // ---- the pixels: an item is 4 pixels of one pixel row
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0, c8 = 0, c9 = 0, c10 = 0, c11 = 0;      // wave-uniform
        const int qpr = (pw + 3) >> 2;                                       // items per pixel row
        const int items = qpr * ph;                                          // <= 4096 * 16384 = 2^26
        const size_t pitch = (size_t)g.w * 3;
        for (int base = 0; base < items; base += 256) {                      // (whole waves stay in step: the ballots below need them)
            const int i = base + tid;
            int m = 0;                                                       // pixels of this lane's item
            unsigned d0 = 0, d1 = 0, d2 = 0;
            if (i < items) {
                const int yy = i / qpr, qq = i - yy * qpr;
                m = imin(4, pw - 4 * qq);
                const uintptr_t a = reinterpret_cast<uintptr_t>(frame + (size_t)(py0 + yy) * pitch + (size_t)(px0 + 4 * qq) * 3);
                const unsigned sh = (unsigned)(a & 3);
                const unsigned* q = reinterpret_cast<const unsigned*>(a - sh);
                const int last = (int)(sh + 3 * m - 1) >> 2;                 // the last aligned dword that holds a byte of the item
                const unsigned w0 = q[0], w1 = last >= 1 ? q[1] : 0u, w2 = last >= 2 ? q[2] : 0u, w3 = last >= 3 ? q[3] : 0u;
                d0 = __builtin_amdgcn_alignbyte(w1, w0, sh);
                d1 = __builtin_amdgcn_alignbyte(w2, w1, sh);
                d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int b, gg, rr;
                if (p == 0) b = d0 & 255, gg = (d0 >> 8) & 255, rr = (d0 >> 16) & 255;
                else if (p == 1) b = d0 >> 24, gg = d1 & 255, rr = (d1 >> 8) & 255;
                else if (p == 2) b = (d1 >> 16) & 255, gg = d1 >> 24, rr = d2 & 255;
                else b = (d2 >> 8) & 255, gg = (d2 >> 16) & 255, rr = d2 >> 24;
                const int bin = p < m ? cl_classify(b, gg, rr, s_recip) : -1;
                c0 += __popcll(__ballot(bin == 0)), c1 += __popcll(__ballot(bin == 1)), c2 += __popcll(__ballot(bin == 2));
                c3 += __popcll(__ballot(bin == 3)), c4 += __popcll(__ballot(bin == 4)), c5 += __popcll(__ballot(bin == 5));
                c6 += __popcll(__ballot(bin == 6)), c7 += __popcll(__ballot(bin == 7)), c8 += __popcll(__ballot(bin == 8));
                c9 += __popcll(__ballot(bin == 9)), c10 += __popcll(__ballot(bin == 10)), c11 += __popcll(__ballot(bin == 11));
            }
        }
        if (lane == 0) {
            int* c = s_cnt[wv];
            c[0] = c0, c[1] = c1, c[2] = c2, c[3] = c3, c[4] = c4, c[5] = c5, c[6] = c6, c[7] = c7, c[8] = c8, c[9] = c9, c[10] = c10, c[11] = c11;
        }
        __syncthreads();
        if (tid < CL_BINS) {                                                 // s[k] = c[k] * 256 // n, n <= 2^28
            const long long c = (long long)s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
            reinterpret_cast<int*>(out)[4 + part * CL_BINS + tid] = (int)((c * 256) / area);
        }
        flags |= part ? CL_F_LOWER : CL_F_UPPER;
        n_part[part] = (int)area;
    }
    if (tid == 0) out[0] = make_int4(flags, n_part[0], n_part[1], 0), out[7] = make_int4(0, 0, 0, 0);
}

// the bin of the largest of 12 accumulators in memory, lowest index on ties
__device__ __forceinline__ int top_of(const int* acc) {
    int t = 0, best = acc[0];
#pragma unroll
    for (int k = 1; k < CL_BINS; ++k) {
        const int v = acc[k];
        if (v > best) best = v, t = k;
    }
    return t;
}

// what the colour stage states of the slot walk (slot_walk.hpp): two sample counts a slot, the accumulators in HBM, the row tags
struct ColoursWalk {
    static constexpr int ARRAYS = CL_ARRAYS, ST_INTS = CL_ST_INTS, EVENT_INTS = CL_EVENT_INTS;
    struct Row {
        int flags;
        const int4* inf;
        int4 tag;
    };
    const int4* info;
    int info_base;
    int* acc_all;                                                            // [slot][part][bin] of the stream
    int4* row_tags;

    __device__ __forceinline__ Row load_row(int r, bool in) const {
        Row x;
        x.inf = info + (size_t)(r - info_base) * (CL_INFO_INTS / 4);
        x.flags = in ? x.inf[0].x : 0;
        x.tag = make_int4(-1, -1, -1, -1);
        return x;
    }
    __device__ __forceinline__ void fresh(const SlotLds& L, int slot) const { L.tab[CL_A_NU][slot] = 0, L.tab[CL_A_NL][slot] = 0; }
    __device__ __forceinline__ void commit(const SlotLds& L, Row& row, int slot, bool fresh_slot, int frame) const {
        int4* acc4 = reinterpret_cast<int4*>(acc_all + slot * 2 * CL_BINS);
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            int& ns = L.tab[part ? CL_A_NL : CL_A_NU][slot];
            const bool add = (row.flags & (part ? CL_F_LOWER : CL_F_UPPER)) && ns < CL_SAMPLES_MAX;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                int4 a = fresh_slot ? make_int4(0, 0, 0, 0) : acc4[part * 3 + q];
                if (add) {
                    const int4 v = row.inf[1 + part * 3 + q];
                    a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
                }
                if (add || fresh_slot) acc4[part * 3 + q] = a;
            }
            if (add) ns += 1;
        }
        const int* acc = acc_all + slot * 2 * CL_BINS;
        const int nu = L.tab[CL_A_NU][slot], nl = L.tab[CL_A_NL][slot];
        int4& tag = row.tag;
        if (nu > 0) tag.x = top_of(acc), tag.z = acc[tag.x] / nu;
        else tag.z = 0;
        if (nl > 0) tag.y = top_of(acc + CL_BINS), tag.w = acc[CL_BINS + tag.y] / nl;
        else tag.w = 0;
    }
    __device__ __forceinline__ void event(const SlotLds& L, int4* ev, int s, int e_rank) const {
        const int tid = threadIdx.x;
        const int* acc = acc_all + tid * 2 * CL_BINS;
        const int nu = L.tab[CL_A_NU][tid], nl = L.tab[CL_A_NL][tid];
        int tu, su, tl, sl;
        cl_describe(acc, nu, &tu, &su, reinterpret_cast<int*>(ev + 4));
        cl_describe(acc + CL_BINS, nl, &tl, &sl, reinterpret_cast<int*>(ev + 7));
        slot_event_head(L, ev, s, nu);
        ev[2] = make_int4(nl, tu, su, tl);
        ev[3] = make_int4(sl, tid, 0, 0);
        ev[10] = make_int4(0, 0, 0, 0), ev[11] = make_int4(0, 0, 0, 0);
    }
    __device__ __forceinline__ void post_emit(const SlotLds& L, bool em, int n_emit, int n_out) const {
        if (em) L.tab[CL_A_STATE][threadIdx.x] = 0;
        __syncthreads();                                                     // the accumulators are read before a row may take the slot
    }
    __device__ __forceinline__ void post_tick(const SlotLds& L, const Row& row, int slot, int off, int n, int& stopped) const {
        if (row_tags && (int)threadIdx.x < n) row_tags[off + threadIdx.x] = row.tag;
    }
    __device__ __forceinline__ void tail(const SlotCall& c, int kk) const {
        if (row_tags)                                                        // a stopped stream's rows: the tick it stopped at and all after
            for (; kk < c.n_ticks; ++kk) {
                const int x = kk * c.streams + blockIdx.x;
                const int off = c.frame_off[x], n = c.frame_off[x + 1] - off;
                if ((int)threadIdx.x < n) row_tags[off + threadIdx.x] = make_int4(-1, -1, -1, -1);
            }
    }
};

__global__ __launch_bounds__(512) void colours_walk_kernel(const int* __restrict__ frame_off, int n_ticks, const int* __restrict__ rows6,
                                                           const int4* __restrict__ info, int info_base, const int* __restrict__ reset,
                                                           const int* __restrict__ mode, int first, ColGeom g, int* state_all, int cap,
                                                           int* __restrict__ n_final, int* __restrict__ pending, int* __restrict__ status,
                                                           int* __restrict__ events, int4* __restrict__ row_tags) {
    const SlotCall c{frame_off, n_ticks, rows6, reset, mode, first, g.streams, g.max_tracks, g.forget_after, state_all, cap, n_final, pending, status,
                     events};
    ColoursWalk v{info, info_base, state_all + (size_t)blockIdx.x * CL_ST_INTS + CL_ST_ACC, row_tags};
    slot_walk(c, v);
}

}  // namespace

void launch_colours_sample(const uint8_t* frames, const int* frame_off, int n_frames, int max_rows, const int* rows6, const int* state, const int* reset,
                           int first, const ColGeom& g, int info_base, int* info, hipStream_t s) {
    if (n_frames <= 0 || max_rows <= 0) return;
    hipLaunchKernelGGL(colours_sample_kernel, dim3(n_frames, max_rows), dim3(256), 0, s, frames, frame_off, rows6, state, reset, first, g, info_base,
                       reinterpret_cast<int4*>(info));
    KCHECK();
}

void launch_colours_walk(const int* frame_off, int n_ticks, const int* rows6, const int* info, int info_base, const int* reset, const int* mode,
                         int first, const ColGeom& g, int* state, int cap, int* n_final, int* pending, int* status, int* events, int* row_tags,
                         hipStream_t s) {
    hipLaunchKernelGGL(colours_walk_kernel, dim3(g.streams), dim3(T), 0, s, frame_off, n_ticks, rows6, reinterpret_cast<const int4*>(info), info_base,
                       reset, mode, first, g, state, cap, n_final, pending, status, events, reinterpret_cast<int4*>(row_tags));
    KCHECK();
}

}  // namespace aic
