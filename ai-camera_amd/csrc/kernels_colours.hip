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
// colours_walk_kernel    one block of 512 threads per stream, the launch's ticks in order.  A thread is slot t of the table AND row t
//                        of the frame.  The eight small arrays of the table live in LDS for the launch (16 KiB); the accumulators
//                        (24 ints a slot, 48 KiB a stream) stay in HBM: a tick touches only the slots of its counted rows, some 30 of
//                        512, so loading and storing all of them per launch would move more bytes than it saves, and 64 KiB of LDS
//                        would leave one block per CU.  A slot's accumulators are written by the thread of its row and read by the
//                        thread of its slot only across a block barrier.
#include "colours.hpp"

namespace aic {

namespace {

constexpr int T = CL_TRACKS_MAX;

__device__ __forceinline__ bool coord_ok(int v) { return v >= -CL_COORD_MAX && v <= CL_COORD_MAX; }
__device__ __forceinline__ bool row_valid(int x1, int y1, int x2, int y2) {
    return coord_ok(x1) && coord_ok(y1) && coord_ok(x2) && coord_ok(y2) && x2 >= x1 && y2 >= y1;
}
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = imax(v, __shfl_xor(v, d));
    return v;
}

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
    bool go = (fresh || st[1] == 0) && row_valid(x1, y1, x2, y2);            // a stopped stream commits nothing
    if (go) {
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
            if (q[4] == rid || !row_valid(qx1, qy1, qx2, qy2)) continue;
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

__global__ __launch_bounds__(512) void colours_walk_kernel(const int* __restrict__ frame_off, int n_ticks, const int* __restrict__ rows6,
                                                           const int4* __restrict__ info, int info_base, const int* __restrict__ reset,
                                                           const int* __restrict__ mode, int first, ColGeom g, int* state_all, int cap,
                                                           int* __restrict__ n_final, int* __restrict__ pending, int* __restrict__ status,
                                                           int* __restrict__ events, int4* __restrict__ row_tags) {
    __shared__ int s_tab[CL_ARRAYS][T];
    __shared__ int s_live[T], s_list[T];
    __shared__ int s_w[8];
    int* s_id = s_tab[CL_A_ID];
    int* s_state = s_tab[CL_A_STATE];
    int* s_last = s_tab[CL_A_LAST];
    const int s = blockIdx.x, tid = threadIdx.x, S = g.streams;
    int* st = state_all + (size_t)s * CL_ST_INTS;
    int* acc_all = st + CL_ST_ACC;                                           // [slot][part][bin]
    const bool fresh = first && reset[s];
    int frame = fresh ? 0 : st[0];
    int stopped = fresh ? 0 : st[1];
#pragma unroll
    for (int a = 0; a < CL_ARRAYS; ++a) s_tab[a][tid] = fresh ? 0 : st[CL_ST_SLOTS + a * T + tid];
    int n_out = first ? 0 : n_final[s];
    __syncthreads();

    // ENDED slots (E, ranked e_rank in slot order) leave for the output list while it has room; they become free
    auto emit = [&](bool E, int e_rank, int n_E) {
        const int room = cap - n_out;
        const bool em = E && e_rank < room;
        if (em) {
            int4* ev = reinterpret_cast<int4*>(events + ((size_t)s * cap + n_out + e_rank) * CL_EVENT_INTS);
            const int* acc = acc_all + tid * 2 * CL_BINS;
            const int nu = s_tab[CL_A_NU][tid], nl = s_tab[CL_A_NL][tid];
            int tu, su, tl, sl;
            cl_describe(acc, nu, &tu, &su, reinterpret_cast<int*>(ev + 4));
            cl_describe(acc + CL_BINS, nl, &tl, &sl, reinterpret_cast<int*>(ev + 7));
            ev[0] = make_int4(s_state[tid] == 3 ? CL_FLUSHED : CL_EXPIRED, s, s_id[tid], s_tab[CL_A_CLS][tid]);
            ev[1] = make_int4(s_tab[CL_A_FIRST][tid], s_last[tid], s_tab[CL_A_SIGHT][tid], nu);
            ev[2] = make_int4(nl, tu, su, tl);
            ev[3] = make_int4(sl, tid, 0, 0);
            ev[10] = make_int4(0, 0, 0, 0), ev[11] = make_int4(0, 0, 0, 0);
            s_state[tid] = 0;
        }
        const int n_emit = n_E < room ? n_E : (room > 0 ? room : 0);
        n_out += n_emit;
        __syncthreads();                                                     // the accumulators are read before a row may take the slot
    };

    if (n_ticks == 0) {
        const int m = mode[s];
        if (m == CL_MODE_FLUSH && s_state[tid] == 1) s_state[tid] = 3;
        if (m != CL_MODE_NONE) {
            const bool E = tid < g.max_tracks && s_state[tid] >= 2;
            int n_E;
            const int e_rank = block_scan(E, s_w, n_E);
            emit(E, e_rank, n_E);
        }
    }
    int kk = 0;
    for (; kk < n_ticks && !stopped; ++kk) {
        const int x = kk * S + s;
        const int off = frame_off[x], n = frame_off[x + 1] - off;            // 0..512, checked by the host
        // ---- this thread as row tid
        int flags = 0, rid = 0, rcls = 0;
        const int4* inf = info + (size_t)(off + tid - info_base) * (CL_INFO_INTS / 4);
        if (tid < n) {
            flags = inf[0].x;
            rid = rows6[(size_t)(off + tid) * 6 + 4], rcls = rows6[(size_t)(off + tid) * 6 + 5];
        }
        const int need = CL_F_VALID | CL_F_FIRST | CL_F_NONEMPTY;
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
        int4 tag = make_int4(-1, -1, -1, -1);
        if (counted) {
            const bool fresh_slot = slot < 0;
            if (fresh_slot) {                                                // the k-th new row takes the k-th lowest free slot
                slot = s_list[new_rank];
                s_id[slot] = rid, s_state[slot] = 1, s_tab[CL_A_FIRST][slot] = frame, s_tab[CL_A_SIGHT][slot] = 0;
                s_tab[CL_A_NU][slot] = 0, s_tab[CL_A_NL][slot] = 0;
            }
            s_last[slot] = frame, s_tab[CL_A_CLS][slot] = rcls, s_tab[CL_A_SIGHT][slot] += 1;
            int4* acc4 = reinterpret_cast<int4*>(acc_all + slot * 2 * CL_BINS);
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                int& ns = s_tab[part ? CL_A_NL : CL_A_NU][slot];
                const bool add = (flags & (part ? CL_F_LOWER : CL_F_UPPER)) && ns < CL_SAMPLES_MAX;
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    int4 a = fresh_slot ? make_int4(0, 0, 0, 0) : acc4[part * 3 + q];
                    if (add) {
                        const int4 v = inf[1 + part * 3 + q];
                        a.x += v.x, a.y += v.y, a.z += v.z, a.w += v.w;
                    }
                    if (add || fresh_slot) acc4[part * 3 + q] = a;
                }
                if (add) ns += 1;
            }
            const int* acc = acc_all + slot * 2 * CL_BINS;
            const int nu = s_tab[CL_A_NU][slot], nl = s_tab[CL_A_NL][slot];
            if (nu > 0) tag.x = top_of(acc), tag.z = acc[tag.x] / nu;
            else tag.z = 0;
            if (nl > 0) tag.y = top_of(acc + CL_BINS), tag.w = acc[CL_BINS + tag.y] / nl;
            else tag.w = 0;
        }
        if (row_tags && tid < n) row_tags[off + tid] = tag;
        ++frame;
        __syncthreads();
    }
    __syncthreads();
    if (row_tags)                                                            // a stopped stream's rows: the tick it stopped at and all after
        for (; kk < n_ticks; ++kk) {
            const int x = kk * S + s;
            const int off = frame_off[x], n = frame_off[x + 1] - off;
            if (tid < n) row_tags[off + tid] = make_int4(-1, -1, -1, -1);
        }
#pragma unroll
    for (int a = 0; a < CL_ARRAYS; ++a) st[CL_ST_SLOTS + a * T + tid] = s_tab[a][tid];
    int n_pend;
    block_scan(tid < g.max_tracks && s_state[tid] >= 2, s_w, n_pend);
    if (tid == 0) st[0] = frame, st[1] = stopped, n_final[s] = n_out, pending[s] = n_pend, status[s] = stopped;
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
