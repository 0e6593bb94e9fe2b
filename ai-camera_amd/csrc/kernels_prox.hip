// kernels_prox.hip -- the kernel of the proximity stage (prox.hpp).  Integer arithmetic only; tests/prox_oracle.py is
// the specification.  No floating point, no scratch.
//
// prox_walk_kernel    one block of 512 threads per stream, the launch's ticks in order: the life cycle is slot_walk.hpp's, ProxWalk states
//                     what is this stage's.  A thread is slot t of the table AND row t of the frame.  load_row finds the FIRST row of an
//                     id itself (as the heat walk does) and places the row on the ground; commit measures the slot's speed.  The pair
//                     pass lives in post_tick, behind the commits, where a thread knows its row's slot:
//                       1. the tick's positions, heights and slots go to LDS; the entries of every slot taken anew this tick are cleared
//                          in the resident pair table (HBM), max_tracks - 1 of them per new slot, all threads side by side;
//                       2. thread i builds row i of the NEAR graph as sixteen words of a 512 x 512 bit matrix in LDS (word-major, so a
//                          wave's accesses to word w fall into 64 different banks); the other row's data are broadcast reads;
//                       3. components by min-label propagation over set bits (pull and push, so that an upper triangle is enough) with
//                          pointer jumping, swept until a block-wide flag stays clear;
//                       4. the owner of pair (i, j), the thread of the LOWER row i, reads, judges and writes the pair's entry -- no
//                          atomics on the table -- and leaves the LINKED graph's upper triangle in a second bit matrix and the pairs that
//                          raised an event in the first one, whose near bits nobody needs any more;
//                       5. components again, over the linked graph: parties; the smallest id and the size of a component through LDS
//                          atomics at its label;
//                       6. events are placed by a block scan over per-row counts and the row's event bits in order of j, which is the
//                          oracle's order (row i, row j); a pair's entry is read again for its counters;
//                       7. tags, the record.
//                     Static LDS: 32 KiB slot table + 4 KiB lists (slot_walk.hpp) + 64 KiB two bit matrices + 20 KiB row arrays, 123 216
//                     bytes in all: one block per CU, which a walk of one block per stream is anyway.
#include <climits>

#include "prox.hpp"
#include "slot_walk.hpp"

namespace aic {

namespace {

constexpr int T = PX_TRACKS_MAX;
constexpr int NW = T / 32;                                                   // words of a row of the bit matrices
enum { C_COUNTED = 0, C_PLACED, C_NEAR2, C_LINKED, C_PARTIES, C_SINGLES, C_RUN, C_STILL, C_LINK, C_UNLINK, C_MAXNEAR, C_MAXPARTY, C_N };

struct ProxWalk {
    static constexpr int ARRAYS = PX_ARRAYS, ST_INTS = PX_ST_INTS, EVENT_INTS = PX_EVENT_INTS;
    struct Row {
        int flags, gx, gy, hc;
        bool placed, fresh;
        int gait, v;                                                         // of the row's slot, behind commit
    };
    const int* rows6;
    ProxGeom g;
    ProxRules r;
    ProxGround m;
    int2* pairs;                                                             // the stream's triangle
    ProxOut o;
    int kk, frame;                                                           // the launch's tick and the stream's frame post_tick is at
    int *s_rid, *s_rok, *s_gx, *s_gy, *s_hc, *s_rslot, *s_label, *s_minid, *s_size, *s_fresh, *s_cnt;
    unsigned (*s_adj)[T], (*s_lnk)[T];

    __device__ __forceinline__ Row load_row(int row, bool in) const {
        const int tid = threadIdx.x;
        Row x{0, 0, 0, 1, false, false, 0, 0};
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0, id = 0;
        bool ok = false;
        if (in) {
            const int* q = rows6 + (size_t)row * 6;
            x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3], id = q[4];
            ok = row_valid(x1, y1, x2, y2, PX_COORD_MAX);
        }
        __syncthreads();                                                     // the last tick's readers are through
        s_rid[tid] = id, s_rok[tid] = ok, s_fresh[tid] = 0;
        __syncthreads();
        if (ok) {
            bool dup = false;
            for (int j = 0; j < tid; ++j) dup = dup || (s_rok[j] && s_rid[j] == id);
            const bool nonempty = x1 < g.w && x2 >= 0 && y1 < g.h && y2 >= 0;
            x.flags = SLOT_F_VALID | (dup ? 0 : SLOT_F_FIRST) | (nonempty ? SLOT_F_NONEMPTY : 0);
            if (!dup && nonempty) {
                const int fx = prox_clamp(x1 + x2, 0, 2 * g.w - 1), fy = prox_clamp(2 * y2, 0, 2 * g.h - 1);
                x.hc = prox_clamp(y2 - y1, 1, 32767);
                if (r.metric == PROX_BODY) x.placed = true, x.gx = fx, x.gy = fy;
                else x.placed = prox_place(m, fx, fy, &x.gx, &x.gy);
                if (x.placed) x.flags |= PROX_F_PLACED;
            }
        }
        return x;
    }
    __device__ __forceinline__ void fresh(const SlotLds& L, int slot) const {
#pragma unroll
        for (int a = SLOT_A_SHARED; a < PX_ARRAYS; ++a) L.tab[a][slot] = 0;
        s_fresh[slot] = 1;
    }
    __device__ __forceinline__ void commit(const SlotLds& L, Row& row, int slot, bool fresh_slot, int frame_) const {
        const int was = L.tab[PX_A_PLACED][slot];                            // the frame of the last sighting + 1 if it was placed, else 0
        if (!fresh_slot && row.placed && was) {
            const int dt = frame_ - (was - 1);
            const int mv = prox_moved(r.metric, row.gx - L.tab[PX_A_GX][slot], row.gy - L.tab[PX_A_GY][slot], row.hc);
            const int v = prox_v_q8(L.tab[PX_A_VQ8][slot], L.tab[PX_A_GAIT][slot], prox_speed(mv, dt), r.speed_shift);
            L.tab[PX_A_VQ8][slot] = v;
            L.tab[PX_A_DIST][slot] = prox_sat_add(L.tab[PX_A_DIST][slot], mv);
            L.tab[PX_A_MAXV][slot] = imax(L.tab[PX_A_MAXV][slot], v);
            L.tab[PX_A_GAIT][slot] = prox_gait(v, r.still_speed, r.run_speed);
        }
        L.tab[PX_A_PLACED][slot] = row.placed ? frame_ + 1 : 0;
        if (row.placed) L.tab[PX_A_GX][slot] = row.gx, L.tab[PX_A_GY][slot] = row.gy;
        row.fresh = fresh_slot, row.gait = L.tab[PX_A_GAIT][slot], row.v = L.tab[PX_A_VQ8][slot];
        if (fresh_slot) row.flags |= PROX_F_NEW;
    }
    __device__ __forceinline__ void event(const SlotLds& L, int4* ev, int s, int e_rank) const {
        const int tid = threadIdx.x;
        slot_event_head(L, ev, s, L.tab[PX_A_LINKS][tid]);
        ev[2] = make_int4(L.tab[PX_A_DIST][tid], L.tab[PX_A_MAXV][tid], L.tab[PX_A_VQ8][tid], L.tab[PX_A_PTICKS][tid]);
        ev[3] = make_int4(L.tab[PX_A_MAXP][tid], L.tab[PX_A_GX][tid], L.tab[PX_A_GY][tid], L.tab[PX_A_GAIT][tid]);
    }
    __device__ __forceinline__ void post_emit(const SlotLds& L, bool em, int n_emit, int n_out) const {
        if (em) L.tab[SLOT_A_STATE][threadIdx.x] = 0;
        __syncthreads();                                                     // the slot's arrays are read before a row may take the slot
    }

    // sum (or max) of a per-thread value into s_cnt[k]: a wave's lanes first, then one LDS atomic per wave
    __device__ __forceinline__ void count(int k, int v) const {
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&s_cnt[k], v);
    }
    __device__ __forceinline__ void count_max(int k, int v) const {
        v = wave_max(v);
        if ((threadIdx.x & 63) == 0 && v) atomicMax(&s_cnt[k], v);
    }

    // The components of the graph whose edges are the set bits of M (a symmetric matrix or one triangle of it) among the placed rows:
    // s_label[i] becomes the smallest row of i's component; s_size and s_minid at that row its size and smallest id.  s_label[i] = i on
    // entry.  A sweep pulls the smallest label of the neighbours, pushes its own to them, then jumps along labels; a sweep in which nobody
    // lowered anything read only settled labels, so every edge joins equal labels and every label is its own label: the fixed point.
    __device__ __forceinline__ void components(unsigned (*M)[T], bool pl, int nw) const {
        const int tid = threadIdx.x;
        volatile int* lab = s_label;
        for (;;) {
            int ch = 0;
            if (pl) {
                int mn = lab[tid];
                for (int w = 0; w < nw; ++w)
                    for (unsigned bits = M[w][tid]; bits; bits &= bits - 1) mn = imin(mn, lab[(w << 5) + __ffs(bits) - 1]);
                for (int w = 0; w < nw; ++w)
                    for (unsigned bits = M[w][tid]; bits; bits &= bits - 1) {
                        const int j = (w << 5) + __ffs(bits) - 1;
                        if (lab[j] > mn && atomicMin(&s_label[j], mn) > mn) ch = 1;
                    }
                if (mn < lab[tid]) atomicMin(&s_label[tid], mn), ch = 1;
            }
            __syncthreads();
            if (pl) {
                const int l = lab[tid];
                int root = l;
                for (int p = lab[root]; p < root; p = lab[root]) root = p;
                if (root < l) atomicMin(&s_label[tid], root), ch = 1;
            }
            if (!__syncthreads_or(ch)) break;
        }
        s_size[tid] = 0, s_minid[tid] = INT_MAX;
        __syncthreads();
        if (pl) atomicAdd(&s_size[s_label[tid]], 1), atomicMin(&s_minid[s_label[tid]], s_rid[tid]);
        __syncthreads();
    }

    __device__ __forceinline__ void post_tick(const SlotLds& L, const Row& row, int slot, int off, int n, int& stopped) {
        const int tid = threadIdx.x, S = g.streams, s = blockIdx.x;
        const bool pl = slot >= 0 && row.placed;                             // a placed counted row
        const int nw = (n + 31) >> 5;
        __syncthreads();                                                     // the commits are through, s_list is free
        s_gx[tid] = row.gx, s_gy[tid] = row.gy, s_hc[tid] = row.hc, s_rslot[tid] = pl ? slot : -1, s_label[tid] = tid;
        if (tid < C_N) s_cnt[tid] = 0;
        // ---- 1. a slot taken anew: no state is inherited
        int n_fresh;
        const int f_rank = block_scan(row.fresh, L.w, n_fresh);
        if (row.fresh) L.list[f_rank] = slot;
        __syncthreads();
        for (int k = 0; k < n_fresh; ++k) {
            const int f = L.list[k];
            if (tid < g.max_tracks && tid != f) pairs[prox_pair_index(imin(tid, f), imax(tid, f))] = make_int2(0, 0);
        }
        __syncthreads();                                                     // (with its fence: the zeros land before an owner's write)
        // ---- 2. the near graph, row tid
        int n_near = 0;
        for (int w = 0; w < NW; ++w) {
            unsigned bits = 0;
            if (pl && w < nw) {
                const int j1 = imin(n, (w + 1) << 5);
                for (int j = w << 5; j < j1; ++j)
                    if (s_rslot[j] >= 0 && j != tid && prox_near(r, row.gx, row.gy, row.hc, s_gx[j], s_gy[j], s_hc[j])) bits |= 1u << (j & 31);
            }
            s_adj[w][tid] = bits;
            n_near += __popc(bits);
        }
        __syncthreads();
        // ---- 3. its components
        components(s_adj, pl, nw);
        count(C_COUNTED, slot >= 0), count(C_PLACED, pl), count(C_NEAR2, n_near), count_max(C_MAXNEAR, pl ? s_size[s_label[tid]] : 0);
        count(C_RUN, pl && row.gait == 3), count(C_STILL, pl && row.gait == 1);
        __syncthreads();
        s_label[tid] = tid;
        // ---- 4. pair state: the thread of the lower row owns the pair
        int c_ev = 0, c_link = 0, c_unlink = 0, c_linked = 0;
        for (int w = 0; w < NW; ++w) {
            unsigned lnk = 0, evt = 0;
            if (pl && w < nw && w >= (tid >> 5)) {
                const unsigned nearw = s_adj[w][tid];
                const int j1 = imin(n, (w + 1) << 5);
                for (int j = imax(w << 5, tid + 1); j < j1; ++j) {
                    const int sj = s_rslot[j];
                    if (sj < 0) continue;
                    const int a = imin(slot, sj), b = imax(slot, sj);
                    int2* e = pairs + prox_pair_index(a, b);
                    int2 v = make_int2(0, 0);
                    if (!s_fresh[a] && !s_fresh[b]) v = *e;
                    const int kind = prox_judge((nearw >> (j & 31)) & 1u, r.link_ticks, r.unlink_ticks, frame, &v.x, &v.y);
                    *e = v;
                    if (prox_linked(v.x)) lnk |= 1u << (j & 31), ++c_linked;
                    if (kind) {
                        evt |= 1u << (j & 31), ++c_ev;
                        if (kind == PROX_LINK) {
                            ++c_link;
                            atomicAdd(&L.tab[PX_A_LINKS][slot], 1), atomicAdd(&L.tab[PX_A_LINKS][sj], 1);
                        } else ++c_unlink;
                    }
                }
            }
            s_lnk[w][tid] = lnk, s_adj[w][tid] = evt;                        // (row tid's near bits are read by nobody else)
        }
        int n_ev;
        int k_ev = block_scan(c_ev, L.w, n_ev);                              // (its barriers: the linked graph is complete)
        count(C_LINK, c_link), count(C_UNLINK, c_unlink), count(C_LINKED, c_linked);
        // ---- 5. parties
        components(s_lnk, pl, nw);
        int party = -1, size = 0;
        if (pl) {
            party = s_minid[s_label[tid]], size = s_size[s_label[tid]];
            if (size >= 2) L.tab[PX_A_PTICKS][slot] = prox_sat_add(L.tab[PX_A_PTICKS][slot], 1);
            L.tab[PX_A_MAXP][slot] = imax(L.tab[PX_A_MAXP][slot], size);
        }
        const bool root = pl && s_label[tid] == tid;
        count(C_PARTIES, root && size >= 2), count(C_SINGLES, root && size == 1), count_max(C_MAXPARTY, size);
        // ---- 6. the tick's pair events, in order of (row i, row j)
        const size_t x = (size_t)kk * S + s;                                 // the frame within the launch
        if (c_ev) {
            for (int w = tid >> 5; w < nw && k_ev < o.cap_pairs; ++w)
                for (unsigned bits = s_adj[w][tid]; bits && k_ev < o.cap_pairs; bits &= bits - 1, ++k_ev) {
                    const int j = (w << 5) + __ffs(bits) - 1, sj = s_rslot[j];
                    const int2 v = pairs[prox_pair_index(imin(slot, sj), imax(slot, sj))];
                    const int linked = prox_linked(v.x), ida = s_rid[tid], idb = s_rid[j];
                    int4* ev = reinterpret_cast<int4*>(o.pair_events + (x * o.cap_pairs + k_ev) * PX_PAIR_EVENT_INTS);
                    ev[0] = make_int4(linked ? PROX_LINK : PROX_UNLINK, frame, imin(ida, idb), imax(ida, idb));
                    ev[1] = make_int4(linked ? 0 : frame - v.y, prox_distance(r.metric, row.gx, row.gy, row.hc, s_gx[j], s_gy[j], s_hc[j]),
                                      linked ? prox_on(v.x) : prox_off(v.x), 0);
                }
        }
        // ---- 7. tags and the record
        if (tid < n) {
            int4* tag = reinterpret_cast<int4*>(o.row_tags + (size_t)(off - o.row0 + tid) * PX_TAG_INTS);
            tag[0] = make_int4(row.gx, row.gy, slot >= 0 && row.gait ? row.v : -1, slot >= 0 ? row.gait : 0);
            tag[1] = make_int4(party, size, n_near, row.flags);
        }
        __syncthreads();                                                     // the counters are complete
        if (tid == 0) {
            int4* rec = reinterpret_cast<int4*>(o.records + x * PX_RECORD_INTS);
            const int par = s_cnt[C_PARTIES], sin = s_cnt[C_SINGLES];
            rec[0] = make_int4(frame, s_cnt[C_COUNTED], s_cnt[C_PLACED], s_cnt[C_NEAR2] >> 1);
            rec[1] = make_int4(s_cnt[C_MAXNEAR], s_cnt[C_LINKED], par, sin);
            rec[2] = make_int4(s_cnt[C_MAXPARTY], par + sin, s_cnt[C_RUN], s_cnt[C_STILL]);
            rec[3] = make_int4(s_cnt[C_LINK], s_cnt[C_UNLINK], 0, 0);
            o.n_pair_events[x] = n_ev;
        }
        ++kk, ++frame;
    }
    __device__ __forceinline__ void tail(const SlotCall& c, int k) const {
        for (; k < c.n_ticks; ++k) {                                         // a stopped stream: the tick it stopped at and all after
            const size_t x = (size_t)k * c.streams + blockIdx.x;
            const int off = c.frame_off[x], n = c.frame_off[x + 1] - off;
            if ((int)threadIdx.x < n) {
                int4* tag = reinterpret_cast<int4*>(o.row_tags + (size_t)(off - o.row0 + threadIdx.x) * PX_TAG_INTS);
                tag[0] = make_int4(-1, -1, -1, -1), tag[1] = make_int4(-1, -1, -1, -1);
            }
            if (threadIdx.x < 4) reinterpret_cast<int4*>(o.records + x * PX_RECORD_INTS)[threadIdx.x] = make_int4(-1, -1, -1, -1);
            if (threadIdx.x == 0) o.n_pair_events[x] = 0;
        }
    }
};

__global__ __launch_bounds__(512) void prox_walk_kernel(const int* __restrict__ frame_off, int n_ticks, const int* __restrict__ rows6,
                                                        const int* __restrict__ reset, const int* __restrict__ mode, int first, ProxGeom g,
                                                        int forget_after, ProxRules r, const ProxGround* __restrict__ grounds, int* state_all,
                                                        int* pairs, int cap, int* __restrict__ n_final, int* __restrict__ pending,
                                                        int* __restrict__ status, int* __restrict__ events, ProxOut o) {
    __shared__ int s_rows[10][T], s_cnt[C_N];
    __shared__ unsigned s_adj[NW][T], s_lnk[NW][T];
    const SlotCall c{frame_off, n_ticks, rows6, reset, mode, first, g.streams, g.max_tracks, forget_after, state_all, cap, n_final, pending, status, events};
    const int frame0 = first && reset[blockIdx.x] ? 0 : state_all[(size_t)blockIdx.x * PX_ST_INTS];
    ProxWalk v{rows6, g, r, grounds[blockIdx.x], reinterpret_cast<int2*>(pairs) + (size_t)blockIdx.x * ((size_t)g.max_tracks * (g.max_tracks - 1) / 2), o, 0, frame0,
               s_rows[0], s_rows[1], s_rows[2], s_rows[3], s_rows[4], s_rows[5], s_rows[6], s_rows[7], s_rows[8], s_rows[9], s_cnt, s_adj, s_lnk};
    slot_walk(c, v);
}

}  // namespace

void launch_prox_walk(const int* frame_off, int n_ticks, const int* rows6, const int* reset, const int* mode, int first, const ProxGeom& g,
                      int forget_after, const ProxRules& r, const ProxGround* grounds, int* state, int* pairs, int cap, int* n_final, int* pending,
                      int* status, int* events, const ProxOut& o, hipStream_t s) {
    hipLaunchKernelGGL(prox_walk_kernel, dim3(g.streams), dim3(T), 0, s, frame_off, n_ticks, rows6, reset, mode, first, g, forget_after, r, grounds, state,
                       pairs, cap, n_final, pending, status, events, o);
    KCHECK();
}

}  // namespace aic
