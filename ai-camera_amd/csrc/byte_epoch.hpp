// byte_epoch.hpp -- the BYTE life cycle on the device, once: what the ByteTrack and the BoT-SORT epoch kernels share (device code only;
// included by kernels_bytetrack.hip and kernels_botsort.hip).
//
// ONE block of 512 threads walks the frames of one stream: thread i <-> list position i / detection i / slot i.  A launch holds one
// block per stream of a bank (blockIdx.x = stream: its own table, its own slice of the HBM scratch, its own rows of the group); a
// single tracker is the bank of one.  Per frame:
//   bands (high: s > high, second: low < s < high) -> pool = activated tracked ++ lost, velocities of the tracks that are not Tracked
//   zeroed, Kalman predict (unconfirmed tracks are not predicted) -> stage 1 (pool x high band, match_thresh) -> stage 2 (pool's unmatched
//   Tracked x second band, IoU, 0.5) -> stage 3 (unconfirmed x high band left over, 0.7) -> new tracks -> lost timeout -> list rebuild
//   (joint / sub semantics) -> duplicate removal -> output rows.
// Every assignment problem is lap.lapjv(extend_cost, cost_limit) restated: the square extended matrix of side T + N (top-left the costs,
// bottom-right 0, elsewhere fp32(thresh / 2)) through the SciPy-tie LSAP; a real pair is a row < T on a column < N.
//
// byte_epoch<V> is instantiated with a variant V, a type of static __forceinline__ members that states what its tracker does differently:
//   Args (EpochCall c, Params prm, int lds_bytes, ...), Lds (ByteLds or a type derived from it), Table, Ctx (per-block state of its own)
//   EXTRA_LDS_BYTES, carve_extra      LDS arrays of its own
//   table                             the stream's table
//   high, low                         the band thresholds
//   detection                         the measurement of a detection (L.meas) and what else it keeps of one
//   mean_box, zero_velocity           the box of a filter mean; the velocities a pooled track that is not Tracked loses
//   predict                           the filter step of the pool (and what happens to the unconfirmed tracks)
//   cost_pass, post_solve             between the matrix fill and the solve; behind the solve, on both of its exits
//   commit                            matched rows take their detections: the filter update, with the variant's own barriers and fences
//   activate, initiate                a new track: per-thread scalars of its own; the filters, one wavefront per track
//   outputs                           which tracks of the tracked list are output
//   load_slot, store_slot, begin, finish   table and header fields of its own
// `app` tells cost_pass, post_solve and commit that the stage is one that looks at appearance (stages 1 and 3).  The skeleton never asks
// which variant it runs.
#pragma once
#include "kernels.hpp"
#include "trk_dev.hpp"
#include "trk_math.hpp"
#include "trk_wave.hpp"
#include "bytetrack.hpp"

namespace aic {
namespace {

constexpr int BYTE_LDS_BYTES = 159 * 1024;                       // dynamic LDS of a block: with 512 threads, one block per CU
// L.wcnt[NW + ...]: read-offs, LSAPs, error, largest side, appearance pairs (BoT-SORT)
enum { BW_FAST = 1, BW_LSAP = 2, BW_ERR = 3, BW_SIDE = 4, BW_APP = 5, BW_N = 8 };

struct ByteLds : LsapLds {
    // track table by slot
    int *id, *state, *act, *start, *end, *cls;
    float *score, *mean;            // mean [cap][8]
    // lists (slots) and per-position scratch
    int *tl, *ll, *tl2, *ll2, *pool, *unc, *rows, *lostn, *newd, *fre, *mrow, *mrow1, *flag;
    // detections of the frame; meas = the filter's measurement of the box
    float *tlwh, *meas, *dconf;
    int *dcls, *hi, *lo, *cols, *mcol, *hm;
    int* wcnt;                      // [NW + BW_N]
    float* arena;
    int arena_floats;
};

// bytes of the carve in front of the arena, and the arena that leaves
template <class V> constexpr size_t byte_fixed_bytes() {
    return LSAP_LDS_BYTES + (size_t)TRK_DEV_NMAX * (25 * 4 + 4 + 32 + 16 + 16 + 4) + 4 * (NW + BW_N) + V::EXTRA_LDS_BYTES;
}
template <class V> constexpr int byte_arena_floats() { return (int)((BYTE_LDS_BYTES - byte_fixed_bytes<V>()) / 4); }

template <class V>
__device__ __forceinline__ typename V::Lds byte_carve(char* base, int total_bytes) {
    typename V::Lds L;
    LdsTake take{base};
    const size_t M = TRK_DEV_NMAX;
    carve_lsap(L, take);
    // one statement per field: a table of pointers-to-fields walked in a loop lands in scratch
#define BYTE_TAKE(f) L.f = (int*)take(4 * M)
    BYTE_TAKE(id); BYTE_TAKE(state); BYTE_TAKE(act); BYTE_TAKE(start); BYTE_TAKE(end); BYTE_TAKE(cls);
    BYTE_TAKE(tl); BYTE_TAKE(ll); BYTE_TAKE(tl2); BYTE_TAKE(ll2); BYTE_TAKE(pool); BYTE_TAKE(unc); BYTE_TAKE(rows); BYTE_TAKE(lostn); BYTE_TAKE(newd);
    BYTE_TAKE(fre); BYTE_TAKE(mrow); BYTE_TAKE(mrow1); BYTE_TAKE(flag); BYTE_TAKE(dcls); BYTE_TAKE(hi); BYTE_TAKE(lo); BYTE_TAKE(cols); BYTE_TAKE(mcol); BYTE_TAKE(hm);
#undef BYTE_TAKE
    V::carve_extra(L, take);
    L.score = (float*)take(4 * M);
    L.mean = (float*)take(32 * M);
    L.tlwh = (float*)take(16 * M); L.meas = (float*)take(16 * M); L.dconf = (float*)take(4 * M);
    L.wcnt = (int*)take(4 * (NW + BW_N));
    L.arena = (float*)take.p;
    L.arena_floats = (int)((total_bytes - (take.p - base)) / 4);
    return L;
}

// the IoU distance (iou_dist of trk_math.hpp) of slot's box to detection j, fused with the detection's score: 1 - (1 - d) * s
template <class V>
__device__ __forceinline__ float byte_cost(const typename V::Lds& L, int slot, int j, bool fuse) {
    float b[4];
    V::mean_box(L.mean + slot * 8, b);
    float x = iou_dist(b, L.tlwh + j * 4);
    if (fuse) x = 1.0f - (1.0f - x) * L.dconf[j];                 // fuse_score
    return x;
}

// linear_assignment(cost, thresh) of matching.py for rows (slots) x cols (detections), block-wide.
// Out: L.mrow[r] = column of row r or -1, L.mcol[c] = row of column c or -1.  *err = 3 when the extended side exceeds the LSAPs.
// Ls: the same carve in LDS, what the (noinline) LSAPs get a reference to -- a reference to the kernel's own copy would put it in scratch.
// hbm: the block's HBM scratch, for a matrix beyond the arena.
template <class V>
__device__ void byte_assign(const typename V::Lds& L, const typename V::Lds& Ls, const typename V::Args& a, const typename V::Table& tbl,
                            typename V::Ctx& x, float* hbm, const int* rows, int nr, const int* cols, int nc, int d0, bool fuse, bool app,
                            float th, int* err) {
    const int tid = threadIdx.x;
    for (int r = tid; r < nr; r += BT) L.mrow[r] = -1;
    for (int c = tid; c < nc; c += BT) L.mcol[c] = -1;
    __syncthreads();
    if (nr == 0 || nc == 0) return;                               // matching.py: cost_matrix.size == 0
    const int S = nr + nc;
    if (S > TRK_DEV_NMAX) { if (tid == 0) *err = 3; __syncthreads(); return; }
    if (tid == 0) L.wcnt[NW + BW_SIDE] = max(L.wcnt[NW + BW_SIDE], S);
    float* ext = S * S <= L.arena_floats ? L.arena : hbm;
    const float half = th * 0.5f;
    for (int e = tid; e < S * S; e += BT) {
        const int r = e / S, c = e - r * S;
        float v;
        if (r < nr && c < nc) v = byte_cost<V>(L, rows[r], cols[c], fuse);
        else v = (r < nr) != (c < nc) ? half : 0.f;
        ext[e] = v;
    }
    __threadfence_block();
    __syncthreads();
    V::cost_pass(L, a, tbl, x, ext, S, rows, nr, cols, nc, d0, app);
    if (!a.prm.no_fast) {
        // Unique optimum read off the costs: the extended problem minimises sum over real pairs of (c - thresh) (+ a constant).  If every
        // row and every column holds at most one entry below thresh and no entry equals it, those entries form a matching, every
        // other pair adds a positive term: it is the ONLY optimum, so SciPy returns exactly these real pairs whatever its tie rules.
        int* rcnt = L.pred; int* rarg = L.colof; int* ccnt = L.rowof;
        bool ok = true;
        if (tid < nr) {
            int cnt = 0, arg = -1;
            for (int c = 0; c < nc; ++c) {
                const float v = ext[tid * S + c];
                if (v < th) { ++cnt; arg = c; }
                if (v == th) ok = false;
            }
            rcnt[tid] = cnt, rarg[tid] = arg;
            ok = ok && cnt <= 1;
        }
        if (tid < nc) {
            int cnt = 0;
            for (int r = 0; r < nr; ++r) cnt += ext[r * S + tid] < th ? 1 : 0;
            ccnt[tid] = cnt;
            ok = ok && cnt <= 1;
        }
        if (__syncthreads_and(ok)) {
            if (tid < nr && rarg[tid] >= 0) { L.mrow[tid] = rarg[tid]; L.mcol[rarg[tid]] = tid; }
            if (tid == 0) L.wcnt[NW + BW_FAST] += 1;
            __syncthreads();
            V::post_solve(L, x, ext, S, rows, nr, cols, fuse, app);
            return;
        }
    }
    if (tid == 0) L.wcnt[NW + BW_LSAP] += 1;
    if (tid < 64) {
        const bool ok = S <= 64 ? lsap_wave64(ext, S, S, Ls, tid) : S <= 128 ? lsap_wave_reg<2>(ext, S, S, Ls, tid) : lsap_wave(ext, S, S, Ls, tid);
        if (!ok && tid == 0) *err = 2;                            // cannot happen: the extended matrix is finite and square
    }
    __syncthreads();
    if (tid < nr) {
        const int c = L.asg[tid];
        if (c >= 0 && c < nc) { L.mrow[tid] = c; L.mcol[c] = tid; }
    }
    __syncthreads();
    V::post_solve(L, x, ext, S, rows, nr, cols, fuse, app);
}

// The epoch kernel.  smem: the block's dynamic LDS; s_lds: a __shared__ home for the carve (see byte_assign); x: the variant's own state.
template <class V>
__device__ __forceinline__ void byte_epoch(const typename V::Args& a, char* smem, typename V::Lds& s_lds, typename V::Ctx& x) {
    const typename V::Lds L = byte_carve<V>(smem, a.lds_bytes);
    if (threadIdx.x == 0) s_lds = L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const auto& P = a.prm;
    const int cap = P.cap;
    int* err = L.wcnt + NW + BW_ERR;
    // ---- this block's stream: frame range, table, HBM scratch
    const typename V::Table tbl = V::table(a, blockIdx.x);
    EpochStream st;
    if (!epoch_stream(a.c, &tbl.hdr->err, st)) return;
    const EpochDets& dets = a.c.dets;
    const EpochOut& out = a.c.out;

    // ---- load the table
    int ntl = tbl.hdr->n_tracked, nll = tbl.hdr->n_lost, next_id = tbl.hdr->next_id, frame = tbl.hdr->frame_id;
    if (tid < cap) {
        const BtTrack t = tbl.trk[tid];
        L.id[tid] = t.id, L.state[tid] = t.state, L.act[tid] = t.act, L.start[tid] = t.start, L.end[tid] = t.end, L.cls[tid] = t.cls;
        L.score[tid] = t.score;
        V::load_slot(L, tbl, tid);
    }
    for (int e = tid; e < cap * 8; e += BT) L.mean[e] = tbl.mean[e];
    if (tid < ntl) L.tl[tid] = tbl.tl[tid];
    if (tid < nll) L.ll[tid] = tbl.ll[tid];
    if (tid == 0) {
        *err = 0; L.wcnt[NW + BW_FAST] = 0; L.wcnt[NW + BW_LSAP] = 0; L.wcnt[NW + BW_SIDE] = tbl.hdr->max_side;
        V::begin(L, x);
    }
    __syncthreads();
    int fi = a.c.f0;
    for (; fi < st.kend; ++fi) {
        const int f = st.row0 + fi * a.c.frame_stride;
        ++frame;
        const int n = dets.frame_n[f], d0 = dets.frame_d0[f];
        if (n > TRK_DEV_NMAX) { if (tid == 0) *err = 3; break; }
        if (tid < n) {
            const float* b = dets.tlwh + (size_t)(d0 + tid) * 4;
            const float bx = b[0], by = b[1], bw = b[2], bh = b[3];
            L.tlwh[tid * 4 + 0] = bx, L.tlwh[tid * 4 + 1] = by, L.tlwh[tid * 4 + 2] = bw, L.tlwh[tid * 4 + 3] = bh;
            L.dconf[tid] = dets.conf[d0 + tid];
            L.dcls[tid] = dets.cls[d0 + tid];
            V::detection(L, a, x, tid, d0 + tid, bx, by, bw, bh);
        }
        const float s = tid < n ? dets.conf[d0 + tid] : 0.f;
        const int nh = block_compact(tid < n && s > V::high(P), tid, L.hi, L.wcnt);
        const int nlo = block_compact(tid < n && s > V::low(P) && s < V::high(P), tid, L.lo, L.wcnt);
        // ---- unconfirmed / tracked / pool = joint(tracked, lost)
        const int tsl = tid < ntl ? L.tl[tid] : 0;
        const int ntk = block_compact(tid < ntl && L.act[tsl], tsl, L.pool, L.wcnt);
        const int nun = block_compact(tid < ntl && !L.act[tsl], tsl, L.unc, L.wcnt);
        if (tid < nll) L.pool[ntk + tid] = L.ll[tid];
        const int np = ntk + nll;
        __syncthreads();
        if (tid < np && L.state[L.pool[tid]] != BT_TRACKED) V::zero_velocity(L.mean + L.pool[tid] * 8);
        __syncthreads();
        V::predict(L, a, tbl, f, np, nun);
        __threadfence_block();
        __syncthreads();

        // ---- stage 1: pool x high band
        byte_assign<V>(L, s_lds, a, tbl, x, st.ext, L.pool, np, L.hi, nh, d0, P.fuse != 0, true, P.match_thresh, err);
        if (*err) break;
        V::commit(L, a, tbl, x, L.pool, np, L.hi, d0, true);
        const int nr2 = block_compact(tid < np && L.mrow[tid] < 0 && L.state[L.pool[tid]] == BT_TRACKED, tid < np ? L.pool[tid] : 0, L.rows, L.wcnt);
        if (tid < nh) L.hm[tid] = L.mcol[tid] >= 0;
        if (tid < np && L.mrow[tid] >= 0) {                       // update (Tracked) / re_activate (Lost -> refound)
            const int sl = L.pool[tid], j = L.hi[L.mrow[tid]];
            L.state[sl] = BT_TRACKED, L.act[sl] = 1, L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j];
        }
        __syncthreads();

        // ---- stage 2: the pool's unmatched Tracked tracks x second band, IoU distance, no fusion, no appearance
        byte_assign<V>(L, s_lds, a, tbl, x, st.ext, L.rows, nr2, L.lo, nlo, d0, false, false, P.second_thresh, err);
        if (*err) break;
        V::commit(L, a, tbl, x, L.rows, nr2, L.lo, d0, false);
        if (tid < nr2) {
            const int sl = L.rows[tid], c = L.mrow[tid];
            if (c >= 0) {
                const int j = L.lo[c];
                L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j], L.act[sl] = 1;
            } else L.state[sl] = BT_LOST;                          // mark_lost
        }
        const int nlost = block_compact(tid < nr2 && L.mrow[tid] < 0, tid < nr2 ? L.rows[tid] : 0, L.lostn, L.wcnt);

        // ---- stage 3: unconfirmed x the high band left over, the cost of stage 1, 0.7
        const int nh3 = block_compact(tid < nh && !L.hm[tid], tid < nh ? L.hi[tid] : 0, L.cols, L.wcnt);
        byte_assign<V>(L, s_lds, a, tbl, x, st.ext, L.unc, nun, L.cols, nh3, d0, P.fuse != 0, true, P.unconf_thresh, err);
        if (*err) break;
        V::commit(L, a, tbl, x, L.unc, nun, L.cols, d0, true);
        if (tid < nun) {
            const int sl = L.unc[tid], c = L.mrow[tid];
            if (c >= 0) {
                const int j = L.cols[c];
                L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j], L.act[sl] = 1;
            } else L.state[sl] = BT_REMOVED;                       // mark_removed
        }
        // ---- lost tracks past max_time_lost (the old lost list; refound ones have end == frame)
        if (tid < nll) {
            const int sl = L.ll[tid];
            if (L.state[sl] == BT_LOST && frame - L.end[sl] > P.max_lost) L.state[sl] = BT_REMOVED;
        }
        __syncthreads();
        // ---- lists: tracked = joint(joint([t in tracked if Tracked], activated), refound); lost = sub(sub(lost, tracked) + newly lost, removed).
        // Taken BEFORE the new tracks get their slots: a slot freed in this frame (a removed track) may be handed out again below.
        const int nnew = block_compact(tid < nh3 && L.mcol[tid] < 0 && L.dconf[tid < nh3 ? L.cols[tid] : 0] >= P.new_thresh,
                                       tid < nh3 ? L.cols[tid] : 0, L.newd, L.wcnt);  // new tracks: the high band left after stage 3, s >= new_thresh
        if (tid < cap) L.flag[tid] = 0;                            // slots of the live tracks (capacity first: the lists below then fit)
        __syncthreads();
        if (tid < ntl && L.state[L.tl[tid]] != BT_REMOVED) L.flag[L.tl[tid]] = 1;
        if (tid < nll && L.state[L.ll[tid]] != BT_REMOVED) L.flag[L.ll[tid]] = 1;
        __syncthreads();
        const int nfree = block_compact(tid < cap && !L.flag[tid], tid, L.fre, L.wcnt);
        if (nnew > nfree) { if (tid == 0) *err = 1; break; }
        const int c1 = block_compact(tid < ntl && L.state[tsl] == BT_TRACKED, tsl, L.tl2, L.wcnt);
        const int lsl = tid < nll ? L.ll[tid] : 0;
        const int c3 = block_compact(tid < nll && L.state[lsl] == BT_TRACKED, lsl, L.tl2 + c1 + nnew, L.wcnt);
        const int c4 = block_compact(tid < nll && L.state[lsl] == BT_LOST, lsl, L.ll2, L.wcnt);
        if (tid < nlost) L.ll2[c4 + tid] = L.lostn[tid];
        // ---- new tracks in detection order, on the lowest free slots
        if (tid < nnew) {                                         // STrack.activate
            const int sl = L.fre[tid], j = L.newd[tid];
            L.id[sl] = next_id + tid, L.state[sl] = BT_TRACKED, L.act[sl] = frame == 1, L.start[sl] = frame, L.end[sl] = frame;
            L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j];
            V::activate(L, sl, j);
            L.tl2[c1 + tid] = sl;
        }
        V::initiate(L, a, tbl, nnew, d0);
        next_id += nnew;
        __threadfence_block();
        __syncthreads();
        const int na = c1 + nnew + c3, nb = c4 + nlost;
        // ---- remove_duplicate_stracks: pairs at IoU distance < 0.15, the younger (end - start) of the two is dropped, ties drop the tracked one
        L.hm[tid] = 0, L.mrow1[tid] = 0;                         // drop flags of the tracked / lost lists
        __syncthreads();
        for (int e = tid; e < na * nb; e += BT) {
            const int p = e / nb, q = e - p * nb;
            const int sp = L.tl2[p], sq = L.ll2[q];
            float bp[4], bq[4];
            V::mean_box(L.mean + sp * 8, bp);
            V::mean_box(L.mean + sq * 8, bq);
            if (iou_dist(bp, bq) < P.dup_dist) {
                if (L.end[sp] - L.start[sp] > L.end[sq] - L.start[sq]) L.mrow1[q] = 1; else L.hm[p] = 1;
            }
        }
        __syncthreads();
        const int tsl2 = tid < na ? L.tl2[tid] : 0, lsl2 = tid < nb ? L.ll2[tid] : 0;
        ntl = block_compact(tid < na && !L.hm[tid], tsl2, L.tl, L.wcnt);
        nll = block_compact(tid < nb && !L.mrow1[tid], lsl2, L.ll, L.wcnt);

        // ---- outputs: the variant's choice among the tracked list, list order; w and h clamped at 0
        const int* olist;
        const int no = V::outputs(L, ntl, olist);
        if (tid == 0) out.n_tracks[f] = no;
        if (tid < no && tid < out.max_rows) {
            const int sl = olist[tid];
            float b[4];
            V::mean_box(L.mean + sl * 8, b);
            const float x1 = b[0], y1 = b[1];
            const float w = b[2] > 0.f ? b[2] : 0.f, h = b[3] > 0.f ? b[3] : 0.f;
            write_row(out, f, tid, x1, y1, x1 + w, y1 + h, L.id[sl], L.cls[sl], L.score[sl]);
        }
        __syncthreads();
    }
    // ---- write back (on an error the tracker stops: the host refuses further updates)
    __syncthreads();
    const int e = *err;
    if (e == 0) {
        if (tid < cap) {
            BtTrack t;
            t.id = L.id[tid], t.state = L.state[tid], t.act = L.act[tid], t.start = L.start[tid], t.end = L.end[tid], t.cls = L.cls[tid];
            t.score = L.score[tid], t.pad = 0;
            tbl.trk[tid] = t;
            V::store_slot(L, tbl, tid);
        }
        for (int i = tid; i < cap * 8; i += BT) tbl.mean[i] = L.mean[i];
        if (tid < ntl) tbl.tl[tid] = L.tl[tid];
        if (tid < nll) tbl.ll[tid] = L.ll[tid];
    }
    if (tid == 0) {
        auto* h = tbl.hdr;
        if (e == 0) h->n_tracked = ntl, h->n_lost = nll, h->next_id = next_id, h->frame_id = frame;
        else h->err = e, h->err_frame = fi;
        h->n_fast += L.wcnt[NW + BW_FAST], h->n_lsap += L.wcnt[NW + BW_LSAP], h->max_side = L.wcnt[NW + BW_SIDE];
        V::finish(h, L, x);
    }
}

}  // namespace
}  // namespace aic
