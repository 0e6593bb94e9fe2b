// kernels_bytetrack.hip -- ByteTrack on the device, k frames per launch (structures: bytetrack.hpp).
//
// Specification: BYTETracker.update() of the ByteTrack authors (yolox/tracker/byte_tracker.py, matching.py) as restated in
// tests/bytetrack_oracle.py, with its four deliberate changes (this project's IoU, the reference DeepSORT fp32 Kalman filter,
// per-tracker ids, SciPy's tie rules on lap's extended matrix).  The Kalman arithmetic is trk_math.hpp's, the LSAPs, the DPP
// reductions and the ordered compaction are trk_wave.hpp's (shared with the DeepSORT epoch kernel).
//
// ONE block of 512 threads walks the frames of one stream: thread i <-> list position i / detection i / slot i.  A launch holds one
// block per stream of a bank (blockIdx.x = stream: its own table, its own slice of the HBM scratch, its own rows of the group); a
// single tracker is the bank of one.  Per frame:
//   bands (high: s > track_thresh, second: low < s < track_thresh) -> pool = activated tracked ++ lost, Kalman predict (mean[7] = 0
//   first for lost tracks; unconfirmed tracks are not predicted) -> stage 1 (pool x high, fused IoU, match_thresh) -> stage 2 (pool's
//   unmatched Tracked x second band, IoU, 0.5) -> stage 3 (unconfirmed x high left over, fused, 0.7) -> new tracks -> lost timeout ->
//   list rebuild (joint / sub semantics) -> duplicate removal -> output rows.
// Every assignment problem is lap.lapjv(extend_cost, cost_limit) restated: the square extended matrix of side T + N (top-left the costs,
// bottom-right 0, elsewhere fp32(thresh / 2)) through the SciPy-tie LSAP; a real pair is a row < T on a column < N.
#include "kernels.hpp"
#include "trk_dev.hpp"
#include "trk_math.hpp"
#include "trk_wave.hpp"
#include "bytetrack.hpp"

namespace aic {

struct BtArgs {
    char* bank;                     // stream s: bt_table(bank + s * table_stride, cap)
    size_t table_stride;
    BtParams prm;
    EpochDets dets;
    int f0, k;                      // local frames [f0, f0 + k) of every stream, cut at stream_k[s]
    const int* stream_f0;           // [streams] local frame i of stream s = row stream_f0[s] + i * frame_stride of dets / out;
    const int* stream_k;            // [streams] frames of stream s in the call.  Both NULL: one stream, row = local frame
    int frame_stride;
    float* ext;                     // [streams][TRK_DEV_NMAX^2] extended matrices that do not fit the LDS arena
    EpochOut out;
    int lds_bytes;
};

namespace {

struct BtLds {
    // LSAP (trk_wave.hpp), side <= TRK_DEV_NMAX
    double *u, *v, *dist;
    int *pred, *rowof, *colof, *todo, *pos, *asg;
    // track table by slot
    int *id, *state, *act, *start, *end, *cls;
    float *score, *mean;            // mean [cap][8]
    // lists (slots) and per-position scratch
    int *tl, *ll, *tl2, *ll2, *pool, *unc, *rows, *lostn, *newd, *fre, *mrow, *mrow1, *flag;
    // detections of the frame
    float *tlwh, *xyah, *dconf;
    int *dcls, *hi, *lo, *cols, *mcol, *hm;
    int* wcnt;                      // [NW + 8]; [NW + 3] = error
    float* arena;
    int arena_floats;
};

__device__ __forceinline__ BtLds bt_carve(char* base, int total_bytes) {
    BtLds L;
    char* p = base;
    auto take = [&](size_t bytes) { char* q = p; p += (bytes + 15) & ~(size_t)15; return q; };
    const size_t M = TRK_DEV_NMAX;
    static_assert(TRK_DEV_NMAX == TRK_DEV_TMAX, "one side for tracks, detections and LSAP");
    L.u = (double*)take(8 * M); L.v = (double*)take(8 * M); L.dist = (double*)take(8 * M);
    // one statement per field: a table of pointers-to-fields walked in a loop lands in scratch
#define BT_TAKE(f) L.f = (int*)take(4 * M)
    BT_TAKE(pred); BT_TAKE(rowof); BT_TAKE(colof); BT_TAKE(todo); BT_TAKE(pos); BT_TAKE(asg);
    BT_TAKE(id); BT_TAKE(state); BT_TAKE(act); BT_TAKE(start); BT_TAKE(end); BT_TAKE(cls);
    BT_TAKE(tl); BT_TAKE(ll); BT_TAKE(tl2); BT_TAKE(ll2); BT_TAKE(pool); BT_TAKE(unc); BT_TAKE(rows); BT_TAKE(lostn); BT_TAKE(newd);
    BT_TAKE(fre); BT_TAKE(mrow); BT_TAKE(mrow1); BT_TAKE(flag); BT_TAKE(dcls); BT_TAKE(hi); BT_TAKE(lo); BT_TAKE(cols); BT_TAKE(mcol); BT_TAKE(hm);
#undef BT_TAKE
    L.score = (float*)take(4 * M);
    L.mean = (float*)take(32 * M);
    L.tlwh = (float*)take(16 * M); L.xyah = (float*)take(16 * M); L.dconf = (float*)take(4 * M);
    L.wcnt = (int*)take(4 * (NW + 8));
    L.arena = (float*)p;
    L.arena_floats = (int)((total_bytes - (p - base)) / 4);
    return L;
}

// track box (mean_to_tlwh of deepsort_oracle.py / track.py:133-151)
__device__ __forceinline__ void mean_box(const float* m, float b[4]) {
    float bw = 0.f, bh = m[3];
    if (bh > 0.f) bw = m[2] * bh; else bh = fmaxf(0.f, bh);
    b[0] = m[0] - bw / 2.0f, b[1] = m[1] - bh / 2.0f, b[2] = bw, b[3] = bh;
}
// 1 - IoU of box b against candidate c (tlwh), matching.py:13-106 (union floored at 1e-7), fp32
__device__ __forceinline__ float iou_dist(const float b[4], const float* c) {
    const float brx = b[0] + b[2], bry = b[1] + b[3];
    const float crx = c[0] + c[2], cry = c[1] + c[3];
    const float iw = fmaxf(0.f, fminf(brx, crx) - fmaxf(b[0], c[0]));
    const float ih = fmaxf(0.f, fminf(bry, cry) - fmaxf(b[1], c[1]));
    const float inter = iw * ih;
    const float uni = b[2] * b[3] + c[2] * c[3] - inter;
    return 1.0f - inter / fmaxf(uni, 1e-7f);
}

// linear_assignment(cost, thresh) of matching.py for rows (slots) x cols (detections), block-wide.
// Out: L.mrow[r] = column of row r or -1, L.mcol[c] = row of column c or -1.  *err = 3 when the extended side exceeds the LSAPs.
// Ls: the same carve in LDS, what the (noinline) LSAPs get a reference to -- a reference to the kernel's own copy would put it in scratch.
__device__ void bt_assign(const BtLds& L, const BtLds& Ls, const BtArgs& a, float* hbm, const int* rows, int nr, const int* cols, int nc, bool fuse, float th, int* err) {
    const int tid = threadIdx.x;
    for (int r = tid; r < nr; r += BT) L.mrow[r] = -1;
    for (int c = tid; c < nc; c += BT) L.mcol[c] = -1;
    __syncthreads();
    if (nr == 0 || nc == 0) return;                               // matching.py: cost_matrix.size == 0
    const int S = nr + nc;
    if (S > TRK_DEV_NMAX) { if (tid == 0) *err = 3; __syncthreads(); return; }
    if (tid == 0) L.wcnt[NW + 4] = max(L.wcnt[NW + 4], S);
    float* ext = S * S <= L.arena_floats ? L.arena : hbm;
    const float half = th * 0.5f;
    for (int e = tid; e < S * S; e += BT) {
        const int r = e / S, c = e - r * S;
        float x;
        if (r < nr && c < nc) {
            float b[4];
            mean_box(L.mean + rows[r] * 8, b);
            const int j = cols[c];
            x = iou_dist(b, L.tlwh + j * 4);
            if (fuse) x = 1.0f - (1.0f - x) * L.dconf[j];         // fuse_score: 1 - (1 - d) * s
        } else x = (r < nr) != (c < nc) ? half : 0.f;
        ext[e] = x;
    }
    __threadfence_block();
    __syncthreads();
    if (!a.prm.no_fast) {
        // Unique optimum read off the costs: the extended problem minimises sum over real pairs of (c - thresh) (+ a constant).  If every
        // row and every column holds at most one entry below thresh and no entry equals it, those entries form a matching, every
        // other pair adds a positive term: it is the ONLY optimum, so SciPy returns exactly these real pairs whatever its tie rules.
        int* rcnt = L.pred; int* rarg = L.colof; int* ccnt = L.rowof;
        bool ok = true;
        if (tid < nr) {
            int cnt = 0, arg = -1;
            for (int c = 0; c < nc; ++c) {
                const float x = ext[tid * S + c];
                if (x < th) { ++cnt; arg = c; }
                if (x == th) ok = false;
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
            if (tid == 0) L.wcnt[NW + 1] += 1;
            __syncthreads();
            return;
        }
    }
    if (tid == 0) L.wcnt[NW + 2] += 1;
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
}

}  // namespace

__global__ __launch_bounds__(TRK_DEV_TMAX) void bytetrack_epoch_kernel(BtArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ BtLds s_lds;
    const BtLds L = bt_carve(smem, a.lds_bytes);
    if (threadIdx.x == 0) s_lds = L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const BtParams& P = a.prm;
    const int cap = P.cap;
    int* err = L.wcnt + NW + 3;
    // ---- this block's stream: frame range, table, HBM scratch
    const int sid = blockIdx.x;
    const int row0 = a.stream_f0 ? a.stream_f0[sid] : 0;
    const int kend = a.stream_k ? min(a.f0 + a.k, a.stream_k[sid]) : a.f0 + a.k;
    if (a.f0 >= kend) return;                                     // nothing for this stream in this epoch: its table is not touched
    const BtTable tbl = bt_table(a.bank + (size_t)sid * a.table_stride, cap);
    float* hbm = a.ext + (size_t)sid * TRK_DEV_NMAX * TRK_DEV_NMAX;
    if (tbl.hdr->err) return;                                   // an earlier epoch of the call failed: the table is not a frame boundary

    // ---- load the table
    int ntl = tbl.hdr->n_tracked, nll = tbl.hdr->n_lost, next_id = tbl.hdr->next_id, frame = tbl.hdr->frame_id;
    if (tid < cap) {
        const BtTrack t = tbl.trk[tid];
        L.id[tid] = t.id, L.state[tid] = t.state, L.act[tid] = t.act, L.start[tid] = t.start, L.end[tid] = t.end, L.cls[tid] = t.cls;
        L.score[tid] = t.score;
    }
    for (int e = tid; e < cap * 8; e += BT) L.mean[e] = tbl.mean[e];
    if (tid < ntl) L.tl[tid] = tbl.tl[tid];
    if (tid < nll) L.ll[tid] = tbl.ll[tid];
    if (tid == 0) { *err = 0; L.wcnt[NW + 1] = 0; L.wcnt[NW + 2] = 0; L.wcnt[NW + 4] = tbl.hdr->max_side; }
    __syncthreads();
    float* cov = tbl.cov;
    int fi = a.f0;
    for (; fi < kend; ++fi) {
        const int f = row0 + fi * a.frame_stride;
        ++frame;
        const int n = a.dets.frame_n[f], d0 = a.dets.frame_d0[f];
        if (n > TRK_DEV_NMAX) { if (tid == 0) *err = 3; break; }
        if (tid < n) {
            const float* b = a.dets.tlwh + (size_t)(d0 + tid) * 4;
            const float x = b[0], y = b[1], w = b[2], h = b[3];
            L.tlwh[tid * 4 + 0] = x, L.tlwh[tid * 4 + 1] = y, L.tlwh[tid * 4 + 2] = w, L.tlwh[tid * 4 + 3] = h;
            // tlwh_to_xyah (detection.py:36-47)
            L.xyah[tid * 4 + 0] = x + w / 2.0f, L.xyah[tid * 4 + 1] = y + h / 2.0f, L.xyah[tid * 4 + 2] = h > 0.f ? w / h : 0.f, L.xyah[tid * 4 + 3] = h;
            L.dconf[tid] = a.dets.conf[d0 + tid];
            L.dcls[tid] = a.dets.cls[d0 + tid];
        }
        const float s = tid < n ? a.dets.conf[d0 + tid] : 0.f;
        const int nh = block_compact(tid < n && s > P.track_thresh, tid, L.hi, L.wcnt);
        const int nlo = block_compact(tid < n && s > P.low_thresh && s < P.track_thresh, tid, L.lo, L.wcnt);
        // ---- unconfirmed / tracked / pool = joint(tracked, lost)
        const int tsl = tid < ntl ? L.tl[tid] : 0;
        const int ntk = block_compact(tid < ntl && L.act[tsl], tsl, L.pool, L.wcnt);
        const int nun = block_compact(tid < ntl && !L.act[tsl], tsl, L.unc, L.wcnt);
        if (tid < nll) L.pool[ntk + tid] = L.ll[tid];
        const int np = ntk + nll;
        __syncthreads();
        if (tid < np && L.state[L.pool[tid]] != BT_TRACKED) L.mean[L.pool[tid] * 8 + 7] = 0.f;
        __syncthreads();
        for (int r = wv; r < np; r += NW) {
            const int sl = L.pool[r];
            kf_predict_wave(cov + (size_t)sl * 64, L.mean + sl * 8, lane);
        }
        __threadfence_block();
        __syncthreads();

        // ---- stage 1: pool x high band
        bt_assign(L, s_lds, a, hbm, L.pool, np, L.hi, nh, P.fuse != 0, P.match_thresh, err);
        if (*err) break;
        for (int r = wv; r < np; r += NW) {
            const int c = L.mrow[r];
            if (c >= 0) kf_update_wave(cov + (size_t)L.pool[r] * 64, L.mean + L.pool[r] * 8, L.xyah + L.hi[c] * 4, lane);
        }
        __threadfence_block();
        __syncthreads();
        const int nr2 = block_compact(tid < np && L.mrow[tid] < 0 && L.state[L.pool[tid]] == BT_TRACKED, tid < np ? L.pool[tid] : 0, L.rows, L.wcnt);
        if (tid < nh) L.hm[tid] = L.mcol[tid] >= 0;
        if (tid < np && L.mrow[tid] >= 0) {                       // update (Tracked) / re_activate (Lost -> refound)
            const int sl = L.pool[tid], j = L.hi[L.mrow[tid]];
            L.state[sl] = BT_TRACKED, L.act[sl] = 1, L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j];
        }
        __syncthreads();

        // ---- stage 2: the pool's unmatched Tracked tracks x second band, IoU distance, no fusion
        bt_assign(L, s_lds, a, hbm, L.rows, nr2, L.lo, nlo, false, P.second_thresh, err);
        if (*err) break;
        for (int r = wv; r < nr2; r += NW) {
            const int c = L.mrow[r];
            if (c >= 0) kf_update_wave(cov + (size_t)L.rows[r] * 64, L.mean + L.rows[r] * 8, L.xyah + L.lo[c] * 4, lane);
        }
        __threadfence_block();
        __syncthreads();
        if (tid < nr2) {
            const int sl = L.rows[tid], c = L.mrow[tid];
            if (c >= 0) {
                const int j = L.lo[c];
                L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j], L.act[sl] = 1;
            } else L.state[sl] = BT_LOST;                          // mark_lost
        }
        const int nlost = block_compact(tid < nr2 && L.mrow[tid] < 0, tid < nr2 ? L.rows[tid] : 0, L.lostn, L.wcnt);

        // ---- stage 3: unconfirmed x the high band left over, fused, 0.7
        const int nh3 = block_compact(tid < nh && !L.hm[tid], tid < nh ? L.hi[tid] : 0, L.cols, L.wcnt);
        bt_assign(L, s_lds, a, hbm, L.unc, nun, L.cols, nh3, P.fuse != 0, P.unconf_thresh, err);
        if (*err) break;
        for (int r = wv; r < nun; r += NW) {
            const int c = L.mrow[r];
            if (c >= 0) kf_update_wave(cov + (size_t)L.unc[r] * 64, L.mean + L.unc[r] * 8, L.xyah + L.cols[c] * 4, lane);
        }
        __threadfence_block();
        __syncthreads();
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
            L.tl2[c1 + tid] = sl;
        }
        for (int r = wv; r < nnew; r += NW) kf_initiate_wave(cov + (size_t)L.fre[r] * 64, L.mean + L.fre[r] * 8, L.xyah + L.newd[r] * 4, lane);
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
            mean_box(L.mean + sp * 8, bp);
            mean_box(L.mean + sq * 8, bq);
            if (iou_dist(bp, bq) < P.dup_dist) {
                if (L.end[sp] - L.start[sp] > L.end[sq] - L.start[sq]) L.mrow1[q] = 1; else L.hm[p] = 1;
            }
        }
        __syncthreads();
        const int tsl2 = tid < na ? L.tl2[tid] : 0, lsl2 = tid < nb ? L.ll2[tid] : 0;
        ntl = block_compact(tid < na && !L.hm[tid], tsl2, L.tl, L.wcnt);
        nll = block_compact(tid < nb && !L.mrow1[tid], lsl2, L.ll, L.wcnt);

        // ---- outputs: the activated tracks of the tracked list, list order
        const int osl = tid < ntl ? L.tl[tid] : 0;
        const int no = block_compact(tid < ntl && L.act[osl], osl, L.rows, L.wcnt);
        if (tid == 0) a.out.n_tracks[f] = no;
        if (tid < no && tid < a.out.max_rows) {
            const int sl = L.rows[tid];
            float b[4];
            mean_box(L.mean + sl * 8, b);
            const float x1 = b[0], y1 = b[1];
            const float w = b[2] > 0.f ? b[2] : 0.f, h = b[3] > 0.f ? b[3] : 0.f;
            int* r = a.out.rows + ((size_t)f * a.out.max_rows + tid) * 6;
            r[0] = (int)rintf(x1), r[1] = (int)rintf(y1), r[2] = (int)rintf(x1 + w), r[3] = (int)rintf(y1 + h);   // round half to even
            r[4] = L.id[sl], r[5] = L.cls[sl];
            a.out.conf[(size_t)f * a.out.max_rows + tid] = L.score[sl];
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
        }
        for (int i = tid; i < cap * 8; i += BT) tbl.mean[i] = L.mean[i];
        if (tid < ntl) tbl.tl[tid] = L.tl[tid];
        if (tid < nll) tbl.ll[tid] = L.ll[tid];
    }
    if (tid == 0) {
        BtHdr* h = tbl.hdr;
        if (e == 0) h->n_tracked = ntl, h->n_lost = nll, h->next_id = next_id, h->frame_id = frame;
        else h->err = e, h->err_frame = fi;
        h->n_fast += L.wcnt[NW + 1], h->n_lsap += L.wcnt[NW + 2], h->max_side = L.wcnt[NW + 4];
    }
}

static int bt_lds_bytes() { return 159 * 1024; }

void launch_bytetrack_epoch(char* bank, size_t table_stride, int streams, const BtParams& prm, const EpochDets& dets, int f0, int k,
                            const int* stream_f0, const int* stream_k, int frame_stride, float* ext, const EpochOut& out, hipStream_t s) {
    set_lds_limit(bytetrack_epoch_kernel, bt_lds_bytes());
    BtArgs a{bank, table_stride, prm, dets, f0, k, stream_f0, stream_k, frame_stride, ext, out, bt_lds_bytes()};
    hipLaunchKernelGGL(bytetrack_epoch_kernel, dim3(streams), dim3(TRK_DEV_TMAX), bt_lds_bytes(), s, a);
    KCHECK();
}

}  // namespace aic
