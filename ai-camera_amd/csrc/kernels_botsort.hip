// kernels_botsort.hip -- BoT-SORT with ReID on the device, k frames per launch (structures: botsort.hpp).
//
// Specification: BoTSORT.update() of the BoT-SORT authors (tracker/bot_sort.py, matching.py, kalman_filter.py) as restated in
// tests/botsort_oracle.py, with the deliberate changes listed there.  The filter, the warp and the ordered feature sums are
// kf8wh_math.hpp's; the LSAPs and the ordered compaction are trk_wave.hpp's (shared with the DeepSORT and ByteTrack epoch kernels).
//
// ONE block of 512 threads walks the frames of one stream (a bank: one block per stream, each on its own table, smoothed features and
// HBM scratch): thread i <-> list position i / detection i / slot i.  Per frame:
//   bands -> pool = activated tracked ++ lost, Kalman predict (vw = vh = 0 first for tracks that are not Tracked) -> camera-motion warp of
//   pool and unconfirmed -> stage 1 (pool x high, min(fused IoU distance, gated appearance distance), match_thresh) -> stage 2 (pool's
//   unmatched Tracked x low band, IoU, 0.5) -> stage 3 (unconfirmed x high left over, the fused cost, 0.7) -> new tracks -> lost timeout ->
//   list rebuild -> duplicate removal -> output rows (every track of the tracked list).
// A committed match of stages 1 and 3 and a new track take the detection's feature into the slot's smoothed vector in HBM.
// Every assignment problem is lap.lapjv(extend_cost, cost_limit) restated as in kernels_bytetrack.hip.
#include "kernels.hpp"
#include "trk_dev.hpp"
#include "kf8wh_math.hpp"
#include "trk_wave.hpp"
#include "botsort.hpp"

namespace aic {

struct BsArgs {
    char* bank;                     // stream s: bs_table(bank + s * table_stride, cap, smooth + s * smooth_stride)
    size_t table_stride;
    float* smooth;                  // [streams][cap][dim] smoothed unit features
    size_t smooth_stride;           // floats between two streams' features
    BsParams prm;
    EpochDets dets;
    const float* warps;             // [rows, 6], indexed like dets.frame_n / out
    int f0, k;                      // local frames [f0, f0 + k) of every stream, cut at stream_k[s]
    const int* stream_f0;           // [streams] local frame i of stream s = row stream_f0[s] + i * frame_stride of dets / out / warps;
    const int* stream_k;            // [streams] frames of stream s in the call.  Both NULL: one stream, row = local frame
    int frame_stride;
    float* ext;                     // [streams][TRK_DEV_NMAX^2] extended matrices that do not fit the LDS arena
    EpochOut out;
    int lds_bytes;
};

namespace {

struct BsLds {
    // LSAP (trk_wave.hpp), side <= TRK_DEV_NMAX
    double *u, *v, *dist;
    int *pred, *rowof, *colof, *todo, *pos, *asg;
    // track table by slot
    int *id, *state, *act, *start, *end, *cls, *hasf;
    float *score, *mean;            // mean [cap][8]
    // lists (slots) and per-position scratch
    int *tl, *ll, *tl2, *ll2, *pool, *unc, *rows, *lostn, *newd, *fre, *mrow, *mrow1, *flag;
    // detections of the frame
    float *tlwh, *xywh, *dconf;
    int *dcls, *dhas, *hi, *lo, *cols, *mcol, *hm;
    int* wcnt;                      // [NW + 8]; [NW + 1] read-offs, [NW + 2] LSAPs, [NW + 3] error, [NW + 4] largest side, [NW + 5] appearance pairs
    float* arena;
    int arena_floats;
};

__device__ __forceinline__ BsLds bs_carve(char* base, int total_bytes) {
    BsLds L;
    char* p = base;
    auto take = [&](size_t bytes) { char* q = p; p += (bytes + 15) & ~(size_t)15; return q; };
    const size_t M = TRK_DEV_NMAX;
    static_assert(TRK_DEV_NMAX == TRK_DEV_TMAX, "one side for tracks, detections and LSAP");
    L.u = (double*)take(8 * M); L.v = (double*)take(8 * M); L.dist = (double*)take(8 * M);
    // one statement per field: a table of pointers-to-fields walked in a loop lands in scratch
#define BS_TAKE(f) L.f = (int*)take(4 * M)
    BS_TAKE(pred); BS_TAKE(rowof); BS_TAKE(colof); BS_TAKE(todo); BS_TAKE(pos); BS_TAKE(asg);
    BS_TAKE(id); BS_TAKE(state); BS_TAKE(act); BS_TAKE(start); BS_TAKE(end); BS_TAKE(cls); BS_TAKE(hasf);
    BS_TAKE(tl); BS_TAKE(ll); BS_TAKE(tl2); BS_TAKE(ll2); BS_TAKE(pool); BS_TAKE(unc); BS_TAKE(rows); BS_TAKE(lostn); BS_TAKE(newd);
    BS_TAKE(fre); BS_TAKE(mrow); BS_TAKE(mrow1); BS_TAKE(flag); BS_TAKE(dcls); BS_TAKE(dhas); BS_TAKE(hi); BS_TAKE(lo); BS_TAKE(cols);
    BS_TAKE(mcol); BS_TAKE(hm);
#undef BS_TAKE
    L.score = (float*)take(4 * M);
    L.mean = (float*)take(32 * M);
    L.tlwh = (float*)take(16 * M); L.xywh = (float*)take(16 * M); L.dconf = (float*)take(4 * M);
    L.wcnt = (int*)take(4 * (NW + 8));
    L.arena = (float*)p;
    L.arena_floats = (int)((total_bytes - (p - base)) / 4);
    return L;
}

// track box: [cx - w / 2, cy - h / 2, w, h]
__device__ __forceinline__ void mean_box(const float* m, float b[4]) {
    b[0] = m[0] - m[2] / 2.0f, b[1] = m[1] - m[3] / 2.0f, b[2] = m[2], b[3] = m[3];
}
// 1 - IoU of box b against candidate c (tlwh), union floored at 1e-7, fp32
__device__ __forceinline__ float iou_dist(const float b[4], const float* c) {
    const float brx = b[0] + b[2], bry = b[1] + b[3];
    const float crx = c[0] + c[2], cry = c[1] + c[3];
    const float iw = fmaxf(0.f, fminf(brx, crx) - fmaxf(b[0], c[0]));
    const float ih = fmaxf(0.f, fminf(bry, cry) - fmaxf(b[1], c[1]));
    const float inter = iw * ih;
    const float uni = b[2] * b[3] + c[2] * c[3] - inter;
    return 1.0f - inter / fmaxf(uni, 1e-7f);
}

// the filter of slot sl through the registers of one wavefront (mean in LDS, covariance in HBM)
template <class F>
__device__ __forceinline__ void kf_slot(const BsLds& L, float* cov, int sl, int lane, F f) {
    float p = cov[(size_t)sl * 64 + lane], m = L.mean[sl * 8 + (lane >> 3)];
    f(p, m);
    cov[(size_t)sl * 64 + lane] = p;
    if ((lane & 7) == 0) L.mean[sl * 8 + (lane >> 3)] = m;
}

// pairs of the assignment whose cost is the appearance distance (cost < fused IoU distance)
__device__ __forceinline__ void count_appearance(const BsLds& L, const float* ext, int S, const int* rows, int nr, const int* cols, bool fuse) {
    const int tid = threadIdx.x;
    if (tid < nr && L.mrow[tid] >= 0) {
        const int c = L.mrow[tid], j = cols[c];
        float b[4];
        mean_box(L.mean + rows[tid] * 8, b);
        float x = iou_dist(b, L.tlwh + j * 4);
        if (fuse) x = 1.0f - (1.0f - x) * L.dconf[j];
        if (ext[tid * S + c] < x) atomicAdd(&L.wcnt[NW + 5], 1);
    }
}

// linear_assignment(cost, thresh) of matching.py for rows (slots) x cols (detections), block-wide; reid: cost = min(d_iou, gated d_emb).
// Out: L.mrow[r] = column of row r or -1, L.mcol[c] = row of column c or -1.  *err = 3 when the extended side exceeds the LSAPs.
// Ls: the same carve in LDS, what the (noinline) LSAPs get a reference to -- a reference to the kernel's own copy would put it in scratch.
// smooth / hbm: the block's own smoothed features and HBM scratch.
__device__ void bs_assign(const BsLds& L, const BsLds& Ls, const BsArgs& a, const float* smooth, float* hbm, const int* rows, int nr,
                          const int* cols, int nc, int d0, bool fuse, bool reid, float th, int* err, long long* cyc) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
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
    if (reid) {
        const long long t_cost = threadIdx.x == 0 ? clock64() : 0;
        // The appearance term, for the pairs that pass the proximity veto (taken on the IoU distance before score fusion) and have a feature on
        // both sides: a wavefront takes 64 pairs, finds the ones that need a dot product and walks them, 16-byte loads straight from HBM / L2.
        const int dim = a.prm.dim;
        for (int base = wv * 64; base < nr * nc; base += NW * 64) {
            const int q = base + lane;
            bool need = false;
            int r = 0, c = 0;
            if (q < nr * nc) {
                r = q / nc, c = q - r * nc;
                const int j = cols[c];
                if (L.hasf[rows[r]] && L.dhas[j]) {
                    float b[4];
                    mean_box(L.mean + rows[r] * 8, b);
                    need = !(iou_dist(b, L.tlwh + j * 4) > a.prm.proximity);
                }
            }
            unsigned long long todo = __ballot(need);
            float mine = 0.f;
            while (todo) {
                const int bit = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int q2 = base + bit, r2 = q2 / nc, c2 = q2 - r2 * nc;
                const float d = wave_dot(smooth + (size_t)rows[r2] * dim, a.dets.feat_n + (size_t)(d0 + cols[c2]) * dim, dim, lane);
                if (lane == bit) mine = d;
            }
            if (need) {
                const float e = fmaxf(0.f, 1.0f - mine) / 2.0f;
                if (e <= a.prm.appearance) ext[r * S + c] = fminf(ext[r * S + c], e);
            }
        }
        __threadfence_block();
        __syncthreads();
        if (threadIdx.x == 0) *cyc += clock64() - t_cost;         // the pass as the block sees it: thread 0's share and its wait at the barrier
    }
    if (!a.prm.no_fast) {
        // Unique optimum read off the costs (see kernels_bytetrack.hip): if every row and every column holds at most one entry below thresh
        // and no entry equals it, those entries are the ONLY optimum of the extended problem.
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
            if (reid) count_appearance(L, ext, S, rows, nr, cols, fuse);
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
    if (reid) count_appearance(L, ext, S, rows, nr, cols, fuse);
    __syncthreads();
}

// Kalman update and feature update of the matched rows: one wavefront per row
__device__ __forceinline__ void bs_commit(const BsLds& L, const BsArgs& a, const BsTable& tbl, const int* rows, int nr, const int* cols, int d0,
                                          bool feats) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int r = wv; r < nr; r += NW) {
        const int c = L.mrow[r];
        if (c < 0) continue;
        const int sl = rows[r], j = cols[c];
        kf_slot(L, tbl.cov, sl, lane, [&](float& p, float& m) { kf8_update_wave(p, m, L.xywh + j * 4, lane); });
        if (feats && L.dhas[j])
            feat_update_wave(tbl.feat + (size_t)sl * a.prm.dim, a.dets.feat_n + (size_t)(d0 + j) * a.prm.dim, a.prm.dim, !L.hasf[sl],
                             a.prm.alpha, a.prm.one_minus_alpha, lane);
    }
    __threadfence_block();
    __syncthreads();
    if (feats && threadIdx.x < nr && L.mrow[threadIdx.x] >= 0 && L.dhas[cols[L.mrow[threadIdx.x]]]) L.hasf[rows[threadIdx.x]] = 1;
    __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(TRK_DEV_TMAX) void botsort_epoch_kernel(BsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ BsLds s_lds;
    __shared__ long long s_cyc;
    const long long t_all = clock64();
    const BsLds L = bs_carve(smem, a.lds_bytes);
    if (threadIdx.x == 0) s_lds = L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const BsParams& P = a.prm;
    const int cap = P.cap, dim = P.dim;
    const bool reid = P.reid && a.dets.feat_n != nullptr;
    int* err = L.wcnt + NW + 3;
    // ---- this block's stream: frame range, table, smoothed features, HBM scratch
    const int sid = blockIdx.x;
    const int row0 = a.stream_f0 ? a.stream_f0[sid] : 0;
    const int kend = a.stream_k ? min(a.f0 + a.k, a.stream_k[sid]) : a.f0 + a.k;
    if (a.f0 >= kend) return;                                     // nothing for this stream in this epoch: its table is not touched
    const BsTable tbl = bs_table(a.bank + (size_t)sid * a.table_stride, cap, a.smooth + (size_t)sid * a.smooth_stride);
    float* hbm = a.ext + (size_t)sid * TRK_DEV_NMAX * TRK_DEV_NMAX;
    if (tbl.hdr->err) return;                                     // an earlier epoch of the call failed: the table is not a frame boundary

    // ---- load the table
    int ntl = tbl.hdr->n_tracked, nll = tbl.hdr->n_lost, next_id = tbl.hdr->next_id, frame = tbl.hdr->frame_id;
    if (tid < cap) {
        const BtTrack t = tbl.trk[tid];
        L.id[tid] = t.id, L.state[tid] = t.state, L.act[tid] = t.act, L.start[tid] = t.start, L.end[tid] = t.end, L.cls[tid] = t.cls;
        L.score[tid] = t.score;
        L.hasf[tid] = tbl.hasf[tid];
    }
    for (int e = tid; e < cap * 8; e += BT) L.mean[e] = tbl.mean[e];
    if (tid < ntl) L.tl[tid] = tbl.tl[tid];
    if (tid < nll) L.ll[tid] = tbl.ll[tid];
    if (tid == 0) { s_cyc = 0; *err = 0; L.wcnt[NW + 1] = 0; L.wcnt[NW + 2] = 0; L.wcnt[NW + 4] = tbl.hdr->max_side; L.wcnt[NW + 5] = 0; }
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
            L.xywh[tid * 4 + 0] = x + w / 2.0f, L.xywh[tid * 4 + 1] = y + h / 2.0f, L.xywh[tid * 4 + 2] = w, L.xywh[tid * 4 + 3] = h;
            L.dconf[tid] = a.dets.conf[d0 + tid];
            L.dcls[tid] = a.dets.cls[d0 + tid];
            L.dhas[tid] = reid && (a.dets.valid == nullptr || a.dets.valid[d0 + tid] != 0);
        }
        const float s = tid < n ? a.dets.conf[d0 + tid] : 0.f;
        const int nh = block_compact(tid < n && s > P.high, tid, L.hi, L.wcnt);
        const int nlo = block_compact(tid < n && s > P.low && s < P.high, tid, L.lo, L.wcnt);
        // ---- unconfirmed / tracked / pool = joint(tracked, lost)
        const int tsl = tid < ntl ? L.tl[tid] : 0;
        const int ntk = block_compact(tid < ntl && L.act[tsl], tsl, L.pool, L.wcnt);
        const int nun = block_compact(tid < ntl && !L.act[tsl], tsl, L.unc, L.wcnt);
        if (tid < nll) L.pool[ntk + tid] = L.ll[tid];
        const int np = ntk + nll;
        __syncthreads();
        if (tid < np && L.state[L.pool[tid]] != BT_TRACKED) L.mean[L.pool[tid] * 8 + 6] = 0.f, L.mean[L.pool[tid] * 8 + 7] = 0.f;
        __syncthreads();
        const float* wp = a.warps ? a.warps + (size_t)f * 6 : nullptr;
        for (int r = wv; r < np; r += NW)
            kf_slot(L, cov, L.pool[r], lane, [&](float& p, float& m) {
                kf8_predict_wave(p, m, lane);
                if (wp) kf8_warp_wave(p, m, wp, lane);
            });
        if (wp)
            for (int r = wv; r < nun; r += NW) kf_slot(L, cov, L.unc[r], lane, [&](float& p, float& m) { kf8_warp_wave(p, m, wp, lane); });
        __threadfence_block();
        __syncthreads();

        // ---- stage 1: pool x high band
        bs_assign(L, s_lds, a, tbl.feat, hbm, L.pool, np, L.hi, nh, d0, P.fuse != 0, reid, P.match_thresh, err, &s_cyc);
        if (*err) break;
        bs_commit(L, a, tbl, L.pool, np, L.hi, d0, reid);
        const int nr2 = block_compact(tid < np && L.mrow[tid] < 0 && L.state[L.pool[tid]] == BT_TRACKED, tid < np ? L.pool[tid] : 0, L.rows, L.wcnt);
        if (tid < nh) L.hm[tid] = L.mcol[tid] >= 0;
        if (tid < np && L.mrow[tid] >= 0) {                       // update (Tracked) / re_activate (Lost -> refound)
            const int sl = L.pool[tid], j = L.hi[L.mrow[tid]];
            L.state[sl] = BT_TRACKED, L.act[sl] = 1, L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j];
        }
        __syncthreads();

        // ---- stage 2: the pool's unmatched Tracked tracks x low band, IoU distance, no fusion, no features
        bs_assign(L, s_lds, a, tbl.feat, hbm, L.rows, nr2, L.lo, nlo, d0, false, false, P.second_thresh, err, &s_cyc);
        if (*err) break;
        bs_commit(L, a, tbl, L.rows, nr2, L.lo, d0, false);
        if (tid < nr2) {
            const int sl = L.rows[tid], c = L.mrow[tid];
            if (c >= 0) {
                const int j = L.lo[c];
                L.end[sl] = frame, L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j], L.act[sl] = 1;
            } else L.state[sl] = BT_LOST;                          // mark_lost
        }
        const int nlost = block_compact(tid < nr2 && L.mrow[tid] < 0, tid < nr2 ? L.rows[tid] : 0, L.lostn, L.wcnt);

        // ---- stage 3: unconfirmed x the high band left over, the fused cost, 0.7
        const int nh3 = block_compact(tid < nh && !L.hm[tid], tid < nh ? L.hi[tid] : 0, L.cols, L.wcnt);
        bs_assign(L, s_lds, a, tbl.feat, hbm, L.unc, nun, L.cols, nh3, d0, P.fuse != 0, reid, P.unconf_thresh, err, &s_cyc);
        if (*err) break;
        bs_commit(L, a, tbl, L.unc, nun, L.cols, d0, reid);
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
                                       tid < nh3 ? L.cols[tid] : 0, L.newd, L.wcnt);
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
            L.score[sl] = L.dconf[j], L.cls[sl] = L.dcls[j], L.hasf[sl] = L.dhas[j];
            L.tl2[c1 + tid] = sl;
        }
        for (int r = wv; r < nnew; r += NW) {
            const int sl = L.fre[r], j = L.newd[r];
            kf_slot(L, cov, sl, lane, [&](float& p, float& m) { kf8_initiate_wave(p, m, L.xywh + j * 4, lane); });
            if (L.dhas[j]) feat_update_wave(tbl.feat + (size_t)sl * dim, a.dets.feat_n + (size_t)(d0 + j) * dim, dim, true, 0.f, 0.f, lane);
        }
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

        // ---- outputs: every track of the tracked list, list order
        if (tid == 0) a.out.n_tracks[f] = ntl;
        if (tid < ntl && tid < a.out.max_rows) {
            const int sl = L.tl[tid];
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
            tbl.hasf[tid] = L.hasf[tid];
        }
        for (int i = tid; i < cap * 8; i += BT) tbl.mean[i] = L.mean[i];
        if (tid < ntl) tbl.tl[tid] = L.tl[tid];
        if (tid < nll) tbl.ll[tid] = L.ll[tid];
    }
    if (tid == 0) {
        BsHdr* h = tbl.hdr;
        if (e == 0) h->n_tracked = ntl, h->n_lost = nll, h->next_id = next_id, h->frame_id = frame;
        else h->err = e, h->err_frame = fi;
        h->n_fast += L.wcnt[NW + 1], h->n_lsap += L.wcnt[NW + 2], h->max_side = L.wcnt[NW + 4], h->n_app += L.wcnt[NW + 5];
        h->cyc_cost += s_cyc, h->cyc_all += clock64() - t_all;
    }
}

// out[r] = in[r] / |in[r]|: one wavefront per row, four rows per block
__global__ __launch_bounds__(256) void botsort_normalize_kernel(const float* in, float* out, int rows, int dim) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float* x = in + (size_t)r * dim;
    const float nrm = sqrtf(wave_dot(x, x, dim, lane));
    for (int e = lane * 4; e < dim; e += 256) {
        float4 v = *reinterpret_cast<const float4*>(x + e);
        v.x = v.x / nrm, v.y = v.y / nrm, v.z = v.z / nrm, v.w = v.w / nrm;
        *reinterpret_cast<float4*>(out + (size_t)r * dim + e) = v;
    }
}

static int bs_lds_bytes() { return 159 * 1024; }

void launch_botsort_epoch(char* bank, size_t table_stride, float* smooth, size_t smooth_stride, int streams, const BsParams& prm,
                          const EpochDets& dets, const float* warps, int f0, int k, const int* stream_f0, const int* stream_k, int frame_stride,
                          float* ext, const EpochOut& out, hipStream_t s) {
    set_lds_limit(botsort_epoch_kernel, bs_lds_bytes());
    BsArgs a{bank, table_stride, smooth, smooth_stride, prm, dets, warps, f0, k, stream_f0, stream_k, frame_stride, ext, out, bs_lds_bytes()};
    // one block per stream; 512 threads (__launch_bounds__) and 159 KB of dynamic LDS keep it at one block per CU
    hipLaunchKernelGGL(botsort_epoch_kernel, dim3(streams), dim3(TRK_DEV_TMAX), bs_lds_bytes(), s, a);
    KCHECK();
}

void launch_botsort_normalize(const float* in, float* out, int rows, int dim, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(botsort_normalize_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, in, out, rows, dim);
    KCHECK();
}

}  // namespace aic
