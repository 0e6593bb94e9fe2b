// kernels_ocsort.hip -- OC-SORT on the device, k frames per launch (structures: ocsort.hpp).
//
// Specification: OCSort.update() of the OC-SORT authors as restated in tests/ocsort_oracle.py, with the deliberate changes listed there
// (this project's IoU, the fp32 7-state filter in a stated operation order, per-tracker ids, SciPy's tie rules on the rectangular problem,
// a fixed fp32 asin, ascending unmatched lists, non-finite predictions dropped).  The filter arithmetic is kf7_math.hpp's, the LSAPs, the
// DPP reductions and the ordered compaction are trk_wave.hpp's (shared with the DeepSORT and ByteTrack epoch kernels).
//
// ONE block of 512 threads walks the frames of one stream: thread i <-> list position i / detection i / slot i.  Per frame:
//   bands (high: s > det_thresh; with use_byte the low band 0.1 < s < det_thresh) -> predict every track (one wavefront per track), drop a
//   track whose box is not finite, look up the observation delta_t ages back -> stage 1: high band x tracks on -(IoU + OCM term), IoU and
//   term in one pass that also counts the entries above the threshold per row and column (upstream's read-off, else the LSAP) -> BYTE
//   stage (low band x unmatched tracks, IoU with the prediction) -> OCR stage (unmatched high band x unmatched tracks, IoU with the LAST
//   OBSERVATION) -> one update pass: a matched track takes its detection (a frozen filter first goes back to its frozen state and replays
//   the virtual trajectory, ORU; the wavefront that owns the track walks it, no block barrier inside), an unmatched observed filter is
//   frozen -> new tracks -> output rows (the list reversed, as upstream) -> removal at time_since_update > max_age.
// Assignment problems are rectangular, detections x tracks as upstream; a real pair must also have IoU >= the threshold.
#include "kernels.hpp"
#include "trk_dev.hpp"
#include "kf7_math.hpp"
#include "trk_wave.hpp"
#include "ocsort.hpp"

namespace aic {

struct OcArgs {
    EpochCall c;                    // stream s: oc_table(c.bank + s * c.table_stride, cap); c.ext: cost matrices beyond the LDS arena
    OcParams prm;
    int lds_bytes;
};

namespace {

enum { OC_STAGE1 = 0, OC_BYTE = 1, OC_OCR = 2 };
// L.wcnt[NW + ...]
enum { W_FAST = 1, W_LSAP = 2, W_ERR = 3, W_SIDE = 4, W_ANY = 5, W_ORU = 6, W_GAP = 7, W_OCR = 8, W_BYTE = 9, W_N = 10 };

struct OcLds {
    // LSAP (trk_wave.hpp), side <= 512
    double *u, *v, *dist;
    int *pred, *rowof, *colof, *todo, *pos, *asg;
    // track table by slot
    int *id, *age, *hits, *streak, *tsu, *cls, *kst, *hobs, *hvel;
    float *score, *last, *vel, *mean, *pbox, *prev;               // last / pbox / prev [cap][4], vel [cap][2], mean [cap][8]
    // lists and per-position scratch
    int *tl, *tl2, *hi, *lo, *ud, *ut, *mrow, *tdet, *fre, *newd, *flag, *dfree, *outl;
    // detections of the frame
    float *dbox, *dconf;
    int* dcls;
    int* wcnt;                      // [NW + W_N]
    float* arena;
    int arena_floats;
};

__device__ __forceinline__ OcLds oc_carve(char* base, int total_bytes) {
    OcLds L;
    char* p = base;
    auto take = [&](size_t bytes) { char* q = p; p += (bytes + 15) & ~(size_t)15; return q; };
    const size_t M = TRK_DEV_NMAX;
    static_assert(TRK_DEV_NMAX == TRK_DEV_TMAX, "one side for tracks, detections and LSAP");
    L.u = (double*)take(8 * M); L.v = (double*)take(8 * M); L.dist = (double*)take(8 * M);
    // one statement per field: a table of pointers-to-fields walked in a loop lands in scratch
#define OC_TAKE(f) L.f = (int*)take(4 * M)
    OC_TAKE(pred); OC_TAKE(rowof); OC_TAKE(colof); OC_TAKE(todo); OC_TAKE(pos); OC_TAKE(asg);
    OC_TAKE(id); OC_TAKE(age); OC_TAKE(hits); OC_TAKE(streak); OC_TAKE(tsu); OC_TAKE(cls); OC_TAKE(kst); OC_TAKE(hobs); OC_TAKE(hvel);
    OC_TAKE(tl); OC_TAKE(tl2); OC_TAKE(hi); OC_TAKE(lo); OC_TAKE(ud); OC_TAKE(ut); OC_TAKE(mrow); OC_TAKE(tdet); OC_TAKE(fre); OC_TAKE(newd);
    OC_TAKE(flag); OC_TAKE(dfree); OC_TAKE(outl); OC_TAKE(dcls);
#undef OC_TAKE
    L.score = (float*)take(4 * M);
    L.last = (float*)take(16 * M); L.vel = (float*)take(8 * M); L.mean = (float*)take(32 * M);
    L.pbox = (float*)take(16 * M); L.prev = (float*)take(16 * M);
    L.dbox = (float*)take(16 * M); L.dconf = (float*)take(4 * M);
    L.wcnt = (int*)take(4 * (NW + W_N));
    L.arena = (float*)p;
    L.arena_floats = (int)((total_bytes - (p - base)) / 4);
    return L;
}
constexpr size_t OC_FIXED_LDS_BYTES = (3 * 8 + 6 * 4) * (size_t)TRK_DEV_NMAX + (size_t)TRK_DEV_NMAX * (23 * 4 + 4 + 16 + 8 + 32 + 16 + 16 + 16 + 4) + ((4 * (NW + W_N) + 15) & ~15);
static_assert((159 * 1024 - OC_FIXED_LDS_BYTES) / 4 == 8428, "the LDS arena of the OC-SORT kernel");

// One association problem, block-wide: rows = detections `rows[0..nr)`, columns = list positions `cols[0..nc)`.
//   OC_STAGE1: cost -(IoU(det, prediction) + OCM term); upstream's read-off when every row and column has at most one IoU above the threshold
//              (and there is one), else the LSAP.
//   OC_BYTE:   cost -IoU(det, prediction);   OC_OCR: cost -IoU(det, last observation); both solved only if some IoU exceeds the threshold.
// A pair stands if its IoU is not below the threshold.  Out: L.mrow[r] = column index or -1.  Returns through *err (2: no finite solution).
// Ls: the same carve in LDS, what the (noinline) LSAPs get a reference to -- a reference to the kernel's own copy would put it in scratch.
__device__ void oc_assign(const OcLds& L, const OcLds& Ls, const OcArgs& a, float* hbm, const int* rows, int nr, const int* cols, int nc, int mode, int* err) {
    const int tid = threadIdx.x;
    const float th = a.prm.iou_thresh;
    int* rcnt = L.pred; int* rarg = L.colof; int* ccnt = L.rowof;  // free until the LSAP starts
    if (tid < nr) { L.mrow[tid] = -1; rcnt[tid] = 0; rarg[tid] = -1; }
    if (tid < nc) ccnt[tid] = 0;
    if (tid == 0) L.wcnt[NW + W_ANY] = 0;
    __syncthreads();
    if (nr == 0 || nc == 0) return;
    float* cm = nr * nc <= L.arena_floats ? L.arena : hbm;
    const float* tbox = mode == OC_OCR ? L.last : L.pbox;
    for (int e = tid; e < nr * nc; e += BT) {
        const int r = e / nc, c = e - r * nc;
        const int j = rows[r], sl = L.tl[cols[c]];
        const float* d = L.dbox + j * 4;
        const float iou = iou_xyxy(d, tbox + sl * 4);
        float x = iou;
        if (mode == OC_STAGE1) {
            // OCM: inertia * valid * asin(clip(vel . dir(previous observation -> detection))) / pi * score
            float t = 0.f;
            if (L.hobs[sl]) {
                const float* q = L.prev + sl * 4;
                const float dx = (d[0] + d[2]) / 2.0f - (q[0] + q[2]) / 2.0f;
                const float dy = (d[1] + d[3]) / 2.0f - (q[1] + q[3]) / 2.0f;
                const float norm = sqrtf(dx * dx + dy * dy) + 1e-6f;
                float cs = L.vel[sl * 2 + 1] * (dx / norm) + L.vel[sl * 2 + 0] * (dy / norm);
                cs = fminf(fmaxf(cs, -1.0f), 1.0f);
                t = ((asin32(cs) / 3.141592653589793f) * a.prm.inertia) * L.dconf[j];
            }
            x = iou + t;
        }
        cm[e] = -x;
        if (iou > th) {
            L.wcnt[NW + W_ANY] = 1;
            if (mode == OC_STAGE1) { atomicAdd(&rcnt[r], 1); atomicAdd(&ccnt[c], 1); rarg[r] = c; }
        }
    }
    __threadfence_block();
    __syncthreads();
    const bool any = L.wcnt[NW + W_ANY] != 0;
    if (mode != OC_STAGE1 && !any) return;                        // ocsort.py: iou_left.max() > iou_threshold
    if (mode == OC_STAGE1 && !a.prm.no_fast) {
        const bool ok = any && (tid >= nr || rcnt[tid] <= 1) && (tid >= nc || ccnt[tid] <= 1);
        if (__syncthreads_and(ok)) {                              // association.py: a.sum(1).max() == 1 and a.sum(0).max() == 1
            if (tid < nr && rcnt[tid] == 1) L.mrow[tid] = rarg[tid];
            if (tid == 0) L.wcnt[NW + W_FAST] += 1;
            __syncthreads();
            return;
        }
    }
    if (tid == 0) { L.wcnt[NW + W_LSAP] += 1; L.wcnt[NW + W_SIDE] = max(L.wcnt[NW + W_SIDE], max(nr, nc)); }
    if (tid < 64) {
        const int S = max(nr, nc);
        const bool ok = S <= 64 ? lsap_wave64(cm, nr, nc, Ls, tid) : S <= 128 ? lsap_wave_reg<2>(cm, nr, nc, Ls, tid) : lsap_wave(cm, nr, nc, Ls, tid);
        if (!ok && tid == 0) *err = 2;
    }
    __syncthreads();
    if (tid < nr) {
        const int c = L.asg[tid];
        if (c >= 0 && c < nc) {
            const float iou = iou_xyxy(L.dbox + rows[tid] * 4, tbox + L.tl[cols[c]] * 4);
            if (!(iou < th)) L.mrow[tid] = c;
        }
    }
    __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(TRK_DEV_TMAX) void ocsort_epoch_kernel(OcArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ OcLds s_lds;
    const OcLds L = oc_carve(smem, a.lds_bytes);
    if (threadIdx.x == 0) s_lds = L;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int li = lane >> 3, lj = lane & 7;
    const OcParams& P = a.prm;
    const int cap = P.cap, DT = P.delta_t;
    int* err = L.wcnt + NW + W_ERR;
    // ---- this block's stream: frame range, table, HBM scratch
    const int sid = blockIdx.x;
    const EpochCall& c = a.c;
    const int row0 = c.stream_f0 ? c.stream_f0[sid] : 0;
    const int kend = c.stream_k ? min(c.f0 + c.k, c.stream_k[sid]) : c.f0 + c.k;
    if (c.f0 >= kend) return;                                     // nothing for this stream in this epoch: its table is not touched
    const OcTable tbl = oc_table(c.bank + (size_t)sid * c.table_stride, cap);
    float* hbm = c.ext + (size_t)sid * TRK_DEV_NMAX * TRK_DEV_TMAX;
    if (tbl.hdr->err) return;                                   // an earlier epoch of the call failed: the table is not a frame boundary

    // ---- load the table
    int nt = tbl.hdr->n_tracks, next_id = tbl.hdr->next_id, frame = tbl.hdr->frame;
    if (tid < cap) {
        const OcTrack t = tbl.trk[tid];
        L.id[tid] = t.id, L.age[tid] = t.age, L.hits[tid] = t.hits, L.streak[tid] = t.streak, L.tsu[tid] = t.tsu, L.cls[tid] = t.cls;
        L.kst[tid] = t.kstate, L.hobs[tid] = t.has_obs, L.hvel[tid] = t.has_vel, L.score[tid] = t.score;
#pragma unroll
        for (int q = 0; q < 4; ++q) L.last[tid * 4 + q] = t.last[q];
        L.vel[tid * 2] = t.vel[0], L.vel[tid * 2 + 1] = t.vel[1];
    }
    for (int e = tid; e < cap * 8; e += BT) L.mean[e] = tbl.mean[e];
    if (tid < nt) L.tl[tid] = tbl.tl[tid];
    if (tid < W_N) L.wcnt[NW + tid] = 0;
    __syncthreads();
    if (tid == 0) L.wcnt[NW + W_SIDE] = tbl.hdr->max_side, L.wcnt[NW + W_GAP] = tbl.hdr->max_gap;
    __syncthreads();
    float* cov = tbl.cov;
    int fi = c.f0;
    for (; fi < kend; ++fi) {
        const int f = row0 + fi * c.frame_stride;
        ++frame;
        const int n = c.dets.frame_n[f], d0 = c.dets.frame_d0[f];
        if (n > TRK_DEV_NMAX) { if (tid == 0) *err = 3; break; }
        float s = 0.f;
        if (tid < n) {
            const float* b = c.dets.tlwh + (size_t)(d0 + tid) * 4;
            const float x = b[0], y = b[1], w = b[2], h = b[3];
            L.dbox[tid * 4 + 0] = x, L.dbox[tid * 4 + 1] = y, L.dbox[tid * 4 + 2] = x + w, L.dbox[tid * 4 + 3] = y + h;
            s = c.dets.conf[d0 + tid];
            L.dconf[tid] = s;
            L.dcls[tid] = c.dets.cls[d0 + tid];
        }
        L.dfree[tid] = 1;
        const int nh = block_compact(tid < n && s > P.det_thresh, tid, L.hi, L.wcnt);
        const int nlo = block_compact(P.use_byte && tid < n && s > P.low_thresh && s < P.det_thresh, tid, L.lo, L.wcnt);

        // ---- predict (KalmanBoxTracker.predict): one wavefront per track, covariance through registers
        for (int r = wv; r < nt; r += NW) {
            const int sl = L.tl[r];
            float p = cov[(size_t)sl * 64 + lane], m = L.mean[sl * 8 + li];
            if (L.mean[sl * 8 + 6] + L.mean[sl * 8 + 2] <= 0.f && li == 6) m = 0.f;
            wave_lds_sync();
            kf7_predict_wave(p, m, lane);
            cov[(size_t)sl * 64 + lane] = p;
            if (lj == 0) L.mean[sl * 8 + li] = m;
        }
        __threadfence_block();
        __syncthreads();
        bool keep = false;
        const int psl = tid < nt ? L.tl[tid] : 0;
        if (tid < nt) {
            const int sl = psl;
            const int age = L.age[sl] + 1;
            L.age[sl] = age;
            if (L.tsu[sl] > 0) L.streak[sl] = 0;
            L.tsu[sl] += 1;
            float b[4];
            x_to_bbox(L.mean[sl * 8 + 0], L.mean[sl * 8 + 1], L.mean[sl * 8 + 2], L.mean[sl * 8 + 3], b);
#pragma unroll
            for (int q = 0; q < 4; ++q) L.pbox[sl * 4 + q] = b[q];
            keep = isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]);
            // k_previous_obs: the observation delta_t ages back, else the nearest younger one, else the last observation
            float q4[4] = {L.last[sl * 4], L.last[sl * 4 + 1], L.last[sl * 4 + 2], L.last[sl * 4 + 3]};
            if (L.hobs[sl]) {
                for (int dt = DT; dt >= 1; --dt) {
                    const int key = age - dt;
                    if (key < 1) continue;
                    const int o = sl * OC_DTMAX + key % DT;
                    if (tbl.ring_age[o] == key) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) q4[q] = tbl.ring_box[(size_t)o * 4 + q];
                        break;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) L.prev[sl * 4 + q] = q4[q];
        }
        const int ntk = block_compact(tid < nt && keep, psl, L.tl2, L.wcnt);
        if (tid < ntk) L.tl[tid] = L.tl2[tid];
        nt = ntk;
        L.tdet[tid] = -1;
        L.ut[tid] = tid;
        __syncthreads();

        // ---- stage 1: high band x every track
        oc_assign(L, s_lds, a, hbm, L.hi, nh, L.ut, nt, OC_STAGE1, err);
        if (*err) break;
        if (tid < nh && L.mrow[tid] >= 0) { L.tdet[L.mrow[tid]] = L.hi[tid]; L.dfree[L.hi[tid]] = 0; }
        __syncthreads();

        // ---- BYTE stage: low band x unmatched tracks, IoU with the prediction
        if (nlo > 0) {
            const int nut = block_compact(tid < nt && L.tdet[tid] < 0, tid, L.ut, L.wcnt);
            oc_assign(L, s_lds, a, hbm, L.lo, nlo, L.ut, nut, OC_BYTE, err);
            if (*err) break;
            if (tid < nlo && nut > 0 && L.mrow[tid] >= 0) { L.tdet[L.ut[L.mrow[tid]]] = L.lo[tid]; atomicAdd(&L.wcnt[NW + W_BYTE], 1); }
            __syncthreads();
        }
        // ---- OCR stage: unmatched high band x unmatched tracks, IoU with the last observation
        {
            const int hj = tid < nh ? L.hi[tid] : 0;
            const int nud = block_compact(tid < nh && L.dfree[hj], hj, L.ud, L.wcnt);
            const int nut = block_compact(tid < nt && L.tdet[tid] < 0, tid, L.ut, L.wcnt);
            oc_assign(L, s_lds, a, hbm, L.ud, nud, L.ut, nut, OC_OCR, err);
            if (*err) break;
            if (tid < nud && nut > 0 && L.mrow[tid] >= 0) {
                L.tdet[L.ut[L.mrow[tid]]] = L.ud[tid];
                L.dfree[L.ud[tid]] = 0;
                atomicAdd(&L.wcnt[NW + W_OCR], 1);
            }
            __syncthreads();
        }

        // ---- update pass, filters: KalmanFilterNew.update(z) / update(None)
        for (int r = wv; r < nt; r += NW) {
            const int sl = L.tl[r], d = L.tdet[r], ks = L.kst[sl];
            if (d < 0) {
                if (ks == KF7_OBSERVED) {                         // freeze: the filter as predicted into the first missed frame
                    tbl.fcov[(size_t)sl * 64 + lane] = cov[(size_t)sl * 64 + lane];
                    if (lj == 0) tbl.fmean[sl * 8 + li] = L.mean[sl * 8 + li];
                }
                continue;
            }
            const float* nb = L.dbox + d * 4;
            float z2[4];
            bbox_to_z(nb, z2);
            float p, m;
            if (ks == KF7_FROZEN) {
                // ORU (unfreeze): back to the frozen filter, `gap` virtual observations on the straight line, in (x, y, w, h), from the last
                // observation to the new one; update, then predict except after the last.  gap <= max_age + 1.
                p = tbl.fcov[(size_t)sl * 64 + lane], m = tbl.fmean[sl * 8 + li];
                const int gap = min(L.tsu[sl], P.max_age + 1);
                float z1[4];
                bbox_to_z(L.last + sl * 4, z1);
                const float w1 = sqrtf(z1[2] * z1[3]), h1 = sqrtf(z1[2] / z1[3]);
                const float w2 = sqrtf(z2[2] * z2[3]), h2 = sqrtf(z2[2] / z2[3]);
                const float g = (float)gap;
                const float dx = (z2[0] - z1[0]) / g, dy = (z2[1] - z1[1]) / g, dw = (w2 - w1) / g, dh = (h2 - h1) / g;
                for (int i = 0; i < gap; ++i) {
                    const float kk = (float)(i + 1);
                    const float w = w1 + kk * dw, h = h1 + kk * dh;
                    const float zv[4] = {z1[0] + kk * dx, z1[1] + kk * dy, w * h, w / h};
                    kf7_update_wave(p, m, zv, lane);
                    if (i != gap - 1) kf7_predict_wave(p, m, lane);
                }
            } else {
                p = cov[(size_t)sl * 64 + lane], m = L.mean[sl * 8 + li];
            }
            kf7_update_wave(p, m, z2, lane);
            wave_lds_sync();
            cov[(size_t)sl * 64 + lane] = p;
            if (lj == 0) L.mean[sl * 8 + li] = m;
        }
        __threadfence_block();
        __syncthreads();
        // ---- update pass, bookkeeping: KalmanBoxTracker.update
        if (tid < nt) {
            const int sl = L.tl[tid], d = L.tdet[tid];
            if (d < 0) {
                if (L.kst[sl] == KF7_OBSERVED) L.kst[sl] = KF7_FROZEN;
            } else {
                const float* nb = L.dbox + d * 4;
                if (L.hobs[sl]) {
                    float v[2];
                    speed_direction(L.prev + sl * 4, nb, v);
                    L.vel[sl * 2] = v[0], L.vel[sl * 2 + 1] = v[1];
                    L.hvel[sl] = 1;
                }
                if (L.kst[sl] == KF7_FROZEN) {
                    atomicAdd(&L.wcnt[NW + W_ORU], 1);
                    atomicMax(&L.wcnt[NW + W_GAP], L.tsu[sl]);
                }
                L.kst[sl] = KF7_OBSERVED;
                const int age = L.age[sl], o = sl * OC_DTMAX + age % DT;
                tbl.ring_age[o] = age;
#pragma unroll
                for (int q = 0; q < 4; ++q) { L.last[sl * 4 + q] = nb[q]; tbl.ring_box[(size_t)o * 4 + q] = nb[q]; }
                L.hobs[sl] = 1, L.tsu[sl] = 0, L.hits[sl] += 1, L.streak[sl] += 1;
                L.score[sl] = L.dconf[d], L.cls[sl] = L.dcls[d];
            }
        }
        // ---- new tracks from the unmatched high band, detection order, on the lowest free slots
        const int hj = tid < nh ? L.hi[tid] : 0;
        const int nnew = block_compact(tid < nh && L.dfree[hj], hj, L.newd, L.wcnt);
        if (tid < cap) L.flag[tid] = 0;
        __syncthreads();
        if (tid < nt) L.flag[L.tl[tid]] = 1;
        __syncthreads();
        const int nfree = block_compact(tid < cap && !L.flag[tid], tid, L.fre, L.wcnt);
        if (nnew > nfree) { if (tid == 0) *err = 1; break; }
        if (tid < nnew) {                                         // KalmanBoxTracker.__init__
            const int sl = L.fre[tid], j = L.newd[tid];
            L.id[sl] = next_id + tid, L.age[sl] = 0, L.hits[sl] = 0, L.streak[sl] = 0, L.tsu[sl] = 0, L.cls[sl] = L.dcls[j];
            L.kst[sl] = KF7_NEW, L.hobs[sl] = 0, L.hvel[sl] = 0, L.score[sl] = L.dconf[j];
            float z[4];
            bbox_to_z(L.dbox + j * 4, z);
#pragma unroll
            for (int q = 0; q < 4; ++q) { L.last[sl * 4 + q] = -1.f; L.mean[sl * 8 + q] = z[q]; L.mean[sl * 8 + 4 + q] = 0.f; }
            L.vel[sl * 2] = 0.f, L.vel[sl * 2 + 1] = 0.f;
            for (int q = 0; q < OC_DTMAX; ++q) tbl.ring_age[sl * OC_DTMAX + q] = -1;
            L.tl[nt + tid] = sl;
        }
        for (int e = tid; e < nnew * 64; e += BT) {
            const int i = (e & 63) >> 3, j = e & 7;
            cov[(size_t)L.fre[e >> 6] * 64 + (e & 63)] = i == j && i < 7 ? kf7_p0(i) : 0.f;
        }
        next_id += nnew;
        nt += nnew;
        __threadfence_block();
        __syncthreads();

        // ---- outputs (the list reversed), then removal at time_since_update > max_age
        const int osl = tid < nt ? L.tl[nt - 1 - tid] : 0;
        const int no = block_compact(tid < nt && L.tsu[osl] < 1 && (L.streak[osl] >= P.min_hits || frame <= P.min_hits), osl, L.outl, L.wcnt);
        if (tid == 0) c.out.n_tracks[f] = no;
        if (tid < no && tid < c.out.max_rows) {
            const int sl = L.outl[tid];
            float b[4];
            if (L.hobs[sl]) { b[0] = L.last[sl * 4], b[1] = L.last[sl * 4 + 1], b[2] = L.last[sl * 4 + 2], b[3] = L.last[sl * 4 + 3]; }
            else x_to_bbox(L.mean[sl * 8 + 0], L.mean[sl * 8 + 1], L.mean[sl * 8 + 2], L.mean[sl * 8 + 3], b);
            int* r = c.out.rows + ((size_t)f * c.out.max_rows + tid) * 6;
            r[0] = (int)rintf(b[0]), r[1] = (int)rintf(b[1]), r[2] = (int)rintf(b[2]), r[3] = (int)rintf(b[3]);   // round half to even
            r[4] = L.id[sl], r[5] = L.cls[sl];
            c.out.conf[(size_t)f * c.out.max_rows + tid] = L.score[sl];
        }
        const int rsl = tid < nt ? L.tl[tid] : 0;
        const int nkeep = block_compact(tid < nt && !(L.tsu[rsl] > P.max_age), rsl, L.tl2, L.wcnt);
        if (tid < nkeep) L.tl[tid] = L.tl2[tid];
        nt = nkeep;
        __syncthreads();
    }
    // ---- write back (on an error the tracker stops: the host refuses further updates)
    __syncthreads();
    const int e = *err;
    if (e == 0) {
        if (tid < cap) {
            OcTrack t;
            t.id = L.id[tid], t.age = L.age[tid], t.hits = L.hits[tid], t.streak = L.streak[tid], t.tsu = L.tsu[tid], t.cls = L.cls[tid];
            t.kstate = L.kst[tid], t.has_obs = L.hobs[tid], t.has_vel = L.hvel[tid], t.score = L.score[tid];
#pragma unroll
            for (int q = 0; q < 4; ++q) t.last[q] = L.last[tid * 4 + q];
            t.vel[0] = L.vel[tid * 2], t.vel[1] = L.vel[tid * 2 + 1];
            tbl.trk[tid] = t;
        }
        for (int i = tid; i < cap * 8; i += BT) tbl.mean[i] = L.mean[i];
        if (tid < nt) tbl.tl[tid] = L.tl[tid];
    }
    if (tid == 0) {
        OcHdr* h = tbl.hdr;
        if (e == 0) h->n_tracks = nt, h->next_id = next_id, h->frame = frame;
        else h->err = e, h->err_frame = fi;
        h->n_fast += L.wcnt[NW + W_FAST], h->n_lsap += L.wcnt[NW + W_LSAP], h->max_side = L.wcnt[NW + W_SIDE];
        h->n_oru += L.wcnt[NW + W_ORU], h->max_gap = L.wcnt[NW + W_GAP], h->n_ocr += L.wcnt[NW + W_OCR], h->n_byte += L.wcnt[NW + W_BYTE];
    }
}

static int oc_lds_bytes() { return 159 * 1024; }

void launch_ocsort_epoch(const OcParams& prm, const EpochCall& c, hipStream_t s) {
    set_lds_limit(ocsort_epoch_kernel, oc_lds_bytes());
    OcArgs a{c, prm, oc_lds_bytes()};
    hipLaunchKernelGGL(ocsort_epoch_kernel, dim3(c.streams), dim3(TRK_DEV_TMAX), oc_lds_bytes(), s, a);
    KCHECK();
}

}  // namespace aic
