// trk_wave.hpp -- block / wavefront building blocks of the one-block tracker epoch kernels (kernels_trk_dev.hip: DeepSORT,
// byte_epoch.hpp: ByteTrack and BoT-SORT, kernels_ocsort.hip: OC-SORT): ordered block compaction, DPP wave reductions and the three
// restatements of SciPy's rectangular LSAP.  The LSAPs are templates over the caller's LDS carve: they read and write only its fields
// u, v, dist (double[side]) and pred, rowof, colof, todo, pos, asg (int[side]): LsapLds below, which the carve of byte_epoch.hpp starts
// with.  The stream prologue of an EpochCall (trk_dev.hpp) and the writer of an output row are here as well; OC-SORT keeps copies of its
// own for now (with the shared ones its kernel compiled differently and two cells of its benchmark slowed).
#pragma once
#include "kernels.hpp"
#include "trk_dev.hpp"

namespace aic {
namespace {

constexpr int BT = TRK_DEV_TMAX;        // threads of the epoch kernel: thread t <-> track t, thread j <-> detection j
constexpr int NW = BT / 64;

__device__ __forceinline__ void wave_lds_sync() {            // LDS traffic of ONE wave: program order + a compiler fence
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ordered (stable) compaction over the block: flagged threads write `value` at list[rank]; returns the count. Two barriers.
__device__ __forceinline__ int block_compact(bool flag, int value, int* list, int* wcnt) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(flag);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int cnt = wcnt[i];
        if (i < w) off += cnt;
        tot += cnt;
    }
    if (flag) list[off + before] = value;
    __syncthreads();
    return tot;
}

// ---- the banked epoch kernels: LDS carve, stream prologue, output row ------------------------------------------------------------
struct LdsTake {                        // the dynamic LDS handed out front to back, 16-byte steps
    char* p;
    __device__ __forceinline__ char* operator()(size_t bytes) { char* q = p; p += (bytes + 15) & ~(size_t)15; return q; }
};

struct LsapLds {                        // what the LSAPs below read and write, side <= TRK_DEV_NMAX
    double *u, *v, *dist;
    int *pred, *rowof, *colof, *todo, *pos, *asg;
};
constexpr size_t LSAP_LDS_BYTES = (3 * 8 + 6 * 4) * (size_t)TRK_DEV_NMAX;

__device__ __forceinline__ void carve_lsap(LsapLds& L, LdsTake& take) {
    const size_t M = TRK_DEV_NMAX;
    static_assert(TRK_DEV_NMAX == TRK_DEV_TMAX, "one side for tracks, detections and LSAP");
    // one statement per field: a table of pointers-to-fields walked in a loop lands in scratch
    L.u = (double*)take(8 * M); L.v = (double*)take(8 * M); L.dist = (double*)take(8 * M);
    L.pred = (int*)take(4 * M); L.rowof = (int*)take(4 * M); L.colof = (int*)take(4 * M);
    L.todo = (int*)take(4 * M); L.pos = (int*)take(4 * M); L.asg = (int*)take(4 * M);
}

struct EpochStream {                    // this block's stream of an EpochCall
    int row0, kend;                     // local frame i = row row0 + i * frame_stride of dets / out; local frames [f0, kend)
    float* ext;                         // the stream's slice of the HBM scratch
};

// False: the block has nothing to do and returns.  table_err: err of the stream's table header.
__device__ __forceinline__ bool epoch_stream(const EpochCall& c, const int32_t* table_err, EpochStream& st) {
    const int sid = blockIdx.x;
    st.row0 = c.stream_f0 ? c.stream_f0[sid] : 0;
    st.kend = c.stream_k ? min(c.f0 + c.k, c.stream_k[sid]) : c.f0 + c.k;
    if (c.f0 >= st.kend) return false;                           // nothing for this stream in this epoch: its table is not touched
    st.ext = c.ext + (size_t)sid * TRK_DEV_NMAX * TRK_DEV_TMAX;
    return *table_err == 0;                                      // an earlier epoch of the call failed: the table is not a frame boundary
}

// output row i (< max_rows) of frame row f: the corners, id, class; and the score
__device__ __forceinline__ void write_row(const EpochOut& o, int f, int i, float x1, float y1, float x2, float y2, int id, int cls, float score) {
    int* r = o.rows + ((size_t)f * o.max_rows + i) * 6;
    r[0] = (int)rintf(x1), r[1] = (int)rintf(y1), r[2] = (int)rintf(x2), r[3] = (int)rintf(y2);   // round half to even
    r[4] = id, r[5] = cls;
    o.conf[(size_t)f * o.max_rows + i] = score;
}

__device__ __forceinline__ int block_min_int(int v, int* wcnt) {     // two barriers
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    if (lane == 0) wcnt[w] = v;
    __syncthreads();
    int m = wcnt[0];
#pragma unroll
    for (int i = 1; i < NW; ++i) m = min(m, wcnt[i]);
    __syncthreads();
    return m;
}

// ---- wave reductions on DPP row shifts (full wave active) -------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ unsigned dpp_keep(unsigned old, unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xf, 0xf, false);
}
__device__ __forceinline__ unsigned wave_umin32(unsigned v) {
    v = min(v, dpp_keep<0x111>(0xffffffffu, v));   // row_shr:1  (lanes without a source keep the identity)
    v = min(v, dpp_keep<0x112>(0xffffffffu, v));   // row_shr:2
    v = min(v, dpp_keep<0x114>(0xffffffffu, v));   // row_shr:4
    v = min(v, dpp_keep<0x118>(0xffffffffu, v));   // row_shr:8  -> lane 15 of every row of 16 holds the row minimum
    const unsigned a = __builtin_amdgcn_readlane((int)v, 15), b = __builtin_amdgcn_readlane((int)v, 31);
    const unsigned c = __builtin_amdgcn_readlane((int)v, 47), d = __builtin_amdgcn_readlane((int)v, 63);
    return min(min(a, b), min(c, d));
}
__device__ __forceinline__ unsigned wave_umax32(unsigned v) { return ~wave_umin32(~v); }
// order-preserving 64-bit key of a double (no NaN here): smaller double <=> smaller unsigned key
__device__ __forceinline__ unsigned long long f64_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_f64(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
__device__ __forceinline__ double wave_min_f64(double x) {
    const unsigned long long k = f64_key(x);
    const unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
    const unsigned mh = wave_umin32(hi);
    const unsigned long long top = __ballot(hi == mh);
    if (__popcll(top) == 1) {                                   // one lane holds the smallest high word: it IS the minimum
        const int l = __ffsll((long long)top) - 1;
        const unsigned ml1 = (unsigned)__builtin_amdgcn_readlane((int)lo, l);
        return key_f64(((unsigned long long)mh << 32) | ml1);
    }
    const unsigned ml = wave_umin32(hi == mh ? lo : 0xffffffffu);
    return key_f64(((unsigned long long)mh << 32) | ml);
}

// Rectangular linear sum assignment of SciPy 1.15.3 (Crouse's shortest augmenting path), restating csrc/lsap.cpp for ONE
// wavefront: the scan over the unscanned columns is spread over the lanes, the three details that decide WHICH optimum comes
// back are kept exactly --
//   (1) unscanned columns live in a list initialised in DESCENDING column order, a scanned column is replaced by the list's
//       last entry (pos[] is the inverse of todo[]);
//   (2) among equal reduced path costs the LAST visited unassigned column wins, otherwise the FIRST visited column
//       (= max list position over the unassigned minima if there is one, else min list position over the minima);
//   (3) dual update and back-tracking along pred[] in the reference's order and fp64 operation order.
// cm: nr x nc fp32 (LDS or global), solved transposed when nr > nc (lsap.cpp:113-123).  Result asg[orig row] = orig column or -1.
// Returns false when no finite completion exists (cannot happen for the clamped matrices of min_cost_matching).
template <class Lds>
__device__ __noinline__ bool lsap_wave(const float* cm, int nr, int nc, const Lds& L, int lane) {
    const bool tall = nr > nc;
    const int R = tall ? nc : nr, C = tall ? nr : nc;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (int j = lane; j < C; j += 64) { L.v[j] = 0.0; L.rowof[j] = -1; }
    for (int i = lane; i < R; i += 64) { L.u[i] = 0.0; L.colof[i] = -1; }
    wave_lds_sync();
    for (int root = 0; root < R; ++root) {
        for (int j = lane; j < C; j += 64) { L.dist[j] = inf; L.todo[j] = C - 1 - j; L.pos[j] = C - 1 - j; }
        wave_lds_sync();
        double base = 0.0;
        int live = C, i = root, sink = -1;
        while (sink < 0) {
            const double ui = L.u[i];
            double lmin = inf;
            for (int j = lane; j < C; j += 64) {
                if (L.pos[j] >= 0) {
                    const float cij = tall ? cm[(size_t)j * nc + i] : cm[(size_t)i * nc + j];
                    const double red = ((base + (double)cij) - ui) - L.v[j];
                    double dj = L.dist[j];
                    if (red < dj) { dj = red; L.dist[j] = red; L.pred[j] = i; }
                    lmin = dj < lmin ? dj : lmin;
                }
            }
            const double m = wave_min_f64(lmin);
            if (!(m < inf)) return false;
            unsigned pa = 0u, pb = 0xffffffffu;               // pa: 1 + max position of an unassigned minimum; pb: min position of a minimum
            for (int j = lane; j < C; j += 64) {
                const int pj = L.pos[j];
                if (pj >= 0 && L.dist[j] == m) {
                    pb = min(pb, (unsigned)pj);
                    if (L.rowof[j] < 0) pa = max(pa, (unsigned)pj + 1u);
                }
            }
            pa = wave_umax32(pa);
            const int pick = pa ? (int)pa - 1 : (int)wave_umin32(pb);
            base = m;
            const int j = L.todo[pick];
            const int rj = L.rowof[j];
            if (rj < 0) sink = j; else i = rj;
            if (lane == 0) {
                const int last = L.todo[live - 1];
                L.todo[pick] = last;
                L.pos[last] = pick;
                L.pos[j] = -1;                                  // scanned
            }
            --live;
            wave_lds_sync();
        }
        // dual update (lsap.cpp:83-87), column side: every scanned assigned column's partner row is a seen row
        for (int j = lane; j < C; j += 64) {
            if (L.pos[j] < 0) {
                const double dlt = base - L.dist[j];
                const int i2 = L.rowof[j];
                if (i2 >= 0) L.u[i2] = L.u[i2] + dlt;
                L.v[j] = L.v[j] - dlt;
            }
        }
        wave_lds_sync();
        if (lane == 0) {
            L.u[root] = L.u[root] + base;
            int j = sink;
            for (;;) {                                          // flip the path back to the root
                const int i2 = L.pred[j];
                L.rowof[j] = i2;
                const int t = L.colof[i2];
                L.colof[i2] = j;
                j = t;
                if (i2 == root) break;
            }
        }
        wave_lds_sync();
    }
    if (!tall) {
        for (int r2 = lane; r2 < nr; r2 += 64) L.asg[r2] = L.colof[r2];
    } else {
        for (int r2 = lane; r2 < nr; r2 += 64) L.asg[r2] = L.rowof[r2];   // solver columns = original rows
    }
    wave_lds_sync();
    return true;
}

__device__ __forceinline__ double readlane_f64(double x, int l) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// The same algorithm with max(nr, nc) <= 64: lane j IS column j (dist, v, pred, row_of_col, list position in registers), lane i
// IS row i (u, col_of_row); the list of unscanned columns is only its inverse pos[] (the lane whose pos == p sits at list
// position p).  LDS is touched for the cost entries alone.
template <class Lds>
__device__ __noinline__ bool lsap_wave64(const float* cm, int nr, int nc, const Lds& L, int lane, int ld = 0) {
    if (ld == 0) ld = nc;                                         // row pitch of cm (the wave cascade pads it to an odd number of words)
    const bool tall = nr > nc;
    const int R = tall ? nc : nr, C = tall ? nr : nc;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double v = 0.0, u = 0.0, dist = inf;
    int rowof = -1, colof = -1, pred = -1;
    for (int root = 0; root < R; ++root) {
        dist = inf;
        int pos = lane < C ? C - 1 - lane : -1;
        bool seen = false;
        double base = 0.0;
        int live = C, i = root, sink = -1;
        while (sink < 0) {
            const double ui = readlane_f64(u, i);
            if (pos >= 0) {
                const float cij = tall ? cm[lane * ld + i] : cm[i * ld + lane];
                const double red = ((base + (double)cij) - ui) - v;
                if (red < dist) { dist = red; pred = i; }
            }
            const double m = wave_min_f64(pos >= 0 ? dist : inf);
            if (!(m < inf)) return false;
            const bool cand = pos >= 0 && dist == m;
            const bool cand_u = cand && rowof < 0;
            const unsigned long long bu = __ballot(cand_u);
            int jp;
            if (bu) {                                              // the LAST visited unassigned minimum
                if (__popcll(bu) == 1) jp = __ffsll((long long)bu) - 1;
                else {
                    const unsigned pp = wave_umax32(cand_u ? (unsigned)pos + 1u : 0u) - 1u;
                    jp = __ffsll((long long)__ballot(cand_u && (unsigned)pos == pp)) - 1;
                }
            } else {                                               // the FIRST visited minimum
                const unsigned long long bc = __ballot(cand);
                if (__popcll(bc) == 1) jp = __ffsll((long long)bc) - 1;
                else {
                    const unsigned pp = wave_umin32(cand ? (unsigned)pos : 0xffffffffu);
                    jp = __ffsll((long long)__ballot(cand && (unsigned)pos == pp)) - 1;
                }
            }
            jp = __builtin_amdgcn_readfirstlane(jp);
            base = m;
            const int pick = __builtin_amdgcn_readlane(pos, jp);
            const int rj = __builtin_amdgcn_readlane(rowof, jp);
            if (rj < 0) sink = jp; else i = rj;
            const int jl = __ffsll((long long)__ballot(pos == live - 1)) - 1;   // the list's last entry moves into the freed place
            if (lane == jl) pos = pick;
            if (lane == jp) { pos = -1; seen = true; }
            --live;
        }
        // dual update (lsap.cpp:83-87): a seen row is the partner of a scanned assigned column
        const double dlt = base - dist;
        {
            const int src = colof >= 0 ? colof : 0;
            const double dl = __shfl(dlt, src);
            const int sn = __shfl((int)seen, src);
            if (lane < R && colof >= 0 && sn) u = u + dl;
        }
        if (seen) v = v - dlt;
        if (lane == root) u = u + base;
        int j = sink;
        for (;;) {                                                 // flip the path back to the root
            const int i2 = __builtin_amdgcn_readlane(pred, j);
            if (lane == j) rowof = i2;
            const int t = __builtin_amdgcn_readlane(colof, i2);
            if (lane == i2) colof = j;
            j = t;
            if (i2 == root) break;
        }
    }
    if (lane < nr) L.asg[lane] = tall ? rowof : colof;
    wave_lds_sync();
    return true;
}

// Register-resident form for up to 64 * CPL columns: lane l holds columns l, l + 64, ... (and rows likewise).  Same algorithm and
// tie rules as lsap_wave64 (CPL = 1 compiles to it); every register array is indexed by unrolled constants only.
template <int CPL, class Lds>
__device__ __noinline__ bool lsap_wave_reg(const float* cm, int nr, int nc, const Lds& L, int lane) {
    const bool tall = nr > nc;
    const int R = tall ? nc : nr, C = tall ? nr : nc;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double v[CPL], u[CPL], dist[CPL];
    int rowof[CPL], colof[CPL], pred[CPL], pos[CPL];
    bool seen[CPL];
#pragma unroll
    for (int s = 0; s < CPL; ++s) { v[s] = 0.0; u[s] = 0.0; dist[s] = inf; rowof[s] = -1; colof[s] = -1; pred[s] = -1; }
    auto pick_i = [&](const int (&a)[CPL], int idx) {            // a[idx >> 6] on lane idx & 63, idx uniform
        int x = a[0];
#pragma unroll
        for (int s = 1; s < CPL; ++s) if ((idx >> 6) == s) x = a[s];
        return __builtin_amdgcn_readlane(x, idx & 63);
    };
    for (int root = 0; root < R; ++root) {
#pragma unroll
        for (int s = 0; s < CPL; ++s) {
            const int j = lane + 64 * s;
            dist[s] = inf;
            pos[s] = j < C ? C - 1 - j : -1;
            seen[s] = false;
        }
        double base = 0.0;
        int live = C, i = root, sink = -1;
        while (sink < 0) {
            double us = u[0];
#pragma unroll
            for (int s = 1; s < CPL; ++s) if ((i >> 6) == s) us = u[s];
            const double ui = readlane_f64(us, i & 63);
            double lmin = inf;
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                if (pos[s] >= 0) {
                    const int j = lane + 64 * s;
                    const float cij = tall ? cm[(size_t)j * nc + i] : cm[(size_t)i * nc + j];
                    const double red = ((base + (double)cij) - ui) - v[s];
                    if (red < dist[s]) { dist[s] = red; pred[s] = i; }
                    lmin = dist[s] < lmin ? dist[s] : lmin;
                }
            }
            const double m = wave_min_f64(lmin);
            if (!(m < inf)) return false;
            unsigned pa = 0u, pb = 0xffffffffu;
            int ncand = 0;
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                const bool cand = pos[s] >= 0 && dist[s] == m;
                ncand += __popcll(__ballot(cand));
                if (cand) {
                    pb = min(pb, (unsigned)pos[s]);
                    if (rowof[s] < 0) pa = max(pa, (unsigned)pos[s] + 1u);
                }
            }
            int pick;
            if (ncand == 1) pick = (int)wave_umin32(pb);            // (one lane holds it; a 32-bit reduce is cheaper than locating it twice)
            else {
                const unsigned pam = wave_umax32(pa);
                pick = pam ? (int)pam - 1 : (int)wave_umin32(pb);
            }
            base = m;
            int jp = 0, jl = 0;
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                const unsigned long long b1 = __ballot(pos[s] == pick);
                if (b1) jp = 64 * s + __ffsll((long long)b1) - 1;
                const unsigned long long b2 = __ballot(pos[s] == live - 1);
                if (b2) jl = 64 * s + __ffsll((long long)b2) - 1;
            }
            const int rj = pick_i(rowof, jp);
            if (rj < 0) sink = jp; else i = rj;
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                const int j = lane + 64 * s;
                if (j == jl) pos[s] = pick;                        // the list's last entry moves into the freed place
                if (j == jp) { pos[s] = -1; seen[s] = true; }
            }
            --live;
        }
        // dual update (lsap.cpp:83-87)
        double dlt[CPL];
#pragma unroll
        for (int s = 0; s < CPL; ++s) dlt[s] = base - dist[s];
#pragma unroll
        for (int s = 0; s < CPL; ++s) {                           // row (lane, s): partner column colof[s] = lane' + 64 * s2
            const int cj = colof[s] >= 0 ? colof[s] : 0;
            double dl = 0.0;
            int sn = 0;
#pragma unroll
            for (int s2 = 0; s2 < CPL; ++s2) {
                const double d2 = __shfl(dlt[s2], cj & 63);
                const int n2 = __shfl((int)seen[s2], cj & 63);
                if ((cj >> 6) == s2) { dl = d2; sn = n2; }
            }
            if (lane + 64 * s < R && colof[s] >= 0 && sn) u[s] = u[s] + dl;
        }
#pragma unroll
        for (int s = 0; s < CPL; ++s) {
            if (seen[s]) v[s] = v[s] - dlt[s];
            if (lane + 64 * s == root) u[s] = u[s] + base;
        }
        int j = sink;
        for (;;) {                                                 // flip the path back to the root
            const int i2 = pick_i(pred, j);
            const int t = pick_i(colof, i2);
#pragma unroll
            for (int s = 0; s < CPL; ++s) {
                if (lane + 64 * s == j) rowof[s] = i2;
                if (lane + 64 * s == i2) colof[s] = j;
            }
            j = t;
            if (i2 == root) break;
        }
    }
#pragma unroll
    for (int s = 0; s < CPL; ++s)
        if (lane + 64 * s < nr) L.asg[lane + 64 * s] = tall ? rowof[s] : colof[s];
    wave_lds_sync();
    return true;
}

}  // namespace
}  // namespace aic
