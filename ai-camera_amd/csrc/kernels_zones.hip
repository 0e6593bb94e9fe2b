// kernels_zones.hip -- the two kernels of the zone / line counting stage (zones.hpp).  Integer arithmetic only:
// coordinates are doubled int32 (|v| <= 2^21), differences fit 2^22 and a cross product 2^45, held in int64.
//
// zones_classify_kernel  stateless, one block per frame of the call: 8 rows x 32 zones per pass, one lane per (row, zone) walks the
//                        polygon's edges from LDS, a ballot folds the 32 answers of a row into its inside mask.
// zones_walk_kernel      one block of 512 threads per stream, the stream's frames in order.  The slot table lives in LDS for the
//                        launch (enter frames stay in global memory: they are touched by events only).  A thread is slot t of the
//                        table AND row t of the frame.
#include "zones.hpp"
#include "stage_dev.hpp"

namespace aic {

namespace {

constexpr int POLY_STRIDE = 2 * ZONES_VERTS_MAX + 1;   // odd: lanes = zones fall on distinct LDS banks

__global__ __launch_bounds__(256) void zones_classify_kernel(const int* __restrict__ frame_off, const int* __restrict__ frame_stream,
                                                             const int* __restrict__ rows6, const int* __restrict__ geo, int anchor_centre,
                                                             int4* __restrict__ cls4) {
    __shared__ int s_poly[ZONES_MAX * POLY_STRIDE];
    __shared__ int s_nv[ZONES_MAX];
    const int fi = blockIdx.x, tid = threadIdx.x;
    const int off = frame_off[fi], n = frame_off[fi + 1] - off;
    if (n <= 0) return;
    const int* g = geo + (size_t)frame_stream[fi] * ZONES_GEO_INTS;
    const int nz = g[0];
    for (int i = tid; i < ZONES_MAX * ZONES_VERTS_MAX * 2; i += 256) s_poly[(i >> 6) * POLY_STRIDE + (i & 63)] = g[ZONES_GEO_XY + i];
    if (tid < ZONES_MAX) s_nv[tid] = g[ZONES_GEO_NVERT + tid];
    __syncthreads();
    const int z = tid & 31, sub = tid >> 5;
    for (int r0 = 0; r0 < n; r0 += 8) {
        const int r = r0 + sub;
        const bool act = r < n;
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
        if (act) {
            const int* row = rows6 + (size_t)(off + r) * 6;
            x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
        }
        const int lim = ZONES_COORD_MAX;
        const bool valid = act && x1 >= -lim && x1 <= lim && y1 >= -lim && y1 <= lim && x2 >= -lim && x2 <= lim && y2 >= -lim && y2 <= lim;
        const int px = valid ? x1 + x2 : 0;
        const int py = valid ? (anchor_centre ? y1 + y2 : 2 * y2) : 0;
        bool in = false;
        if (valid && z < nz) {
            const int nv = s_nv[z];
            const int* p = s_poly + z * POLY_STRIDE;
            int ax = p[2 * (nv - 1)], ay = p[2 * (nv - 1) + 1];          // edge (a, b) = (vertex i - 1, vertex i): every edge once
            for (int i = 0; i < nv; ++i) {
                const int bx = p[2 * i], by = p[2 * i + 1];
                const long long d = (long long)(bx - ax) * (py - ay) - (long long)(px - ax) * (by - ay);
                if (((ay > py) != (by > py)) && ((d > 0) == (by > ay))) in = !in;
                ax = bx, ay = by;
            }
        }
        const unsigned long long b = __ballot(in);
        if (act && z == 0) cls4[off + r] = make_int4(px, py, (int)(unsigned)(b >> (32 * ((tid & 63) >> 5))), valid ? 1 : 0);
    }
}

__device__ __forceinline__ void put_event(int* __restrict__ ev, int e, int cap, int kind, int index, int id, int cls, int frame, int value, int ax, int ay) {
    if (e < cap) {
        int4* p = reinterpret_cast<int4*>(ev + (size_t)e * 8);
        p[0] = make_int4(kind, index, id, cls);
        p[1] = make_int4(frame, value, ax, ay);
    }
}

__device__ __forceinline__ long long cross64(int ux, int uy, int vx, int vy) { return (long long)ux * vy - (long long)vx * uy; }

__global__ __launch_bounds__(512) void zones_walk_kernel(const int* __restrict__ fps, const int* __restrict__ fstart, const int* __restrict__ reset,
                                                         const int* __restrict__ frame_off, const int* __restrict__ rows6,
                                                         const int4* __restrict__ cls4, const int* __restrict__ geo, int* __restrict__ state_all,
                                                         long long* __restrict__ counters, int max_tracks, int forget_after, int first, int f_lo,
                                                         int f_hi, int cap, int* __restrict__ n_events, int* __restrict__ events,
                                                         int* __restrict__ occupancy, int* __restrict__ status) {
    constexpr int T = ZONES_TRACKS_MAX;
    __shared__ int s_id[T], s_last[T], s_ax[T], s_ay[T], s_mask[T], s_cls[T];
    __shared__ int s_live[T], s_free[T], r_id[T], r_val[T];
    __shared__ int s_line[ZONES_LINES_MAX * 4];
    __shared__ int s_part[8][6][32];
    __shared__ int s_w[8];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int* st = state_all + (size_t)s * ZONES_ST_INTS;
    int* enter = st + ZONES_ST_ENTER;
    long long* cnt = counters + (size_t)s * ZONES_CNT;
    const int* g = geo + (size_t)s * ZONES_GEO_INTS;
    const int nz = g[0], nl = g[1];
    const bool fresh = first && reset[s];
    int frame = fresh ? 0 : st[0];
    int stopped = fresh ? 0 : st[1];
    if (fresh) {
        s_id[tid] = 0, s_last[tid] = -1, s_ax[tid] = 0, s_ay[tid] = 0, s_mask[tid] = 0, s_cls[tid] = 0;
    } else {
        s_id[tid] = st[ZONES_ST_SLOTS + tid], s_last[tid] = st[ZONES_ST_SLOTS + T + tid], s_ax[tid] = st[ZONES_ST_SLOTS + 2 * T + tid];
        s_ay[tid] = st[ZONES_ST_SLOTS + 3 * T + tid], s_mask[tid] = st[ZONES_ST_SLOTS + 4 * T + tid], s_cls[tid] = st[ZONES_ST_SLOTS + 5 * T + tid];
    }
    if (tid < ZONES_LINES_MAX * 4) s_line[tid] = g[ZONES_GEO_LINES + tid];
    // thread b < 32 carries the four counters of zone / line b
    long long c_in = 0, c_out = 0, c_pos = 0, c_neg = 0;
    if (tid < 32 && !fresh) c_in = cnt[tid], c_out = cnt[32 + tid], c_pos = cnt[64 + tid], c_neg = cnt[96 + tid];
    __syncthreads();

    const int nf = fps[s];
    const int k_hi = f_hi < nf ? f_hi : nf;
    for (int k = f_lo; k < k_hi && !stopped; ++k) {
        const int fi = fstart[s] + k;
        const int off = frame_off[fi], n = frame_off[fi + 1] - off;          // 0..512, checked by the host
        // ---- this thread as row tid
        int rid = 0, rcls = 0, ax = 0, ay = 0, mask = 0, valid = 0;
        if (tid < n) {
            const int4 c = cls4[off + tid];
            ax = c.x, ay = c.y, mask = c.z, valid = c.w;
            rid = rows6[(size_t)(off + tid) * 6 + 4], rcls = rows6[(size_t)(off + tid) * 6 + 5];
        }
        r_id[tid] = rid, r_val[tid] = valid;
        // ---- this thread as slot tid
        const bool used = tid < max_tracks && s_last[tid] >= 0;
        const bool expiring = used && frame - s_last[tid] > forget_after;
        s_live[tid] = used && !expiring;
        const int o_id = s_id[tid], o_last = s_last[tid], o_ax = s_ax[tid], o_ay = s_ay[tid], o_mask = s_mask[tid], o_cls = s_cls[tid];
        __syncthreads();
        bool counted = valid;
        for (int r = 0; r < n; ++r) counted = counted && !(r < tid && r_val[r] && r_id[r] == rid);      // the first row of an id wins
        int slot = -1;
        if (counted)
            for (int t = 0; t < max_tracks; ++t)
                if (s_live[t] && s_id[t] == rid) slot = t;
        const bool is_new = counted && slot < 0;
        int n_new, n_free;
        const int new_rank = block_scan(is_new, s_w, n_new);
        const bool is_free = tid < max_tracks && !s_live[tid];               // free now or freed by this frame's expiry
        const int free_rank = block_scan(is_free, s_w, n_free);
        if (n_new > n_free) {                                                // nothing of this frame is committed
            stopped = AIC_ERR_CAPACITY;
            break;
        }
        if (is_free) s_free[free_rank] = tid;
        // ---- what this thread emits: as a slot, LOST per zone it was inside; as a row, EXIT / ENTER per changed zone, CROSS per line
        const unsigned e_mask = expiring ? (unsigned)o_mask : 0u;
        unsigned m_in = 0, m_out = 0, m_pos = 0, m_neg = 0;
        if (counted) {
            if (slot < 0) m_in = (unsigned)mask;
            else {
                const unsigned was = (unsigned)s_mask[slot];
                m_in = (unsigned)mask & ~was, m_out = was & ~(unsigned)mask;
                const int p0x = s_ax[slot], p0y = s_ay[slot];
                for (int l = 0; l < nl; ++l) {
                    const int lax = s_line[4 * l], lay = s_line[4 * l + 1], lbx = s_line[4 * l + 2], lby = s_line[4 * l + 3];
                    const bool s0 = cross64(lbx - lax, lby - lay, p0x - lax, p0y - lay) >= 0;
                    const bool s1 = cross64(lbx - lax, lby - lay, ax - lax, ay - lay) >= 0;
                    const bool ta = cross64(ax - p0x, ay - p0y, lax - p0x, lay - p0y) >= 0;
                    const bool tb = cross64(ax - p0x, ay - p0y, lbx - p0x, lby - p0y) >= 0;
                    if (s0 != s1 && ta != tb) (s1 ? m_pos : m_neg) |= 1u << l;
                }
            }
        }
        int n_e, n_r;
        const int e_off = block_scan(__popc(e_mask), s_w, n_e);
        const int r_off = block_scan(__popc(m_in | m_out) + __popc(m_pos | m_neg), s_w, n_r);   // the scans' barriers also publish s_free
        // ---- per-index counts of the frame: ballots per wave, summed by thread b
        const unsigned m_occ = counted ? (unsigned)mask : 0u;
        const int nb = nz > nl ? nz : nl;
        for (int b = 0; b < nb; ++b) {
            const int v0 = __popcll(__ballot(m_in >> b & 1)), v1 = __popcll(__ballot(m_out >> b & 1)), v2 = __popcll(__ballot(e_mask >> b & 1));
            const int v3 = __popcll(__ballot(m_pos >> b & 1)), v4 = __popcll(__ballot(m_neg >> b & 1)), v5 = __popcll(__ballot(m_occ >> b & 1));
            if (lane == 0) s_part[wv][0][b] = v0, s_part[wv][1][b] = v1, s_part[wv][2][b] = v2, s_part[wv][3][b] = v3, s_part[wv][4][b] = v4, s_part[wv][5][b] = v5;
        }
        int* ev = events + (size_t)fi * cap * 8;
        if (e_mask) {                                                        // expiry: reads its enter frames before a row may reuse the slot
            int e = e_off;
            for (int z = 0; z < nz; ++z)
                if (e_mask >> z & 1) put_event(ev, e++, cap, 3, z, o_id, o_cls, frame, o_last + 1 - enter[tid * ZONES_MAX + z], o_ax, o_ay);
        }
        if (expiring) s_last[tid] = -1;
        __syncthreads();
        if (tid < nb) {
            int t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
            for (int w = 0; w < 8; ++w)
                t0 += s_part[w][0][tid], t1 += s_part[w][1][tid], t2 += s_part[w][2][tid], t3 += s_part[w][3][tid], t4 += s_part[w][4][tid], t5 += s_part[w][5][tid];
            c_in += t0, c_out += t1 + t2, c_pos += t3, c_neg += t4;
            occupancy[(size_t)fi * ZONES_MAX + tid] = t5;
        }
        if (tid == 0) n_events[fi] = n_e + n_r;
        if (counted) {
            if (slot < 0) slot = s_free[new_rank];                           // the k-th new row takes the k-th lowest free slot
            int e = n_e + r_off;
            const unsigned chg = m_in | m_out;
            for (int z = 0; z < nz; ++z)
                if (chg >> z & 1) {
                    if (m_in >> z & 1) {
                        enter[slot * ZONES_MAX + z] = frame;
                        put_event(ev, e++, cap, 1, z, rid, rcls, frame, 0, ax, ay);
                    } else put_event(ev, e++, cap, 2, z, rid, rcls, frame, frame - enter[slot * ZONES_MAX + z], ax, ay);
                }
            for (int l = 0; l < nl; ++l)
                if ((m_pos | m_neg) >> l & 1) put_event(ev, e++, cap, 4, l, rid, rcls, frame, (m_pos >> l & 1) ? 1 : -1, ax, ay);
            s_id[slot] = rid, s_last[slot] = frame, s_ax[slot] = ax, s_ay[slot] = ay, s_mask[slot] = mask, s_cls[slot] = rcls;
        }
        ++frame;
        __syncthreads();
    }
    __syncthreads();
    st[ZONES_ST_SLOTS + tid] = s_id[tid], st[ZONES_ST_SLOTS + T + tid] = s_last[tid], st[ZONES_ST_SLOTS + 2 * T + tid] = s_ax[tid];
    st[ZONES_ST_SLOTS + 3 * T + tid] = s_ay[tid], st[ZONES_ST_SLOTS + 4 * T + tid] = s_mask[tid], st[ZONES_ST_SLOTS + 5 * T + tid] = s_cls[tid];
    if (tid < 32) cnt[tid] = c_in, cnt[32 + tid] = c_out, cnt[64 + tid] = c_pos, cnt[96 + tid] = c_neg;
    if (tid == 0) st[0] = frame, st[1] = stopped, status[s] = stopped;
}

}  // namespace

void launch_zones_classify(const int* frame_off, const int* frame_stream, int n_frames, const int* rows6, const int* geo, int anchor_centre, int* cls4,
                           hipStream_t s) {
    if (n_frames <= 0) return;
    hipLaunchKernelGGL(zones_classify_kernel, dim3(n_frames), dim3(256), 0, s, frame_off, frame_stream, rows6, geo, anchor_centre,
                       reinterpret_cast<int4*>(cls4));
    KCHECK();
}

void launch_zones_walk(const int* fps, const int* fstart, const int* reset, const int* frame_off, const int* rows6, const int* cls4, const int* geo,
                       int* state, long long* counters, int streams, int max_tracks, int forget_after, int first, int f_lo, int f_hi, int cap_events,
                       int* n_events, int* events, int* occupancy, int* status, hipStream_t s) {
    hipLaunchKernelGGL(zones_walk_kernel, dim3(streams), dim3(ZONES_TRACKS_MAX), 0, s, fps, fstart, reset, frame_off, rows6,
                       reinterpret_cast<const int4*>(cls4), geo, state, counters, max_tracks, forget_after, first, f_lo, f_hi, cap_events, n_events,
                       events, occupancy, status);
    KCHECK();
}

}  // namespace aic
