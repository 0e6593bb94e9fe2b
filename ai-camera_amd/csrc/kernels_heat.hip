// kernels_heat.hip -- the kernels of the heat-map stage (heat.hpp).  Integer arithmetic only; tests/heat_oracle.py is
// the specification.  No scratch.
//
// heat_walk_kernel    one block of 512 threads per stream, the launch's ticks in order: the life cycle is slot_walk.hpp's, HeatWalk states
//                     what is this stage's.  A thread is slot t of the table AND row t of the frame.  The sixteen small arrays of the table
//                     live in LDS for the launch (32 KiB).  The stage has no sample kernel in front of it, so load_row finds the FIRST row
//                     of an id itself: ids and validity go through two LDS arrays of the variant and a row looks at the rows before it.
//                     The twelve layers stay in HBM (1.5 MB at 32768 cells does not fit LDS; a tick touches a handful of cells) and only
//                     this block touches its stream's layers during a launch.  commit adds with integer atomicAdd (one tick adds at most
//                     512 to a cell: no wrap below 2^30 + 512) and an add that finds its cell at 2^30 or above takes itself back, which
//                     leaves min(old + n, 2^30) whatever the order, without a barrier (see bump: a first form, atomicMin behind
//                     __threadfence and a barrier, cost 77 us a launch at 256 streams where this one costs 21 us, as at one stream).
//                     event adds ENDS when a track's event leaves the table.  Nothing touches a layer before the skeleton's capacity
//                     check has passed: commit and event lie behind it.
// heat_decay_kernel   v >>= shift, elementwise over the masked layers.
// heat_levels_kernel  one block of 1024 threads per camera a render call names: the maximum M of the layer, then every cell's u16 level.
//                     A kernel of its own: the maximum is a reduction over the whole layer (up to 128 KB) that each of the thousands of
//                     render blocks would otherwise repeat; here a layer is read twice by one block.
// heat_render_kernel  the per-pixel pass, HBM-bound: every touched byte is read once and written at most once.  A block takes HT_BAND pixel
//                     rows of one frame: whole rows, so ONE contiguous byte range of the bank that may start at any byte (a frame of odd
//                     H * W * 3 moves every later frame).  The range is cut into items of three ALIGNED dwords; a lane loads its item,
//                     shifts it to pixel alignment (at most five pixels reach into twelve bytes), blends, shifts back and stores whole
//                     dwords that changed; the at most two dwords that straddle the range's ends are shared with the neighbouring block
//                     and are written bytewise, each block its own bytes.  The level rows the band needs (at most HT_BAND / cell + 2 rows
//                     of the camera's grid) are staged in LDS together with the hottest level per cell column; a wave's run of 256 pixels
//                     whose contributing columns are all below `floor` is skipped without reading the frame, a band whose rows are and a
//                     camera with M = 0 leave before staging.
#include "heat.hpp"
#include "slot_walk.hpp"

namespace aic {

namespace {

constexpr int T = HT_TRACKS_MAX;

// what the heat stage states of the slot walk (slot_walk.hpp): where a track stood last and its path sums; the layers in HBM; the row tags
struct HeatWalk {
    static constexpr int ARRAYS = HT_ARRAYS, ST_INTS = HT_ST_INTS, EVENT_INTS = HT_EVENT_INTS;
    struct Row {
        int flags, cell, fx, fy;
        bool visit, start;
        int4 tag;
    };
    const int* rows6;
    HeatGeom g;
    int* lay;                                                                // [12][cells] of the stream
    int4* row_tags;
    int *s_rid, *s_rok;                                                      // [512] the tick's row ids and validity

    // min(old + 1, 2^30) whatever the order: an add that finds the cell at or above 2^30 takes itself back, so when all adds of a tick have
    // returned the cell holds min(old + n, 2^30) exactly (it never exceeds 2^30 + 512 on the way: no wrap).  No barrier, no fence: the
    // layers are read by nobody but these atomics before the kernel ends.
    __device__ __forceinline__ void bump(int l, int cell) const {
        int* p = lay + (size_t)l * (g.gw * g.gh) + cell;
        if (atomicAdd(p, 1) >= HEAT_SAT) atomicSub(p, 1);
    }
    __device__ __forceinline__ Row load_row(int r, bool in) const {
        const int tid = threadIdx.x;
        Row x{0, 0, 0, 0, false, false, make_int4(-1, 0, 0, -1)};
        int x1 = 0, y1 = 0, x2 = 0, y2 = 0, id = 0;
        bool ok = false;
        if (in) {
            const int* q = rows6 + (size_t)r * 6;
            x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3], id = q[4];
            ok = row_valid(x1, y1, x2, y2, HT_COORD_MAX);
        }
        __syncthreads();                                                     // the last tick's readers are through
        s_rid[tid] = id, s_rok[tid] = ok;
        __syncthreads();
        if (ok) {
            bool dup = false;
            for (int j = 0; j < tid; ++j) dup = dup || (s_rok[j] && s_rid[j] == id);
            const bool nonempty = x1 < g.w && x2 >= 0 && y1 < g.h && y2 >= 0;
            x.flags = SLOT_F_VALID | (dup ? 0 : SLOT_F_FIRST) | (nonempty ? SLOT_F_NONEMPTY : 0);
            x.fx = heat_fx(x1, x2, g.w), x.fy = heat_fy(y1, y2, g.h, g.anchor);
            x.cell = ((x.fy >> 1) >> g.lc) * g.gw + ((x.fx >> 1) >> g.lc);
        }
        return x;
    }
    __device__ __forceinline__ void fresh(const SlotLds& L, int slot) const {
        L.tab[HT_A_CELL][slot] = -1;                                         // commit sees a new cell
        L.tab[HT_A_PATH][slot] = 0, L.tab[HT_A_INCELL][slot] = 0, L.tab[HT_A_MAXSTEP][slot] = 0, L.tab[HT_A_CELLS][slot] = 0, L.tab[HT_A_MOVING][slot] = 0;
    }
    __device__ __forceinline__ void commit(const SlotLds& L, Row& row, int slot, bool fresh_slot, int frame) const {
        int step = 0, oct = -1;
        if (fresh_slot) {
            L.tab[HT_A_SFX][slot] = row.fx, L.tab[HT_A_SFY][slot] = row.fy;
            row.start = true;
        } else {
            const int dx = row.fx - L.tab[HT_A_FX][slot], dy = row.fy - L.tab[HT_A_FY][slot];
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            step = ax > ay ? ax : ay;
            if (step >= g.min_move) {
                oct = heat_octant(dx, dy);
                L.tab[HT_A_MOVING][slot] = heat_sat_add(L.tab[HT_A_MOVING][slot], 1);
            }
            L.tab[HT_A_PATH][slot] = heat_sat_add(L.tab[HT_A_PATH][slot], step);
            L.tab[HT_A_MAXSTEP][slot] = imax(L.tab[HT_A_MAXSTEP][slot], step);
        }
        if (L.tab[HT_A_CELL][slot] != row.cell) {
            row.visit = true;
            L.tab[HT_A_CELL][slot] = row.cell;
            L.tab[HT_A_CELLS][slot] = heat_sat_add(L.tab[HT_A_CELLS][slot], 1);
            L.tab[HT_A_INCELL][slot] = 1;
        } else {
            L.tab[HT_A_INCELL][slot] = heat_sat_add(L.tab[HT_A_INCELL][slot], 1);
        }
        L.tab[HT_A_FX][slot] = row.fx, L.tab[HT_A_FY][slot] = row.fy;
        bump(HEAT_DWELL, row.cell);
        if (row.visit) bump(HEAT_VISITS, row.cell);
        if (row.start) bump(HEAT_STARTS, row.cell);
        if (oct >= 0) bump(HEAT_DIR0 + oct, row.cell);
        row.tag = make_int4(row.cell, L.tab[HT_A_INCELL][slot], step, oct);
    }
    __device__ __forceinline__ void event(const SlotLds& L, int4* ev, int s, int e_rank) const {
        const int tid = threadIdx.x;
        slot_event_head(L, ev, s, L.tab[HT_A_CELLS][tid]);
        ev[2] = make_int4(L.tab[HT_A_SFX][tid], L.tab[HT_A_SFY][tid], L.tab[HT_A_FX][tid], L.tab[HT_A_FY][tid]);
        ev[3] = make_int4(L.tab[HT_A_PATH][tid], L.tab[HT_A_MAXSTEP][tid], L.tab[HT_A_MOVING][tid], L.tab[HT_A_CELL][tid]);
        bump(HEAT_ENDS, L.tab[HT_A_CELL][tid]);
    }
    __device__ __forceinline__ void post_emit(const SlotLds& L, bool em, int n_emit, int n_out) const {
        if (em) L.tab[SLOT_A_STATE][threadIdx.x] = 0;
        __syncthreads();                                                     // the slot's arrays are read before a row may take the slot
    }
    __device__ __forceinline__ void post_tick(const SlotLds& L, const Row& row, int slot, int off, int n, int& stopped) const {
        if (row_tags && (int)threadIdx.x < n) row_tags[off + threadIdx.x] = row.tag;
    }
    __device__ __forceinline__ void tail(const SlotCall& c, int kk) const {
        if (row_tags)                                                        // a stopped stream's rows: the tick it stopped at and all after
            for (; kk < c.n_ticks; ++kk) {
                const int x = kk * c.streams + blockIdx.x;
                const int off = c.frame_off[x], n = c.frame_off[x + 1] - off;
                if ((int)threadIdx.x < n) row_tags[off + threadIdx.x] = make_int4(-1, 0, 0, -1);
            }
    }
};

__global__ __launch_bounds__(512) void heat_walk_kernel(const int* __restrict__ frame_off, int n_ticks, const int* __restrict__ rows6,
                                                        const int* __restrict__ reset, const int* __restrict__ mode, int first, HeatGeom g,
                                                        int* state_all, int* layers, int cap, int* __restrict__ n_final, int* __restrict__ pending,
                                                        int* __restrict__ status, int* __restrict__ events, int4* __restrict__ row_tags) {
    __shared__ int s_rid[T], s_rok[T];
    const SlotCall c{frame_off, n_ticks, rows6, reset, mode, first, g.streams, g.max_tracks, g.forget_after, state_all, cap, n_final, pending, status,
                     events};
    HeatWalk v{rows6, g, layers + (size_t)blockIdx.x * HEAT_LAYERS * g.gw * g.gh, row_tags, s_rid, s_rok};
    slot_walk(c, v);
}

__global__ __launch_bounds__(256) void heat_decay_kernel(int* layers, int cells, int stream, int streams, int layer_mask, int shift) {
    const int l = blockIdx.y, s = stream < 0 ? blockIdx.z : stream;
    if (!((layer_mask >> l) & 1)) return;
    int* p = layers + ((size_t)s * HEAT_LAYERS + l) * cells;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < cells; i += gridDim.x * 256) p[i] >>= shift;
}

__global__ __launch_bounds__(1024) void heat_levels_kernel(const int* __restrict__ layers, int cells, int layer, int scale, const int* __restrict__ used,
                                                           int* __restrict__ maxima, uint16_t* __restrict__ levels) {
    __shared__ int s_m[16];
    const int s = used[blockIdx.x], tid = threadIdx.x;
    const int* p = layers + ((size_t)s * HEAT_LAYERS + layer) * cells;
    int m = 0;
    for (int i = tid; i < cells; i += 1024) m = imax(m, p[i]);
    m = wave_max(m);
    if ((tid & 63) == 0) s_m[tid >> 6] = m;
    __syncthreads();
    m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) m = imax(m, s_m[i]);
    if (tid == 0) maxima[s] = m;
    if (m == 0) return;
    uint16_t* q = levels + (size_t)s * cells;
    for (int i = tid; i < cells; i += 1024) q[i] = (uint16_t)heat_level(p[i], m, scale);
}

// byte k of the 16 bytes e[0..3]
__device__ __forceinline__ unsigned byte_of(const unsigned* e, int k) { return (e[k >> 2] >> ((k & 3) * 8)) & 255u; }

__global__ __launch_bounds__(256) void heat_render_kernel(uint8_t* frames, const int* __restrict__ frame_cam, HeatGeom g, const int* __restrict__ maxima,
                                                          const uint16_t* __restrict__ levels, const unsigned* __restrict__ lut, int alpha, int floor, unsigned w_magic) {
    extern __shared__ unsigned s_mem[];                                      // lut[256] | hot[gw] | rows[n_rows][gw] as u16
    const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int cam = frame_cam[f];
    if (maxima[cam] == 0) return;
    const int lc = g.lc, gw = g.gw, W = g.w;
    const int y0 = blockIdx.x * HT_BAND, y1 = imin(y0 + HT_BAND, g.h);       // the band's pixel rows [y0, y1)
    int cy0, cy1, cyb, wy_;
    heat_axis(y0, lc, g.gh, &cy0, &cyb, &wy_);
    heat_axis(y1 - 1, lc, g.gh, &cyb, &cy1, &wy_);                           // level rows cy0 .. cy1 contribute
    const int n_rows = cy1 - cy0 + 1;
    uint2* s_lut = reinterpret_cast<uint2*>(s_mem);                          // LUT[L] * alpha + 128 per channel: B | G << 16, R
    int* s_hot = reinterpret_cast<int*>(s_mem + 512);
    uint16_t* s_lev = reinterpret_cast<uint16_t*>(s_mem + 512 + gw);
    const uint16_t* lev = levels + (size_t)cam * gw * g.gh;
    {
        const unsigned c = lut[tid], a = (unsigned)alpha;                    // <= 255 * 256 + 128: 16 bits
        s_lut[tid] = make_uint2(((c & 255u) * a + 128u) | (((c >> 8) & 255u) * a + 128u) << 16, ((c >> 16) & 255u) * a + 128u);
    }
    int any = 0, all = 1;
    for (int cx = tid; cx < gw; cx += 256) {
        int hot = 0;
        for (int r = 0; r < n_rows; ++r) {
            const int q = lev[(size_t)(cy0 + r) * gw + cx];
            s_lev[r * gw + cx] = (uint16_t)q;
            hot = imax(hot, q);
        }
        s_hot[cx] = hot;
        any |= ((hot + 128) >> 8) >= floor;
        all &= ((hot + 128) >> 8) >= floor;
    }
    if (!__syncthreads_or(any)) return;                                      // nothing in the band reaches the floor
    const bool all_hot = __syncthreads_and(all);                             // every column does: no run of the band can be skipped
    auto div_w = [&](int p) { return w_magic ? (int)__umulhi((unsigned)p, w_magic) : p; };      // p / W for 0 <= p < 2^18 (launch_heat_render)
    // ---- the band's bytes: [b0, b1) of the bank, items of 12 aligned bytes from the aligned address at or below b0
    const size_t b0 = ((size_t)f * g.h + y0) * W * 3;
    const int len = (y1 - y0) * W * 3;                                       // <= 8 * 16384 * 3
    const uintptr_t a = reinterpret_cast<uintptr_t>(frames) + b0;
    const int sh = (int)(a & 3);
    unsigned* base = reinterpret_cast<unsigned*>(a - sh);
    const int items = (sh + len + 11) / 12;
    const int c0 = (3 - sh % 3) % 3;                                         // the channel an item's first byte holds (sh = 3: a whole pixel earlier)
    const int n_px = c0 ? 5 : 4;
    const int last_dw = (sh + len - 1) >> 2;                                 // the last dword that holds a byte of the band
    const int n_band = (y1 - y0) * W, c2 = 2 << lc, sh2 = 2 * lc + 2 + 8, inv = 256 - alpha;
    for (int ib = 0; ib < items; ib += 256) {                                // (whole waves stay in step)
        const int i = ib + tid;
        const int r0 = 12 * i - sh;                                          // the band byte of the item's first byte
        const int p0 = (r0 - c0) / 3;                                        // its first pixel (r0 - c0 is a multiple of 3: exact; -1 at most)
        // ---- is any level column under this wave's run hot?  (wave-uniform: every lane looks at the run of lane 0 .. 63)
        bool hot = all_hot;
        if (!all_hot) {
            const int wp0 = imax(p0 - lane * 4, 0), wp1 = imin(wp0 + 4 * 64 + 4, n_band - 1);
            const int ya = div_w(wp0), yb = div_w(wp1);
            int ca = 0, cb = gw - 1, t0, t1, tw;
            if (ya == yb) {
                heat_axis(wp0 - ya * W, lc, gw, &ca, &t1, &tw);
                heat_axis(wp1 - yb * W, lc, gw, &t0, &cb, &tw);
            }
            int m = 0;
            for (int cx = ca + lane; cx <= cb; cx += 64) m = imax(m, s_hot[cx]);
            hot = ((wave_max(m) + 128) >> 8) >= floor;
        }
        if (!hot || i >= items) continue;
        unsigned* q = base + 3 * (size_t)i;
        const int dw = 3 * i;
        unsigned d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = dw + k <= last_dw ? q[k] : 0u;
        // ---- to pixel alignment: e byte t = item byte t - c0
        unsigned e[4], o[4];
        {
            const int sft = 8 * c0;
            e[0] = d[0] << sft;
            e[1] = (unsigned)((((unsigned long long)d[1] << 32) | d[0]) >> (32 - sft));
            e[2] = (unsigned)((((unsigned long long)d[2] << 32) | d[1]) >> (32 - sft));
            e[3] = c0 ? d[2] >> (32 - sft) : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = e[k];
        int y = 0, x = -1;                                                   // (p0 = -1: the previous band's last pixel)
        if (p0 >= 0) y = div_w(p0), x = p0 - y * W;
        // Along a pixel row the sum of heat_bilinear is linear in wx while the pixel stays between the same two cell centres:
        // sum + round = P + Q wx with P = 2 cell (q00 (2 cell - wy) + q10 wy) + round and Q = (q01 - q00)(2 cell - wy) + (q11 - q10) wy,
        // the same integers in another order (|Q wx| < 2^28).  P and Q are renewed when the pair or the row changes.
        int P = 0, Q = 0, cur = -2;                                          // cur: the pair's first cell, unclamped (-1 .. gw - 1)
        const uint16_t *ra = s_lev, *rb = s_lev;
        int wy = 0;
        auto row_setup = [&] {
            int iy0, iy1;
            heat_axis(y0 + y, lc, g.gh, &iy0, &iy1, &wy);
            ra = s_lev + (iy0 - cy0) * gw, rb = s_lev + (iy1 - cy0) * gw;
            cur = -2;
        };
        row_setup();
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (j < n_px) {
                const int p = p0 + j;
                if (p >= 0 && p < n_band) {
                    const int dx = 2 * x + 1 - (1 << lc), ic = dx >> (lc + 1);
                    if (ic != cur) {
                        cur = ic;
                        const int ix0 = imax(ic, 0), ix1 = imin(ic + 1, gw - 1);
                        const int a0 = ra[ix0] * (c2 - wy) + rb[ix0] * wy, a1 = ra[ix1] * (c2 - wy) + rb[ix1] * wy;
                        P = a0 * c2 + (128 << (2 * lc + 2)), Q = a1 - a0;
                    }
                    const int L = (P + Q * (dx & (c2 - 1))) >> sh2;
                    if (L >= floor) {
                        const uint2 c = s_lut[L];
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) {
                            const int k = 3 * j + ch;
                            const unsigned pre = ch == 0 ? c.x & 0xFFFFu : ch == 1 ? c.x >> 16 : c.y;
                            const unsigned v = (byte_of(e, k) * (unsigned)inv + pre) >> 8;
                            o[k >> 2] = (o[k >> 2] & ~(255u << ((k & 3) * 8))) | (v << ((k & 3) * 8));
                        }
                    }
                }
            }
            if (++x == W) {
                x = 0, ++y;
                if (y < y1 - y0) row_setup();
            }
        }
        // ---- back to the item's alignment, and out: whole dwords that changed; the dwords that straddle the band's ends bytewise
        const int sft = 8 * c0;
        unsigned nw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) nw[k] = (unsigned)((((unsigned long long)o[k + 1] << 32) | o[k]) >> sft);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (dw + k > last_dw || nw[k] == d[k]) continue;
            const int lo = 4 * (dw + k) - sh;                                // the band byte of the dword's first byte
            if (lo >= 0 && lo + 4 <= len) q[k] = nw[k];
            else {
                uint8_t* bp = reinterpret_cast<uint8_t*>(q + k);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (lo + t >= 0 && lo + t < len) bp[t] = (uint8_t)(nw[k] >> (8 * t));
            }
        }
    }
}

}  // namespace

void launch_heat_walk(const int* frame_off, int n_ticks, const int* rows6, const int* reset, const int* mode, int first, const HeatGeom& g, int* state,
                      int* layers, int cap, int* n_final, int* pending, int* status, int* events, int* row_tags, hipStream_t s) {
    hipLaunchKernelGGL(heat_walk_kernel, dim3(g.streams), dim3(T), 0, s, frame_off, n_ticks, rows6, reset, mode, first, g, state, layers, cap, n_final,
                       pending, status, events, reinterpret_cast<int4*>(row_tags));
    KCHECK();
}

void launch_heat_decay(int* layers, const HeatGeom& g, int stream, int layer_mask, int shift, hipStream_t s) {
    const int cells = g.cells();
    hipLaunchKernelGGL(heat_decay_kernel, dim3((cells + 1023) / 1024, HEAT_LAYERS, stream < 0 ? g.streams : 1), dim3(256), 0, s, layers, cells, stream,
                       g.streams, layer_mask, shift);
    KCHECK();
}

void launch_heat_levels(const int* layers, const HeatGeom& g, int layer, int scale, const int* used, int n_used, int* maxima, uint16_t* levels,
                        hipStream_t s) {
    if (n_used <= 0) return;
    hipLaunchKernelGGL(heat_levels_kernel, dim3(n_used), dim3(1024), 0, s, layers, g.cells(), layer, scale, used, maxima, levels);
    KCHECK();
}

void launch_heat_render(uint8_t* frames, int n_frames, const int* frame_cam, const HeatGeom& g, const int* maxima, const uint16_t* levels,
                        const unsigned* lut, int alpha_q8, int floor, hipStream_t s) {
    if (n_frames <= 0) return;
    const int rows = HT_BAND / (1 << g.lc) + 3;                              // level rows a band can need (at least two)
    const size_t lds = (512 + (size_t)g.gw + ((size_t)rows * g.gw + 1) / 2) * sizeof(unsigned);
    // p / W as the high half of p * ceil(2^32 / W): exact while p (ceil(2^32 / W) W - 2^32) < 2^32, and p < 2^18, W <= 2^14.  W = 1: p itself.
    const unsigned w_magic = g.w > 1 ? (unsigned)(((1ull << 32) + g.w - 1) / g.w) : 0u;
    if (lds > 48 * 1024) set_lds_limit(heat_render_kernel, lds);             // (at most 59 KiB: 4096 cell columns of 4 pixels)
    hipLaunchKernelGGL(heat_render_kernel, dim3((g.h + HT_BAND - 1) / HT_BAND, n_frames), dim3(256), lds, s, frames, frame_cam, g, maxima, levels, lut,
                       alpha_q8, floor, w_magic);
    KCHECK();
}

}  // namespace aic
