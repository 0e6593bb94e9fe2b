// kernels_scene.hip -- the kernels of the scene-watch stage (scene.hpp).  Integer arithmetic only;
// tests/scene_oracle.py is the specification.  No floating point, no scratch.
//
// scene_gray_kernel   the one that reads the frames, every byte once.  The cell rows of all frames of the launch are one flat run of
//                     "units": a unit is 16 bytes of a cell row when the frame base and the pitch 3 w are multiples of 16 (a
//                     global_load_dwordx4 per pixel row of the cell), 4 bytes otherwise (two aligned dwords and an alignbyte: correct
//                     for any base and width).  Lane l of a block takes unit l, so neighbouring lanes read neighbouring bytes.  A cell
//                     row is 3 c bytes per cell -- 3, 6 or 12 dwords -- and a block of 192 lanes covers a whole number of cells.  A
//                     dword of BGR bytes times the weights 29 / 150 / 77 is one v_dot4 with one of three weight words, chosen by the
//                     dword's index mod 3.  Dword sums over the c pixel rows go through LDS to the lane that owns the cell.
// scene_model_kernel  a thread owns one cell of one stream and walks the launch's ticks in order: bg, dev, prev are read once and
//                     written once per launch, the raw / changed / differs-from-prev bits once per tick.
// scene_stats_kernel  stateless per frame: a 16 x 64 tile of cells with a halo of one in LDS, the 3 x 3 vote, the mask, and the
//                     tick's sums by wave shuffles, then LDS, then integer atomics (order-free).
// scene_rows_kernel   one wave per tracker row: the moving share of the cells its box covers.
// scene_walk_kernel   one thread per stream: conditions, alarms and the gate, tick by tick; writes the records.
#include "scene.hpp"
#include "stage_dev.hpp"

namespace aic {

namespace {

// weights of the four bytes of a dword whose first byte is channel p (0 B, 1 G, 2 R), lowest byte first
__device__ __forceinline__ unsigned weight_word(int p) { return p == 0 ? 0x1D4D961Du : p == 1 ? 0x961D4D96u : 0x4D961D4Du; }

__device__ __forceinline__ unsigned dot4(unsigned v, unsigned w, unsigned acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(v, w, acc, false);                         // v_dot4_u32_u8
#else
    return acc + (v & 255u) * (w & 255u) + ((v >> 8) & 255u) * ((w >> 8) & 255u) + ((v >> 16) & 255u) * ((w >> 16) & 255u) + (v >> 24) * (w >> 24);
#endif
}

constexpr int GRAY_T = 192;

// C: cell size; UD: dwords per unit (4: aligned 16-byte loads, 1: any alignment).  units_per_row = wc * 3 C / (4 UD).
template <int C, int UD>
__global__ __launch_bounds__(GRAY_T) void scene_gray_kernel(const uint8_t* __restrict__ frames, ScGeom g, long n_units, int units_per_row,
                                                            long n_cells, uint8_t* __restrict__ gray) {
    constexpr int DPC = 3 * C / 4;                                           // dwords per cell of one pixel row
    constexpr int CELLS = GRAY_T * UD / DPC;                                 // cells per block: 256 UD / C
    constexpr int SHIFT = 8 + (C == 4 ? 4 : C == 8 ? 6 : 8);
    __shared__ unsigned s_sum[GRAY_T * UD];
    const int tid = threadIdx.x;
    const long u = (long)blockIdx.x * GRAY_T + tid;
    unsigned acc[UD];
#pragma unroll
    for (int j = 0; j < UD; ++j) acc[j] = 0;
    if (u < n_units) {
        const long rowid = u / units_per_row;                                // frame * hc + cell row
        const int k = (int)(u - rowid * units_per_row);
        const long f = rowid / g.hc;
        const int cy = (int)(rowid - f * g.hc);
        const size_t pitch = (size_t)g.w * 3;
        const uint8_t* p = frames + ((size_t)f * g.h + (size_t)cy * C) * pitch + (size_t)k * 4 * UD;
        const int ph = (k * UD) % 3;
        if constexpr (UD == 4) {
            const unsigned w0 = weight_word(ph), w1 = weight_word((ph + 1) % 3), w2 = weight_word((ph + 2) % 3);
            uint4 v[C];
#pragma unroll
            for (int r = 0; r < C; ++r) v[r] = *reinterpret_cast<const uint4*>(p + r * pitch);
#pragma unroll
            for (int r = 0; r < C; ++r) {
                acc[0] = dot4(v[r].x, w0, acc[0]);
                acc[1] = dot4(v[r].y, w1, acc[1]);
                acc[2] = dot4(v[r].z, w2, acc[2]);
                acc[3] = dot4(v[r].w, w0, acc[3]);
            }
        } else {
            const unsigned w0 = weight_word(ph);
            unsigned v[C];
#pragma unroll
            for (int r = 0; r < C; ++r) {                                    // both aligned words hold a byte of the dword: no stray page
                const uintptr_t a = reinterpret_cast<uintptr_t>(p + r * pitch);
                const unsigned sh = (unsigned)(a & 3);
                const unsigned* q = reinterpret_cast<const unsigned*>(a - sh);
                const unsigned lo = q[0], hi = sh ? q[1] : 0u;
                v[r] = __builtin_amdgcn_alignbyte(hi, lo, sh);
            }
#pragma unroll
            for (int r = 0; r < C; ++r) acc[0] = dot4(v[r], w0, acc[0]);
        }
    }
#pragma unroll
    for (int j = 0; j < UD; ++j) s_sum[tid * UD + j] = acc[j];
    __syncthreads();
    for (int i = tid; i < CELLS; i += GRAY_T) {
        const long cell = (long)blockIdx.x * CELLS + i;
        if (cell >= n_cells) break;
        unsigned t = 0;
#pragma unroll
        for (int j = 0; j < DPC; ++j) t += s_sum[i * DPC + j];
        gray[cell] = (uint8_t)(t >> SHIFT);
    }
}

__global__ __launch_bounds__(256) void scene_model_kernel(const uint8_t* __restrict__ gray, int n_ticks, ScGeom g, ScOpts o,
                                                          const int* __restrict__ scalars, const int* __restrict__ reset, int first,
                                                          uint16_t* __restrict__ bg_all, uint16_t* __restrict__ dev_all,
                                                          uint8_t* __restrict__ prev_all, uint8_t* __restrict__ bits) {
    const size_t ncell = (size_t)g.hc * g.wc;
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (cell >= ncell) return;
    int age = (first && reset[s]) ? 0 : scalars[s * SC_S_INTS + SC_S_AGE];
    const size_t si = (size_t)s * ncell + cell;
    int bg = bg_all[si], dv = dev_all[si], prev = prev_all[si];
    const int thresh_q8 = o.thresh << 8, big_q8 = o.big_thresh << 8;
    for (int k = 0; k < n_ticks; ++k) {
        const size_t x = ((size_t)k * g.streams + s) * ncell + cell;
        const int gv = gray[x], g256 = gv << 8;
        int b = gv != prev ? SC_B_DIFF : 0;
        if (age == 0) {
            bg = g256, dv = o.dev_init_q8;
        } else {
            const int diff = g256 - bg, d = diff < 0 ? -diff : diff;
            const int thr = imax(thresh_q8, (dv * o.noise_k_q4) >> 4);
            const bool warm = age >= o.warmup, raw = warm && d > thr;
            if (raw) b |= SC_B_RAW;
            if (warm && d > big_q8) b |= SC_B_CHANGED;
            const int a = o.learn_shift + (raw ? o.slow_extra : 0);
            bg += diff >> a;                                                 // >> of a negative int is a floor shift here
            dv += (d - dv) >> a;
        }
        bits[x] = (uint8_t)b;
        prev = gv;
        age = imin(age + 1, SC_SAT);
    }
    bg_all[si] = (uint16_t)bg, dev_all[si] = (uint16_t)dv, prev_all[si] = (uint8_t)prev;
}

constexpr int TILE_W = 64, TILE_H = 16, HALO_W = TILE_W + 2, HALO_H = TILE_H + 2;

__global__ __launch_bounds__(256) void scene_stats_kernel(const uint8_t* __restrict__ gray, const uint8_t* __restrict__ bits, ScGeom g,
                                                          int min_neighbours, int tiles_x, int tiles, uint8_t* __restrict__ mask,
                                                          int* __restrict__ acc_all) {
    __shared__ uint8_t s_b[HALO_H][HALO_W + 2];
    __shared__ uint8_t s_g[HALO_H][HALO_W + 2];
    __shared__ int s_red[4][10];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t x = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, tx0 = (tile % tiles_x) * TILE_W, ty0 = (tile / tiles_x) * TILE_H;
    const size_t base = x * g.hc * g.wc;
    for (int i = tid; i < HALO_H * HALO_W; i += 256) {
        const int ly = i / HALO_W, lx = i - ly * HALO_W, gy = ty0 + ly - 1, gx = tx0 + lx - 1;
        const bool in = gy >= 0 && gy < g.hc && gx >= 0 && gx < g.wc;
        const size_t at = base + (size_t)(in ? gy : 0) * g.wc + (in ? gx : 0);
        s_b[ly][lx] = in ? bits[at] : 0;
        s_g[ly][lx] = in ? gray[at] : 0;
    }
    __syncthreads();
    int n_raw = 0, n_mov = 0, n_chg = 0, n_diff = 0, sg = 0, ssh = 0, x0e = 0, y0e = 0, x1e = 0, y1e = 0;
#pragma unroll
    for (int j = 0; j < TILE_H / 4; ++j) {
        const int ly = wv + 4 * j + 1, lx = lane + 1, gy = ty0 + ly - 1, gx = tx0 + lx - 1;
        if (gy >= g.hc || gx >= g.wc) continue;
        const int b = s_b[ly][lx], raw = b & SC_B_RAW;
        int cnt = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) cnt += s_b[ly + dy][lx + dx] & SC_B_RAW;
        const int clean = raw && cnt >= min_neighbours;
        mask[base + (size_t)gy * g.wc + gx] = (uint8_t)((clean ? SC_M_CLEAN : 0) | (raw ? SC_M_RAW : 0));
        n_raw += raw, n_mov += clean, n_chg += (b & SC_B_CHANGED) != 0, n_diff += (b & SC_B_DIFF) != 0;
        const int gv = s_g[ly][lx];
        sg += gv;
        if (gy >= 1 && gy < g.hc - 1 && gx >= 1 && gx < g.wc - 1) {
            const int lap = 4 * gv - s_g[ly - 1][lx] - s_g[ly + 1][lx] - s_g[ly][lx - 1] - s_g[ly][lx + 1];
            ssh += lap < 0 ? -lap : lap;
        }
        if (clean) x0e = imax(x0e, 65536 - gx), y0e = imax(y0e, 65536 - gy), x1e = imax(x1e, gx + 1), y1e = imax(y1e, gy + 1);
    }
    n_raw = wave_sum(n_raw), n_mov = wave_sum(n_mov), n_chg = wave_sum(n_chg), n_diff = wave_sum(n_diff), sg = wave_sum(sg), ssh = wave_sum(ssh);
    x0e = wave_max(x0e), y0e = wave_max(y0e), x1e = wave_max(x1e), y1e = wave_max(y1e);
    if (lane == 0) {
        int* r = s_red[wv];
        r[0] = n_raw, r[1] = n_mov, r[2] = n_chg, r[3] = n_diff, r[4] = sg, r[5] = ssh, r[6] = x0e, r[7] = y0e, r[8] = x1e, r[9] = y1e;
    }
    __syncthreads();
    if (tid < 10) {
        int v = 0;
        for (int w = 0; w < 4; ++w) v = tid < 6 ? v + s_red[w][tid] : imax(v, s_red[w][tid]);
        int* acc = acc_all + x * SC_A_INTS;
        if (v) {
            if (tid < 4) atomicAdd(acc + tid, v);                            // SC_A_RAW, MOVING, CHANGED, DIFF
            else if (tid == 4) atomicAdd(reinterpret_cast<unsigned long long*>(acc + SC_A_SUM_G), (unsigned long long)v);
            else if (tid == 5) atomicAdd(reinterpret_cast<unsigned long long*>(acc + SC_A_SUM_SHARP), (unsigned long long)v);
            else atomicMax(acc + SC_A_X0 + (tid - 6), v);
        }
    }
}

__global__ __launch_bounds__(256) void scene_rows_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ frame_off, int row_blocks,
                                                         const int* __restrict__ rows6, ScGeom g, int* __restrict__ row_motion) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t x = blockIdx.x / row_blocks;
    const int r = (blockIdx.x % row_blocks) * 4 + wv;
    const int off = frame_off[x], n = frame_off[x + 1] - off;
    if (r >= n) return;
    const int* row = rows6 + (size_t)(off + r) * 6;
    const int x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3];
    int out = -1;
    const bool valid = row_valid(x1, y1, x2, y2, SC_COORD_MAX);
    const int X0 = imax(x1, 0), Y0 = imax(y1, 0), X1 = imin(x2, g.wc * g.c - 1), Y1 = imin(y2, g.hc * g.c - 1);
    if (valid && X1 >= X0 && Y1 >= Y0) {
        const int cx0 = X0 / g.c, cy0 = Y0 / g.c, cw = X1 / g.c - cx0 + 1, ch = Y1 / g.c - cy0 + 1, covered = cw * ch;
        const uint8_t* m = mask + x * g.hc * g.wc;
        int moving = 0;
        for (int i = lane; i < covered; i += 64) {
            const int yy = i / cw, xx = i - yy * cw;
            moving += m[(size_t)(cy0 + yy) * g.wc + cx0 + xx] & SC_M_CLEAN;
        }
        moving = wave_sum(moving);
        out = (int)(256ll * moving / covered);
    }
    if (lane == 0) row_motion[off + r] = out;
}

__global__ __launch_bounds__(64) void scene_walk_kernel(const int* __restrict__ acc_all, int n_ticks, ScGeom g, ScOpts o,
                                                        const int* __restrict__ reset, int first, int* __restrict__ scalars,
                                                        int* __restrict__ records) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= g.streams) return;
    int* sc = scalars + s * SC_S_INTS;
    const bool fresh = first && reset[s];
    int age = fresh ? 0 : sc[SC_S_AGE], quiet = fresh ? 0 : sc[SC_S_QUIET], ref = fresh ? 0 : sc[SC_S_REF], alarm = fresh ? 0 : sc[SC_S_ALARM];
    int on[SC_KINDS], off[SC_KINDS];
#pragma unroll
    for (int k = 0; k < SC_KINDS; ++k) on[k] = fresh ? 0 : sc[SC_S_ON + k], off[k] = fresh ? 0 : sc[SC_S_OFF + k];
    const long long ncell = (long long)g.hc * g.wc;
    const long long n_int = g.hc >= 3 && g.wc >= 3 ? (long long)(g.hc - 2) * (g.wc - 2) : 0;
    for (int t = 0; t < n_ticks; ++t) {
        const size_t x = (size_t)t * g.streams + s;
        const int* a = acc_all + x * SC_A_INTS;
        const int n_raw = a[SC_A_RAW], n_mov = a[SC_A_MOVING], n_chg = a[SC_A_CHANGED], n_diff = a[SC_A_DIFF];
        const unsigned long long sum_g = *reinterpret_cast<const unsigned long long*>(a + SC_A_SUM_G);
        const unsigned long long sum_sh = *reinterpret_cast<const unsigned long long*>(a + SC_A_SUM_SHARP);
        const int mean = (int)(sum_g / (unsigned long long)ncell);
        const int sharp = n_int ? (int)(sum_sh / (unsigned long long)n_int) : 0;
        const bool ready = age >= o.warmup;
        if (age == 0) ref = sharp << 8;
        int cond = 0;
        if (ready) {
            if (mean < o.dark_luma) cond |= SC_DARK;
            if (mean > o.bright_luma) cond |= SC_BRIGHT;
            if (ref >= o.min_ref_q8 && ((long long)sharp << 16) < (long long)ref * o.defocus_q8) cond |= SC_DEFOCUS;
            if ((long long)n_chg * 65536 > (long long)o.scene_q16 * ncell) cond |= SC_SCENE;
            if (n_diff == 0) cond |= SC_FROZEN;
        }
        if (!ready || !(cond & SC_DEFOCUS)) ref += ((sharp << 8) - ref) >> o.ref_shift;
        int edges = 0;
#pragma unroll
        for (int k = 0; k < SC_KINDS; ++k) {
            if (cond >> k & 1) on[k] = imin(on[k] + 1, SC_SAT), off[k] = 0;
            else off[k] = imin(off[k] + 1, SC_SAT), on[k] = 0;
            if (!(alarm >> k & 1) && on[k] >= o.hold) alarm |= 1 << k, edges |= 1 << k;
            else if ((alarm >> k & 1) && off[k] >= o.hold) alarm &= ~(1 << k), edges |= 1 << (8 + k);
        }
        quiet = n_mov >= o.gate_cells ? 0 : imin(quiet + 1, SC_SAT);
        const int active = !ready || quiet <= o.gate_hold;
        int4* rec = reinterpret_cast<int4*>(records + x * SC_RECORD_INTS);
        const bool box = n_mov > 0;
        rec[0] = make_int4(age, ready, active, n_mov);
        rec[1] = make_int4(n_raw, box ? (65536 - a[SC_A_X0]) * g.c : -1, box ? (65536 - a[SC_A_Y0]) * g.c : -1, box ? a[SC_A_X1] * g.c : -1);
        rec[2] = make_int4(box ? a[SC_A_Y1] * g.c : -1, mean, sharp, ref);
        rec[3] = make_int4(n_chg, cond, alarm, edges);
        age = imin(age + 1, SC_SAT);
    }
    sc[SC_S_AGE] = age, sc[SC_S_QUIET] = quiet, sc[SC_S_REF] = ref, sc[SC_S_ALARM] = alarm;
#pragma unroll
    for (int k = 0; k < SC_KINDS; ++k) sc[SC_S_ON + k] = on[k], sc[SC_S_OFF + k] = off[k];
    sc[14] = sc[15] = 0;
}

template <int C>
void gray_for(const uint8_t* frames, int n_frames, const ScGeom& g, uint8_t* gray, hipStream_t s) {
    const bool aligned = reinterpret_cast<uintptr_t>(frames) % 16 == 0 && g.w % 16 == 0;
    const long n_cells = (long)n_frames * g.hc * g.wc;
    constexpr int DPC = 3 * C / 4;
    if (aligned) {                                                           // wc * C == w: a cell row is 3 w / 16 units
        const int upr = g.wc * DPC / 4;
        const long n_units = (long)n_frames * g.hc * upr;
        hipLaunchKernelGGL((scene_gray_kernel<C, 4>), dim3((unsigned)((n_units + GRAY_T - 1) / GRAY_T)), dim3(GRAY_T), 0, s, frames, g, n_units, upr,
                           n_cells, gray);
    } else {
        const int upr = g.wc * DPC;
        const long n_units = (long)n_frames * g.hc * upr;
        hipLaunchKernelGGL((scene_gray_kernel<C, 1>), dim3((unsigned)((n_units + GRAY_T - 1) / GRAY_T)), dim3(GRAY_T), 0, s, frames, g, n_units, upr,
                           n_cells, gray);
    }
    KCHECK();
}

}  // namespace

void launch_scene_gray(const uint8_t* frames, int n_frames, const ScGeom& g, uint8_t* gray, hipStream_t s) {
    if (g.c == 4) gray_for<4>(frames, n_frames, g, gray, s);
    else if (g.c == 8) gray_for<8>(frames, n_frames, g, gray, s);
    else gray_for<16>(frames, n_frames, g, gray, s);
}

void launch_scene_model(const uint8_t* gray, int n_ticks, const ScGeom& g, const ScOpts& o, const int* scalars, const int* reset, int first,
                        uint16_t* bg, uint16_t* dev, uint8_t* prev, uint8_t* bits, hipStream_t s) {
    const size_t ncell = (size_t)g.hc * g.wc;
    hipLaunchKernelGGL(scene_model_kernel, dim3((unsigned)((ncell + 255) / 256), g.streams), dim3(256), 0, s, gray, n_ticks, g, o, scalars, reset, first,
                       bg, dev, prev, bits);
    KCHECK();
}

void launch_scene_stats(const uint8_t* gray, const uint8_t* bits, int n_frames, const ScGeom& g, const ScOpts& o, uint8_t* mask, int* acc,
                        hipStream_t s) {
    const int tiles_x = ceil_div(g.wc, TILE_W), tiles = tiles_x * ceil_div(g.hc, TILE_H);
    hipLaunchKernelGGL(scene_stats_kernel, dim3((unsigned)((size_t)n_frames * tiles)), dim3(256), 0, s, gray, bits, g, o.min_neighbours, tiles_x, tiles,
                       mask, acc);
    KCHECK();
}

void launch_scene_rows(const uint8_t* mask, const int* frame_off, int n_frames, int max_rows, const int* rows6, const ScGeom& g, int* row_motion,
                       hipStream_t s) {
    if (max_rows == 0) return;
    const int row_blocks = ceil_div(max_rows, 4);
    hipLaunchKernelGGL(scene_rows_kernel, dim3((unsigned)((size_t)n_frames * row_blocks)), dim3(256), 0, s, mask, frame_off, row_blocks, rows6, g,
                       row_motion);
    KCHECK();
}

void launch_scene_walk(const int* acc, int n_ticks, const ScGeom& g, const ScOpts& o, const int* reset, int first, int* scalars, int* records,
                       hipStream_t s) {
    hipLaunchKernelGGL(scene_walk_kernel, dim3(ceil_div(g.streams, 64)), dim3(64), 0, s, acc, n_ticks, g, o, reset, first, scalars, records);
    KCHECK();
}

}  // namespace aic
