// kernels_left.hip -- the kernels of the left-objects stage (left.hpp).  Integer arithmetic only;
// tests/left_oracle.py is the specification.  No floating point, no scratch.  The gray grid is launch_scene_gray's (kernels_scene.hip).
//
// left_occupancy_kernel  one wave per tracker row: the cells its padded box covers, strided over the lanes, get occ = 1 and
//                        atomicMin(occ_id, id) -- commutative, so free of row order.
// left_model_kernel      a thread owns one cell of one stream and walks the launch's ticks in order: fast, slow, still, last_id and
//                        last_tick are read once and written once per launch; per tick it writes cand, slow >> 8 and, for a candidate
//                        cell, the owner's tick (-1 when outside owner_window) and id.
// left_blobs_kernel      one block per frame.  The u16 labels of the whole grid sit in LDS (cell index + 1, 0 = no candidate).  A sweep
//                        gives every cell the least label among itself and its 8 neighbours and then follows that label's own cell
//                        down (a label names a cell of the same blob whose label is no greater: the chain shortcut that lets a spiral
//                        settle in a few sweeps); sweeps repeat until a block-wide flag stays clear.  Every label only ever decreases
//                        and always names a cell of its own blob, so the racing LDS reads are harmless and the fixed point is the
//                        blob's smallest cell index.  Then: areas by LDS atomics on packed u16 pairs, an ordered compaction of the
//                        roots of a kept size (first 64, in label order), and one pass of per-blob reductions (box, c_now, c_bg by
//                        integer LDS atomics, the owner by max tick, then min cell).
// left_walk_kernel       one thread per stream: matching, slots, alarms and events, tick by tick; writes records, objects, events.
// left_events_kernel     one block: packs the per-frame event lists of a launch in frame order behind the call's earlier ones.
#include "left.hpp"
#include "stage_dev.hpp"

namespace aic {

namespace {

__device__ __forceinline__ int iabs(int a) { return a < 0 ? -a : a; }

__global__ __launch_bounds__(256) void left_occupancy_kernel(const int* __restrict__ frame_off, int row_blocks, const int* __restrict__ rows6, ScGeom g,
                                                             int pad, uint8_t* __restrict__ occ, int* __restrict__ occ_id) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t x = blockIdx.x / row_blocks;
    const int r = (blockIdx.x % row_blocks) * 4 + wv;
    const int off = frame_off[x], n = frame_off[x + 1] - off;
    if (r >= n) return;
    const int* row = rows6 + (size_t)(off + r) * 6;
    const int x1 = row[0], y1 = row[1], x2 = row[2], y2 = row[3], id = row[4];
    const bool valid = row_valid(x1, y1, x2, y2, SC_COORD_MAX);
    const int X0 = imax(x1, 0), Y0 = imax(y1, 0), X1 = imin(x2, g.wc * g.c - 1), Y1 = imin(y2, g.hc * g.c - 1);
    if (!valid || X1 < X0 || Y1 < Y0) return;
    const int cx0 = imax(X0 / g.c - pad, 0), cy0 = imax(Y0 / g.c - pad, 0), cx1 = imin(X1 / g.c + pad, g.wc - 1), cy1 = imin(Y1 / g.c + pad, g.hc - 1);
    const int cw = cx1 - cx0 + 1, covered = cw * (cy1 - cy0 + 1);
    const size_t base = x * g.hc * g.wc;
    for (int i = lane; i < covered; i += 64) {
        const int yy = i / cw, xx = i - yy * cw;
        const size_t at = base + (size_t)(cy0 + yy) * g.wc + cx0 + xx;
        occ[at] = 1;
        atomicMin(occ_id + at, id);
    }
}

__global__ __launch_bounds__(256) void left_model_kernel(LfFrames fr, int n_ticks, ScGeom g, LfOpts o, const int* __restrict__ scalars,
                                                         const int* __restrict__ reset, int first, LfCells cs) {
    const size_t ncell = (size_t)g.hc * g.wc;
    const size_t cell = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (cell >= ncell) return;
    int age = (first && reset[s]) ? 0 : scalars[s * LF_S_INTS + LF_S_AGE];
    const size_t si = (size_t)s * ncell + cell;
    int fast = cs.fast[si], slow = cs.slow[si], still = cs.still[si], last_id = cs.last_id[si], last_tick = cs.last_tick[si];
    const int t_q8 = o.thresh << 8;
    for (int k = 0; k < n_ticks; ++k) {
        const size_t x = ((size_t)k * g.streams + s) * ncell + cell;
        const int g256 = (int)fr.gray[x] << 8;
        int cand = 0;
        if (age == 0) {
            fast = slow = g256, still = 0, last_id = -1, last_tick = -1;
        } else {
            const int df = iabs(g256 - fast), ds = iabs(g256 - slow);
            fast += (g256 - fast) >> o.fast_shift;                           // >> of a negative int is a floor shift here
            const bool ready = age >= o.warmup, stable = df <= t_q8, differs = ds > t_q8;
            if (fr.occ[x]) {
                last_id = fr.occ_id[x], last_tick = age;
            } else {
                if (ready && stable) still = differs ? imin(still + 1, 65535) : 0;
                else still = imax(still - o.decay, 0);
                if (still == 0) slow += (g256 - slow) >> (ready ? o.slow_shift : o.fast_shift);
            }
            if (still >= o.absorb_ticks) fast = slow = g256, still = 0;
            cand = still >= o.min_ticks;
        }
        fr.cand[x] = (uint8_t)cand;
        fr.slow8[x] = (uint8_t)(slow >> 8);
        if (cand) {
            fr.own_tick[x] = (last_tick >= 0 && age - last_tick <= o.owner_window) ? last_tick : -1;
            fr.own_id[x] = last_id;
        }
        age = imin(age + 1, SC_SAT);
    }
    cs.fast[si] = (uint16_t)fast, cs.slow[si] = (uint16_t)slow, cs.still[si] = (uint16_t)still, cs.last_id[si] = last_id, cs.last_tick[si] = last_tick;
}

constexpr int BLOB_T = 256;

// |4 v - N - S - E - W| of cell (y, x) on a u8 grid; a neighbour outside the grid is the cell's own value
__device__ __forceinline__ int contrast_at(const uint8_t* __restrict__ v, int y, int x, int hc, int wc) {
    const int c = v[y * wc + x];
    const int n = y > 0 ? v[(y - 1) * wc + x] : c, s = y < hc - 1 ? v[(y + 1) * wc + x] : c;
    const int w = x > 0 ? v[y * wc + x - 1] : c, e = x < wc - 1 ? v[y * wc + x + 1] : c;
    return iabs(4 * c - n - s - e - w);
}

__global__ __launch_bounds__(BLOB_T) void left_blobs_kernel(LfFrames fr, ScGeom g, int min_cells, int max_cells, int* __restrict__ head_all,
                                                            int* __restrict__ blobs_all, int* __restrict__ labels) {
    extern __shared__ __attribute__((aligned(16))) unsigned dyn[];
    __shared__ int s_tab[LF_BLOBS_MAX][LF_BLOB_INTS];
    __shared__ int s_best_tick[LF_BLOBS_MAX], s_best_cell[LF_BLOBS_MAX];
    __shared__ int s_scan[BLOB_T];
    __shared__ int s_changed, s_ncand;
    const int tid = threadIdx.x, hc = g.hc, wc = g.wc, ncell = hc * wc, pairs = (ncell + 1) >> 1;
    uint16_t* lab = reinterpret_cast<uint16_t*>(dyn);                        // [2 pairs] cell index + 1 of the least cell known, 0 = no candidate
    unsigned* aux32 = dyn + pairs;                                           // [pairs] two u16 per word: a root's area, later its blob index + 1
    uint16_t* aux16 = reinterpret_cast<uint16_t*>(aux32);
    const size_t base = (size_t)blockIdx.x * ncell;
    const uint8_t* cand = fr.cand + base;

    int nc = 0;
    for (int i = tid; i < ncell; i += BLOB_T) {
        const int c = cand[i] != 0;
        lab[i] = (uint16_t)(c ? i + 1 : 0);
        nc += c;
    }
    for (int i = tid; i < pairs; i += BLOB_T) aux32[i] = 0;
    if (tid < LF_BLOBS_MAX) {
        int* t = s_tab[tid];
        t[LF_B_AREA] = 0, t[LF_B_X0] = LF_NONE, t[LF_B_Y0] = LF_NONE, t[LF_B_X1] = -1, t[LF_B_Y1] = -1, t[LF_B_CNOW] = 0, t[LF_B_CBG] = 0, t[LF_B_OWNER] = -1;
        s_best_tick[tid] = -1, s_best_cell[tid] = LF_NONE;
    }
    if (tid == 0) s_ncand = 0;
    __syncthreads();
    nc = wave_sum(nc);
    if ((tid & 63) == 0 && nc) atomicAdd(&s_ncand, nc);

    // ---- labels: sweeps until nothing changes
    for (;;) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        int any = 0;
        for (int i = tid; i < ncell; i += BLOB_T) {
            const int mine = lab[i];
            if (!mine) continue;
            const int y = i / wc, x = i - y * wc;
            int m = mine;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= hc) continue;
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= wc || (dy == 0 && dx == 0)) continue;
                    const int v = lab[yy * wc + xx];
                    if (v && v < m) m = v;
                }
            }
            for (;;) {                                                       // the label's own cell may know a smaller one: follow it down
                const int v = lab[m - 1];
                if (v >= m || v == 0) break;
                m = v;
            }
            if (m < mine) lab[i] = (uint16_t)m, any = 1;
        }
        if (any) s_changed = 1;
        __syncthreads();
        const int again = s_changed;
        __syncthreads();
        if (!again) break;
    }

    // ---- areas: a root's count in its own u16 (at most 32768, so the low half never carries into the high one)
    for (int i = tid; i < ncell; i += BLOB_T) {
        const int l = lab[i];
        if (labels) labels[base + i] = l - 1;
        if (l) atomicAdd(&aux32[(l - 1) >> 1], ((l - 1) & 1) ? 0x10000u : 1u);
    }
    __syncthreads();

    // ---- the roots of a kept size, numbered in label order: each thread owns a run of cells
    const int per = (ncell + BLOB_T - 1) / BLOB_T, lo = imin(tid * per, ncell), hi = imin(lo + per, ncell);
    int cnt = 0;
    for (int i = lo; i < hi; ++i) {
        const int a = aux16[i];
        cnt += lab[i] == i + 1 && a >= min_cells && a <= max_cells;
    }
    s_scan[tid] = cnt;
    __syncthreads();
    for (int d = 1; d < BLOB_T; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int idx = s_scan[tid] - cnt;
    const int kept = s_scan[BLOB_T - 1];
    for (int i = lo; i < hi; ++i) {
        if (lab[i] != i + 1) continue;
        const int a = aux16[i];
        int slot = 0;
        if (a >= min_cells && a <= max_cells) {
            if (idx < LF_BLOBS_MAX) s_tab[idx][LF_B_AREA] = a, slot = idx + 1;
            ++idx;
        }
        aux16[i] = (uint16_t)slot;                                           // only this thread reads or writes a root of its run
    }
    __syncthreads();

    // ---- per-blob reductions
    const int n_blobs = imin(kept, LF_BLOBS_MAX);
    if (n_blobs) {
        const uint8_t* gray = fr.gray + base;
        const uint8_t* slow8 = fr.slow8 + base;
        for (int i = tid; i < ncell; i += BLOB_T) {
            const int l = lab[i];
            const int b = l ? (int)aux16[l - 1] - 1 : -1;
            if (b < 0) continue;
            const int y = i / wc, x = i - y * wc;
            int* t = s_tab[b];
            atomicMin(&t[LF_B_X0], x), atomicMin(&t[LF_B_Y0], y), atomicMax(&t[LF_B_X1], x), atomicMax(&t[LF_B_Y1], y);
            atomicAdd(&t[LF_B_CNOW], contrast_at(gray, y, x, hc, wc));
            atomicAdd(&t[LF_B_CBG], contrast_at(slow8, y, x, hc, wc));
            const int tk = fr.own_tick[base + i];
            if (tk >= 0) atomicMax(&s_best_tick[b], tk);
        }
        __syncthreads();
        for (int i = tid; i < ncell; i += BLOB_T) {
            const int l = lab[i];
            const int b = l ? (int)aux16[l - 1] - 1 : -1;
            if (b < 0) continue;
            const int tk = fr.own_tick[base + i];
            if (tk >= 0 && tk == s_best_tick[b]) atomicMin(&s_best_cell[b], i);
        }
        __syncthreads();
        if (tid < n_blobs) {
            int* out = blobs_all + ((size_t)blockIdx.x * LF_BLOBS_MAX + tid) * LF_BLOB_INTS;
            const int* t = s_tab[tid];
#pragma unroll
            for (int k = 0; k < LF_B_OWNER; ++k) out[k] = t[k];
            out[LF_B_OWNER] = s_best_cell[tid] != LF_NONE ? fr.own_id[base + s_best_cell[tid]] : -1;
        }
    }
    if (tid == 0) {
        int* h = head_all + (size_t)blockIdx.x * LF_HEAD_INTS;
        h[LF_H_CAND] = s_ncand, h[LF_H_KEPT] = kept, h[2] = 0, h[3] = 0;
    }
}

__device__ __forceinline__ void put_event(int* __restrict__ e, int tick, int s, int type, const int* __restrict__ sl, int c, int age) {
    e[0] = tick, e[1] = s, e[2] = type, e[3] = sl[LF_O_UID], e[4] = sl[LF_O_KIND];
    e[5] = sl[LF_O_X0] * c, e[6] = sl[LF_O_Y0] * c, e[7] = (sl[LF_O_X1] + 1) * c, e[8] = (sl[LF_O_Y1] + 1) * c;
    e[9] = sl[LF_O_OWNER], e[10] = sl[LF_O_AREA], e[11] = age;
}

__global__ __launch_bounds__(64) void left_walk_kernel(const int* __restrict__ head_all, const int* __restrict__ blobs_all, int n_ticks, int tick0,
                                                       ScGeom g, LfOpts o, int M, const int* __restrict__ reset, int first, int* __restrict__ scalars,
                                                       int* __restrict__ slots_all, int* __restrict__ records, int* __restrict__ objects,
                                                       int* __restrict__ ev_count, int* __restrict__ ev_all) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= g.streams) return;
    int* sc = scalars + s * LF_S_INTS;
    int* slots = slots_all + (size_t)s * M * LF_OBJECT_INTS;
    const bool fresh = first && reset[s];
    int age = fresh ? 0 : sc[LF_S_AGE], uids = fresh ? 0 : sc[LF_S_UIDS];
    if (fresh)
        for (int i = 0; i < M * LF_OBJECT_INTS; ++i) slots[i] = 0;
    for (int t = 0; t < n_ticks; ++t) {
        const size_t x = (size_t)t * g.streams + s;
        const int* h = head_all + x * LF_HEAD_INTS;
        const int* blobs = blobs_all + x * LF_BLOBS_MAX * LF_BLOB_INTS;
        int* ev = ev_all + x * 2 * M * LF_EVENT_INTS;
        const int kept = h[LF_H_KEPT], nb = imin(kept, LF_BLOBS_MAX);
        const bool ready = age >= o.warmup;
        int flags = kept > LF_BLOBS_MAX ? 1 : 0, dropped = 0, n_ev = 0;
        if (ready) {
            unsigned long long taken = 0, appeared = 0, raised = 0;
            for (int b = 0; b < nb; ++b) {
                const int* bl = blobs + b * LF_BLOB_INTS;
                const int bx0 = bl[LF_B_X0], by0 = bl[LF_B_Y0], bx1 = bl[LF_B_X1], by1 = bl[LF_B_Y1];
                int best = -1, best_a = 0, free_slot = -1;
                for (int j = 0; j < M; ++j) {
                    const int* sl = slots + j * LF_OBJECT_INTS;
                    if (sl[LF_O_UID] == 0) {
                        if (free_slot < 0) free_slot = j;
                        continue;
                    }
                    if (taken >> j & 1) continue;
                    const int w = imin(bx1, sl[LF_O_X1]) - imax(bx0, sl[LF_O_X0]) + 1, hh = imin(by1, sl[LF_O_Y1]) - imax(by0, sl[LF_O_Y0]) + 1;
                    const int a = w > 0 && hh > 0 ? w * hh : 0;
                    if (a > best_a) best_a = a, best = j;
                }
                int j = best;
                if (j >= 0) {
                    int* sl = slots + j * LF_OBJECT_INTS;
                    sl[LF_O_MISSING] = 0, sl[LF_O_SEEN] += 1;
                } else if (free_slot >= 0) {
                    j = free_slot;
                    int* sl = slots + j * LF_OBJECT_INTS;
                    sl[LF_O_UID] = ++uids, sl[LF_O_KIND] = 0, sl[LF_O_ALARMED] = 0, sl[LF_O_OWNER] = bl[LF_B_OWNER], sl[LF_O_BORN] = age;
                    sl[LF_O_SEEN] = 1, sl[LF_O_MISSING] = 0;
                    appeared |= 1ull << j;
                } else {
                    ++dropped;
                    continue;
                }
                int* sl = slots + j * LF_OBJECT_INTS;
                sl[LF_O_X0] = bx0, sl[LF_O_Y0] = by0, sl[LF_O_X1] = bx1, sl[LF_O_Y1] = by1, sl[LF_O_AREA] = bl[LF_B_AREA];
                taken |= 1ull << j;
                if (sl[LF_O_SEEN] == o.alarm_hold) {
                    sl[LF_O_ALARMED] = 1, sl[LF_O_KIND] = bl[LF_B_CNOW] >= bl[LF_B_CBG] ? LF_KIND_LEFT : LF_KIND_REMOVED;
                    raised |= 1ull << j;
                }
            }
            for (int j = 0; j < M; ++j) {                                    // events in slot order; an unmatched slot goes missing
                int* sl = slots + j * LF_OBJECT_INTS;
                if (sl[LF_O_UID] == 0) continue;
                if (appeared >> j & 1) put_event(ev + (n_ev++) * LF_EVENT_INTS, tick0 + t, s, LF_APPEARED, sl, g.c, age);
                if (raised >> j & 1) put_event(ev + (n_ev++) * LF_EVENT_INTS, tick0 + t, s, LF_RAISED, sl, g.c, age);
                if (!(taken >> j & 1)) {
                    sl[LF_O_MISSING] += 1;
                    if (sl[LF_O_MISSING] > o.gone_ticks) {
                        put_event(ev + (n_ev++) * LF_EVENT_INTS, tick0 + t, s, LF_ENDED, sl, g.c, age);
                        for (int k = 0; k < LF_OBJECT_INTS; ++k) sl[k] = 0;
                    }
                }
            }
            if (dropped) flags |= 2;
        }
        ev_count[x] = n_ev;
        int live = 0, alarmed = 0;
        int* obj = objects + x * M * LF_OBJECT_INTS;
        for (int j = 0; j < M; ++j) {
            const int* sl = slots + j * LF_OBJECT_INTS;
            int* ob = obj + j * LF_OBJECT_INTS;
            const bool on = sl[LF_O_UID] != 0;
            live += on, alarmed += on && sl[LF_O_ALARMED];
            for (int k = 0; k < LF_OBJECT_INTS; ++k) ob[k] = sl[k];
            if (on) ob[LF_O_X0] = sl[LF_O_X0] * g.c, ob[LF_O_Y0] = sl[LF_O_Y0] * g.c, ob[LF_O_X1] = (sl[LF_O_X1] + 1) * g.c, ob[LF_O_Y1] = (sl[LF_O_Y1] + 1) * g.c;
        }
        int4* rec = reinterpret_cast<int4*>(records + x * LF_RECORD_INTS);
        rec[0] = make_int4(age, ready, h[LF_H_CAND], nb);
        rec[1] = make_int4(live, alarmed, flags, dropped);
        age = imin(age + 1, SC_SAT);
    }
    sc[LF_S_AGE] = age, sc[LF_S_UIDS] = uids, sc[2] = sc[3] = 0;
}

__global__ __launch_bounds__(256) void left_events_kernel(const int* __restrict__ ev_count, const int* __restrict__ ev_all, int n_frames, int M, int cap,
                                                          int* __restrict__ out, int* __restrict__ total) {
    int at = *total;                                                         // every thread keeps the running count itself
    for (int f = 0; f < n_frames; ++f) {
        const int n = ev_count[f];
        const int room = imax(imin(n, cap - at), 0);
        const int* src = ev_all + (size_t)f * 2 * M * LF_EVENT_INTS;
        for (int i = threadIdx.x; i < room * LF_EVENT_INTS; i += 256) out[(size_t)at * LF_EVENT_INTS + i] = src[i];
        at += n;
    }
    __syncthreads();                                                         // all have read *total
    if (threadIdx.x == 0) *total = at;
}

}  // namespace

void launch_left_occupancy(const int* frame_off, int n_frames, int max_rows, const int* rows6, const ScGeom& g, int pad_cells, uint8_t* occ,
                           int* occ_id, hipStream_t s) {
    if (max_rows == 0) return;
    const int row_blocks = ceil_div(max_rows, 4);
    hipLaunchKernelGGL(left_occupancy_kernel, dim3((unsigned)((size_t)n_frames * row_blocks)), dim3(256), 0, s, frame_off, row_blocks, rows6, g, pad_cells,
                       occ, occ_id);
    KCHECK();
}

void launch_left_model(const LfFrames& fr, int n_ticks, const ScGeom& g, const LfOpts& o, const int* scalars, const int* reset, int first,
                       const LfCells& cells, hipStream_t s) {
    const size_t ncell = (size_t)g.hc * g.wc;
    hipLaunchKernelGGL(left_model_kernel, dim3((unsigned)((ncell + 255) / 256), g.streams), dim3(256), 0, s, fr, n_ticks, g, o, scalars, reset, first,
                       cells);
    KCHECK();
}

void launch_left_blobs(const LfFrames& fr, int n_frames, const ScGeom& g, const LfOpts& o, int* head, int* blobs, int* labels, hipStream_t s) {
    const size_t pairs = ((size_t)g.hc * g.wc + 1) / 2, lds = pairs * 8;      // labels and areas, a u16 each per cell: 128 KiB at the most
    set_lds_limit(left_blobs_kernel, (size_t)LF_CELLS_MAX * 4);
    hipLaunchKernelGGL(left_blobs_kernel, dim3((unsigned)n_frames), dim3(BLOB_T), lds, s, fr, g, o.min_cells, o.max_cells, head, blobs, labels);
    KCHECK();
}

void launch_left_walk(const int* head, const int* blobs, int n_ticks, int tick0, const ScGeom& g, const LfOpts& o, int max_objects, const int* reset,
                      int first, int* scalars, int* slots, int* records, int* objects, int* ev_count, int* ev, hipStream_t s) {
    hipLaunchKernelGGL(left_walk_kernel, dim3(ceil_div(g.streams, 64)), dim3(64), 0, s, head, blobs, n_ticks, tick0, g, o, max_objects, reset, first,
                       scalars, slots, records, objects, ev_count, ev);
    KCHECK();
}

void launch_left_events(const int* ev_count, const int* ev, int n_frames, int max_objects, int cap, int* out, int* total, hipStream_t s) {
    hipLaunchKernelGGL(left_events_kernel, dim3(1), dim3(256), 0, s, ev_count, ev, n_frames, max_objects, cap, out, total);
    KCHECK();
}

}  // namespace aic
