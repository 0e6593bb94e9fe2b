// kernels_render.hip -- the tiled rasteriser of the redaction / annotation stage (render.hpp): one launch
// renders every frame of a chunk, grid = tiles x frames, a block of 256 threads per tile of 64 x 32 pixels.  Integer arithmetic only;
// tests/render_oracle.py is the specification and the kernel matches it bit for bit.  Per pixel, the first rule that applies:
//   (a) the colour of the LAST primitive of the frame's list that covers it (kinds 0..2 as kernels_overlay.hip, kind 3 = a segment)
//   (b) mask_color inside a mask polygon of the frame's camera (even-odd, half-open edges, as kernels_zones.hip)
//   (c) inside the union of the frame's redaction rectangles: fill_color, or the mean of the ORIGINAL pixels of its mosaic cell
//   (d) unchanged
// A block:
//   1. bins: every rectangle, primitive and polygon of its frame is tested against the tile by its bounding box, 256 at a time; a wave's
//      ballot is one 64-bit word of a survivor bit set in LDS -- list order kept, any count fits (1500 + 512 + 32 bits), no atomics.
//      Nothing survives: the block returns without reading or writing a pixel.
//   2. stages the tile's original pixels in LDS (coalesced dword loads, or a byte path when rows are not dword aligned), the surviving
//      polygons' vertices beside them, and notes which mosaic cells hold a redacted pixel.
//   3. mosaic: sums of the 4 x 4 sub-cells of the noted cells, then the cells' means (a cell is 4..32 pixels, the tile sides are
//      multiples of 32 and the grid starts at the frame's origin, so a cell never leaves its tile).
//   4. after the barrier every thread resolves its 8 pixels (one row, 8 columns) and stores only what changed.  In place is safe: a block
//      owns its tile and has read all of it before the barrier.
// LDS tile layout: interleaved BGR as in memory, a row is 48 dwords and a thread's 8 pixels are 6 dwords, so a wave reads dwords 6 * lane
// + k: lanes l and l + 16 would share a bank of ds_read_b32's 32 (2-way).  One dword of padding per two rows (96 dwords = 16 threads)
// shifts every 16-lane quarter by one bank and the read is conflict-free; the staging writes stay linear.
#include "font5x7.hpp"
#include "render.hpp"

namespace aic {

namespace {

constexpr int TW = RENDER_TILE_W, TH = RENDER_TILE_H;
constexpr int ROW_BYTES = TW * 3;                       // 192
constexpr int TILE_BYTES = ROW_BYTES * TH + (TH / 2) * 4;
constexpr int PRIM_WORDS = (RENDER_PRIMS_MAX + 255) / 256 * 4;   // 24 ballot words
constexpr int RECT_WORDS = RENDER_ROWS_MAX / 64;                  // 8

struct Prim { int kind, x0, y0, x1, y1, color, toff, tlen_scale; };

__device__ __forceinline__ int lds_off(int y, int b) { return y * ROW_BYTES + (y >> 1) * 4 + b; }

__device__ __forceinline__ bool prim_reaches(const Prim& p, int tx0, int ty0, int tx1, int ty1) {
    long long x0, y0, x1, y1;
    if (p.kind == 1) {
        x0 = p.x0, y0 = p.y0, x1 = p.x1, y1 = p.y1;
    } else if (p.kind == 0) {
        x0 = p.x0 - 1, y0 = p.y0 - 1, x1 = p.x1 + 1, y1 = p.y1 + 1;
    } else if (p.kind == 2) {
        const long long s = p.tlen_scale >> 16, len = p.tlen_scale & 0xffff;
        x0 = p.x0, y0 = p.y0, x1 = p.x0 + 6 * s * len - 1, y1 = p.y0 + 7 * s - 1;
    } else {
        const int t = p.toff;
        x0 = min(p.x0, p.x1) - t, x1 = max(p.x0, p.x1) + t, y0 = min(p.y0, p.y1) - t, y1 = max(p.y0, p.y1) + t;
    }
    return x0 <= tx1 && x1 >= tx0 && y0 <= ty1 && y1 >= ty0;
}

// bit j = primitive p covers pixel (x + j, y), j < 8
__device__ __forceinline__ unsigned prim_hits(const Prim& p, int x, int y, const unsigned char* __restrict__ text) {
    unsigned m = 0;
    if (p.kind == 1) {
        if (y >= p.y0 && y <= p.y1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) m |= (unsigned)(x + j >= p.x0 && x + j <= p.x1) << j;
        }
    } else if (p.kind == 0) {
        if (y >= p.y0 - 1 && y <= p.y1 + 1) {
            const bool yin = y > p.y0 && y < p.y1;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int xx = x + j;
                const bool outer = xx >= p.x0 - 1 && xx <= p.x1 + 1, inner = yin && xx > p.x0 && xx < p.x1;
                m |= (unsigned)(outer && !inner) << j;
            }
        }
    } else if (p.kind == 2) {
        const int s = p.tlen_scale >> 16, len = p.tlen_scale & 0xffff;
        const int dy = y - p.y0;
        if (dy >= 0 && dy < 7 * s) {
            const int gy = dy / s;
            const long long wtext = 6LL * s * len;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long dx = (long long)x + j - p.x0;
                if (dx >= 0 && dx < wtext) {
                    const int ci = (int)(dx / (6 * s)), gx = (int)(dx - (long long)ci * 6 * s) / s;
                    const int ch = text[p.toff + ci];
                    if (gx < 5 && ch >= 32 && ch <= 126) m |= (unsigned)((kFont5x7[(ch - 32) * 5 + gx] >> gy) & 1) << j;
                }
            }
        }
    } else {
        const long long dx = (long long)p.x1 - p.x0, dy = (long long)p.y1 - p.y0, t = p.toff;
        const long long adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
        if (adx >= ady && dx != 0) {
            const int lo = min(p.x0, p.x1), hi = max(p.x0, p.x1);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int xx = x + j;
                long long e = dx * (y - p.y0) - dy * (xx - p.x0);
                e = e < 0 ? -e : e;
                m |= (unsigned)(xx >= lo && xx <= hi && 2 * e <= t * adx) << j;
            }
        } else if (ady > adx) {
            if (y >= min(p.y0, p.y1) && y <= max(p.y0, p.y1)) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    long long e = dy * (x + j - p.x0) - dx * (y - p.y0);
                    e = e < 0 ? -e : e;
                    m |= (unsigned)(2 * e <= t * ady) << j;
                }
            }
        }
    }
    return m;
}

struct RenderArgs {
    unsigned char* frames;            // [F, H, W, 3] of this launch
    int h, w;
    const int* rect_off;              // [F + 1], absolute into rects
    const int* prim_off;              // [F + 1], absolute into prims
    const int* cam;                   // [F]
    const int* rects;                 // [n, 4]
    const Prim* prims;
    const unsigned char* text;
    const int* geo;                   // [cameras][RENDER_GEO_INTS]
    int tiles_x;
    int style, cell, fill_color, mask_color;
};

template <bool DWORDS>
__global__ __launch_bounds__(256) void render_tiles_kernel(RenderArgs a) {
    __shared__ unsigned long long s_pm[PRIM_WORDS], s_rm[RECT_WORDS];
    __shared__ unsigned s_polym;
    __shared__ __attribute__((aligned(16))) unsigned char s_tile[TILE_BYTES];
    __shared__ int s_poly[RENDER_POLYS_MAX * RENDER_VERTS_MAX * 2];
    __shared__ int s_need[128];
    __shared__ int s_sub[128 * 3];
    __shared__ int s_mean[128];       // packed B | G << 8 | R << 16 per cell

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.y;
    const int tx0 = (blockIdx.x % a.tiles_x) * TW, ty0 = (blockIdx.x / a.tiles_x) * TH;
    const int tx1 = min(tx0 + TW, a.w) - 1, ty1 = min(ty0 + TH, a.h) - 1;
    const int r_lo = a.rect_off[f], n_rect = a.rect_off[f + 1] - r_lo;
    const int p_lo = a.prim_off[f], n_prim = a.prim_off[f + 1] - p_lo;
    const int* geo = a.geo + (size_t)a.cam[f] * RENDER_GEO_INTS;
    const int n_poly = geo[0];
    const int* rects = a.rects + (size_t)r_lo * 4;
    const Prim* prims = a.prims + p_lo;

    // ---- 1. binning
    for (int base = 0; base < n_rect; base += 256) {
        const int i = base + tid;
        bool hit = false;
        if (i < n_rect) {
            const int4 r = *reinterpret_cast<const int4*>(rects + (size_t)i * 4);
            hit = r.x <= tx1 && r.z >= tx0 && r.y <= ty1 && r.w >= ty0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_rm[(base >> 6) + wave] = m;
    }
    for (int base = 0; base < n_prim; base += 256) {
        const int i = base + tid;
        bool hit = false;
        if (i < n_prim) hit = prim_reaches(prims[i], tx0, ty0, tx1, ty1);
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_pm[(base >> 6) + wave] = m;
    }
    if (wave == 0) {
        bool hit = false;
        if (lane < n_poly) {
            const int4 b = *reinterpret_cast<const int4*>(geo + RENDER_GEO_BOX + lane * 4);
            hit = b.x <= tx1 && b.z >= tx0 && b.y <= ty1 && b.w >= ty0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_polym = (unsigned)m;
    }
    if (tid < 128) s_need[tid] = 0;
    __syncthreads();
    const int rw = (n_rect + 63) >> 6, pw = (n_prim + 63) >> 6;
    unsigned long long any_r = 0, any_p = 0;
    for (int k = 0; k < rw; ++k) any_r |= s_rm[k];
    for (int k = 0; k < pw; ++k) any_p |= s_pm[k];
    const unsigned polym = s_polym;
    if (!(any_r | any_p | polym)) return;                 // nothing reaches the tile: no pixel is read or written

    // ---- 2. staging: the tile's original pixels (zeros outside the frame), the surviving polygons, the redacted pixels of this thread
    unsigned char* fb = a.frames + (size_t)f * a.h * a.w * 3;
    const size_t row_bytes = (size_t)a.w * 3;
    const int row_valid = (int)min((long long)ROW_BYTES, (long long)row_bytes - (long long)tx0 * 3);   // bytes of a tile row inside the frame
    if (DWORDS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int i = tid + 256 * k, y = i / 48, c = i % 48;
            unsigned v = 0;
            if (ty0 + y < a.h && c * 4 < row_valid) v = *reinterpret_cast<const unsigned*>(fb + (size_t)(ty0 + y) * row_bytes + (size_t)tx0 * 3 + c * 4);
            *reinterpret_cast<unsigned*>(s_tile + lds_off(y, c * 4)) = v;
        }
    } else {
        for (int k = 0; k < 24; ++k) {
            const int i = tid + 256 * k, y = i / ROW_BYTES, c = i % ROW_BYTES;
            unsigned char v = 0;
            if (ty0 + y < a.h && c < row_valid) v = fb[(size_t)(ty0 + y) * row_bytes + (size_t)tx0 * 3 + c];
            s_tile[lds_off(y, c)] = v;
        }
    }
    for (unsigned pm = polym; pm;) {
        const int p = __ffs(pm) - 1;
        pm &= pm - 1;
        const int nv2 = geo[RENDER_GEO_NVERT + p] * 2;
        if (tid < nv2) s_poly[p * RENDER_VERTS_MAX * 2 + tid] = geo[RENDER_GEO_XY + p * RENDER_VERTS_MAX * 2 + tid];
    }
    const int ly = tid >> 3, lx = (tid & 7) * 8;          // this thread's pixels: row ly, columns lx .. lx + 7 of the tile
    const int x = tx0 + lx, y = ty0 + ly;
    unsigned valid = 0;
    if (y < a.h) {
#pragma unroll
        for (int j = 0; j < 8; ++j) valid |= (unsigned)(x + j < a.w) << j;
    }
    unsigned red = 0;
    if (valid) {
        for (int k = rw - 1; k >= 0 && red != valid; --k) {
            for (unsigned long long m = s_rm[k]; m && red != valid;) {
                const int b = 63 - __clzll((long long)m);
                m &= ~(1ull << b);
                const int4 r = *reinterpret_cast<const int4*>(rects + (size_t)(k * 64 + b) * 4);
                if (y >= r.y && y <= r.w) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) red |= (unsigned)(x + j >= r.x && x + j <= r.z) << j;
                }
            }
        }
        red &= valid;
    }
    const bool mosaic = a.style == RENDER_STYLE_MOSAIC && any_r != 0;
    const int c = a.cell, cs = 31 - __clz(c), ncx = TW >> cs, q = c >> 2;      // c is 4, 8, 16 or 32
    if (mosaic && red) {                                  // 8 columns from a multiple of 8: two cells when c = 4, else one; every writer stores 1
        const int cell0 = (ly >> cs) * ncx + (lx >> cs);
        if (c == 4) {
            if (red & 0x0f) s_need[cell0] = 1;
            if (red & 0xf0) s_need[cell0 + 1] = 1;
        } else {
            s_need[cell0] = 1;
        }
    }
    __syncthreads();

    // ---- 3. mosaic means of the noted cells
    if (mosaic) {
        for (int k = tid; k < 128 * 3; k += 256) {
            const int sub = k / 3, ch = k % 3, sx = sub & 15, sy = sub >> 4;
            int sum = 0;
            if (s_need[(sy / q) * ncx + sx / q]) {
#pragma unroll
                for (int yy = 0; yy < 4; ++yy)
#pragma unroll
                    for (int xx = 0; xx < 4; ++xx) sum += s_tile[lds_off(sy * 4 + yy, (sx * 4 + xx) * 3 + ch)];
            }
            s_sub[k] = sum;
        }
        __syncthreads();
        const int ncells = ncx * (TH >> cs);
        if (tid < ncells && s_need[tid]) {
            const int cx = tid % ncx, cy = tid / ncx;
            const int n = min(c, a.w - (tx0 + cx * c)) * min(c, a.h - (ty0 + cy * c));      // the pixels the cell has inside the frame
            int packed = 0;
            for (int ch = 0; ch < 3; ++ch) {
                int sum = 0;
                for (int sy = 0; sy < q; ++sy)
                    for (int sx = 0; sx < q; ++sx) sum += s_sub[((cy * q + sy) * 16 + cx * q + sx) * 3 + ch];
                packed |= ((sum + n / 2) / n) << (8 * ch);
            }
            s_mean[tid] = packed;
        }
        __syncthreads();
    }
    if (!valid) return;

    // ---- 4. resolve this thread's 8 pixels
    unsigned o[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = *reinterpret_cast<const unsigned*>(s_tile + lds_off(ly, lx * 3 + k * 4));
    unsigned col[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int bit = 24 * j, k = bit >> 5, sh = bit & 31;
        col[j] = (sh <= 8 ? o[k] >> sh : (o[k] >> sh) | (o[k + 1] << (32 - sh))) & 0xffffff;
    }
    unsigned have = 0;
    // (a) primitives, last first
    for (int k = pw - 1; k >= 0 && have != valid; --k) {
        for (unsigned long long m = s_pm[k]; m && have != valid;) {
            const int b = 63 - __clzll((long long)m);
            m &= ~(1ull << b);
            const Prim p = prims[k * 64 + b];
            const unsigned hits = prim_hits(p, x, y, a.text) & valid & ~have;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((hits >> j) & 1) col[j] = (unsigned)p.color & 0xffffff;
            have |= hits;
        }
    }
    // (b) static masks
    if (polym && have != valid) {
        unsigned inside = 0;
        for (unsigned pm = polym; pm;) {
            const int p = __ffs(pm) - 1;
            pm &= pm - 1;
            const int nv = geo[RENDER_GEO_NVERT + p];
            const int* v = s_poly + p * RENDER_VERTS_MAX * 2;
            unsigned odd = 0;
            for (int i = 0; i < nv; ++i) {
                const int i2 = i + 1 == nv ? 0 : i + 1;
                const int ax = v[2 * i], ay = v[2 * i + 1], bx = v[2 * i2], by = v[2 * i2 + 1];
                if ((ay > y) != (by > y)) {
                    const long long d0 = (long long)(bx - ax) * (y - ay) - (long long)(x - ax) * (by - ay);
                    const long long step = by - ay;                                      // d(x + j) = d0 - j * step
                    const bool up = by > ay;
#pragma unroll
                    for (int j = 0; j < 8; ++j) odd ^= (unsigned)(((d0 - j * step) > 0) == up) << j;
                }
            }
            inside |= odd;
        }
        const unsigned hits = inside & valid & ~have;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if ((hits >> j) & 1) col[j] = (unsigned)a.mask_color;
        have |= hits;
    }
    // (c) redaction
    {
        const unsigned hits = red & ~have;
        if (hits) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if ((hits >> j) & 1) col[j] = mosaic ? (unsigned)s_mean[(ly >> cs) * ncx + ((lx + j) >> cs)] : (unsigned)a.fill_color;
            have |= hits;
        }
    }
    if (!have) return;
    // ---- stores: only what changed
    unsigned char* dst = fb + (size_t)y * row_bytes + (size_t)x * 3;
    if (DWORDS) {
        unsigned nw[6];
        nw[0] = col[0] | col[1] << 24;
        nw[1] = col[1] >> 8 | col[2] << 16;
        nw[2] = col[2] >> 16 | col[3] << 8;
        nw[3] = col[4] | col[5] << 24;
        nw[4] = col[5] >> 8 | col[6] << 16;
        nw[5] = col[6] >> 16 | col[7] << 8;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (nw[k] != o[k]) reinterpret_cast<unsigned*>(dst)[k] = nw[k];      // a differing dword holds a changed, hence valid, pixel
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int bit = 24 * j, k = bit >> 5, sh = bit & 31;
            const unsigned was = (sh <= 8 ? o[k] >> sh : (o[k] >> sh) | (o[k + 1] << (32 - sh))) & 0xffffff;
            if (((have >> j) & 1) && col[j] != was) {
                dst[3 * j] = (unsigned char)col[j], dst[3 * j + 1] = (unsigned char)(col[j] >> 8), dst[3 * j + 2] = (unsigned char)(col[j] >> 16);
            }
        }
    }
}

}  // namespace

void launch_render_tiles(unsigned char* frames, int n_frames, int h, int w, const int* rect_off, const int* prim_off, const int* cam, const int* rects,
                         const int* prims, const unsigned char* text, const int* geo, int style, int cell, int fill_color, int mask_color,
                         hipStream_t s) {
    if (n_frames <= 0) return;
    RenderArgs a;
    a.frames = frames, a.h = h, a.w = w, a.rect_off = rect_off, a.prim_off = prim_off, a.cam = cam, a.rects = rects;
    a.prims = reinterpret_cast<const Prim*>(prims), a.text = text, a.geo = geo;
    a.tiles_x = ceil_div(w, TW);
    a.style = style, a.cell = cell, a.fill_color = fill_color, a.mask_color = mask_color;
    const dim3 grid((unsigned)a.tiles_x * (unsigned)ceil_div(h, TH), (unsigned)n_frames);
    const bool dwords = ((size_t)w * 3) % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 4 == 0;
    if (dwords) hipLaunchKernelGGL(render_tiles_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(render_tiles_kernel<false>, grid, dim3(256), 0, s, a);
    KCHECK();
}

}  // namespace aic
