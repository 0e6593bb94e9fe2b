// row_band.cpp -- the row-band planner (row_band.hpp).  Plain C++.
#include "row_band.hpp"

#include <algorithm>

namespace aic {

namespace {

inline int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
inline int ceil_div(int a, int b) { return -floor_div(-a, b); }
inline bool overlap(int a0, int an, int b0, int bn) { return a0 < b0 + bn && b0 < a0 + an; }

struct Slice { int buf, c0, cn; RowBand band; };

RowBand all_rows(int h) { RowBand b; b.lo = 0, b.hi = h - 1, b.full = true; return b; }

RowBand clip(int lo, int hi, int h) {
    RowBand b;
    b.lo = std::max(lo, 0), b.hi = std::min(hi, h - 1);
    b.full = h - (b.hi - b.lo + 1) < kRowBandMinSaved;
    if (b.full) b.lo = 0, b.hi = h - 1;
    return b;
}

// the hull of the bands of the slices [c0, c0 + cn) of `buf` overlaps; channels nobody has written: unknown -> all rows
RowBand read_band(const std::vector<Slice>& sl, int buf, int c0, int cn, int h) {
    int covered = 0, lo = h, hi = -1;
    for (const Slice& s : sl) {
        if (s.buf != buf || !overlap(s.c0, s.cn, c0, cn)) continue;
        if (s.band.full) return all_rows(h);
        covered += std::min(s.c0 + s.cn, c0 + cn) - std::max(s.c0, c0);
        lo = std::min(lo, s.band.lo), hi = std::max(hi, s.band.hi);
    }
    if (covered < cn) return all_rows(h);
    RowBand b;
    b.lo = lo, b.hi = hi, b.full = false;
    return b;
}

// the writer of [c0, c0 + cn) takes those channels over: what other slices held of them goes
void write_band(std::vector<Slice>& sl, int buf, int c0, int cn, const RowBand& band) {
    std::vector<Slice> out;
    for (const Slice& s : sl) {
        if (s.buf != buf || !overlap(s.c0, s.cn, c0, cn)) { out.push_back(s); continue; }
        if (s.c0 < c0) out.push_back(Slice{buf, s.c0, c0 - s.c0, s.band});
        if (s.c0 + s.cn > c0 + cn) out.push_back(Slice{buf, c0 + cn, s.c0 + s.cn - (c0 + cn), s.band});
    }
    out.push_back(Slice{buf, c0, cn, band});
    sl.swap(out);
}

constexpr int kAllChannels = 1 << 30;

}  // namespace

std::vector<RowBand> plan_row_bands(const std::vector<RbOp>& ops, const std::vector<int>& buf_h, int top, int unpad_h, bool side_pad) {
    std::vector<RowBand> bands(ops.size());
    std::vector<Slice> sl;
    const int nb = (int)buf_h.size();
    if (nb == 0) return bands;
    {
        RowBand in = all_rows(buf_h[0]);
        if (!side_pad && top >= 0 && unpad_h > 0 && top + unpad_h <= buf_h[0]) in = clip(top, top + unpad_h - 1, buf_h[0]);
        sl.push_back(Slice{0, 0, kAllChannels, in});
    }
    for (size_t i = 0; i < ops.size(); ++i) {
        const RbOp& o = ops[i];
        if (o.dst < 0 || o.dst >= nb || o.src < 0 || o.src >= nb) { bands[i] = RowBand{}; continue; }
        const int ho = buf_h[o.dst];
        if (!o.conv || o.stride < 1 || o.k < 1) {
            bands[i] = all_rows(ho);
            write_band(sl, o.dst, o.dst_c0, o.dst_cn, bands[i]);    // (an op the planner does not model: nothing is known about what it wrote)
            continue;
        }
        RowBand b = read_band(sl, o.src, o.src_c0, o.src_cn, buf_h[o.src]);
        if (!b.full) b = clip(ceil_div(b.lo + o.pad - o.k + 1, o.stride), floor_div(b.hi + o.pad, o.stride), ho);
        else b = all_rows(ho);
        if (o.res >= 0 && !b.full) {
            const RowBand r = o.res < nb && buf_h[o.res] == ho ? read_band(sl, o.res, o.res_c0, o.dst_cn, ho) : all_rows(ho);
            b = r.full ? all_rows(ho) : clip(std::min(b.lo, r.lo), std::max(b.hi, r.hi), ho);
        }
        bands[i] = b;
        write_band(sl, o.dst, o.dst_c0, o.dst_cn, b);
    }
    return bands;
}

TileWindow tile_window(int y0, int rows, int th, int Ho) {
    if (rows <= 0 || th <= 0) return TileWindow{0, th > 0 ? ceil_div(Ho, th) : 0};
    const int tiles = std::min(ceil_div(rows, th), ceil_div(Ho, th));
    return TileWindow{std::max(0, std::min(y0, Ho - tiles * th)), tiles};
}

std::vector<RowWindow> plan_row_windows(const std::vector<RbStep>& steps, const std::vector<RowBand>& bands) {
    const int ns = (int)steps.size();
    std::vector<RowWindow> win(ns);
    auto writes = [&](int j, const RbStep& s) { return steps[j].dst == s.dst && overlap(steps[j].dst_c0, steps[j].dst_cn, s.dst_c0, s.dst_cn); };
    // the rows a step computes: its window, in whole tiles unless the kernel stores exact rows
    auto computed = [&](int j, int& lo, int& hi) {
        const RbStep& s = steps[j];
        if (win[j].rows == 0) { lo = 0, hi = s.Ho - 1; return; }
        if (s.exact) { lo = win[j].y0, hi = win[j].y0 + win[j].rows - 1; return; }
        const TileWindow t = tile_window(win[j].y0, win[j].rows, s.th, s.Ho);
        lo = t.origin, hi = std::min(t.origin + t.tiles * s.th, s.Ho) - 1;
    };
    for (int i = ns - 1; i >= 0; --i) {           // readers before their writers: a writer of a shared slice covers what they read
        const RbStep& s = steps[i];
        win[i] = RowWindow{};
        if (s.th <= 0 || s.op < 0 || s.op >= (int)bands.size() || bands[s.op].full || bands[s.op].hi < bands[s.op].lo) continue;
        int lo = bands[s.op].lo, hi = bands[s.op].hi;
        bool shared = false, full = false;
        for (int j = 0; j < ns; ++j) shared = shared || (j != i && writes(j, s));
        if (shared) {
            // the readers this writer serves: from behind it to the next writer of the slice, cyclically (a reader in front of the list's
            // first writer reads what the last writer left in the previous run)
            for (int d = 1; d < ns && !full; ++d) {
                const int j = (i + d) % ns;
                if (writes(j, s)) break;
                for (const RbRead& r : steps[j].reads) {
                    if (r.buf != s.dst || !overlap(r.c0, r.cn, s.dst_c0, s.dst_cn)) continue;
                    if (j < i) { full = true; break; }               // (its window is not planned yet: it reads anything)
                    int a, b;
                    computed(j, a, b);
                    if (r.all || win[j].rows == 0) { full = true; break; }
                    lo = std::min(lo, std::max(a * r.stride - r.halo_lo, 0));
                    hi = std::max(hi, std::min(b * r.stride + r.halo_hi, s.Ho - 1));
                }
            }
        }
        if (full) continue;
        const int rows = hi - lo + 1;
        if (ceil_div(rows, s.th) >= ceil_div(s.Ho, s.th) || s.Ho - rows < (s.exact ? kRowBandMinSaved : 1)) continue;
        win[i] = RowWindow{lo, rows};
    }
    return win;
}

}  // namespace aic
