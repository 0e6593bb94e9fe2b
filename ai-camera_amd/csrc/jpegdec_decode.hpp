// jpegdec_decode.hpp -- the part of the JPEG decoder that touches camera bytes, as one __host__ __device__ header (in the manner of
// kf7_math.hpp / pre_math.hpp): the per-image record, the Huffman tables, the marker classifier, the bit reader and the block decoder.
// kernels_jpegdec.hip compiles it for the device; jpegdec_host.cpp compiles the same text for the CPU (jpegdec_host_decode), where
// tests/jpegdec_host_probe.cpp runs every corrupt stream under the sanitizers before any of them reaches a GPU.  Every read of a
// file byte goes through JdBits::fill or jd_marker_at, both bounded by the interval's own [pos, end); every loop is bounded by the
// coefficient index or the MCU count.  tests/jpegdec_oracle.py is the specification.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define JD_HD __host__ __device__
#else
#define JD_HD
#endif

namespace aic {

enum JdReason : int32_t {
    JD_OK = 0, JD_TRUNCATED, JD_NOT_JPEG, JD_NOT_BASELINE, JD_PRECISION, JD_COMPONENTS, JD_SAMPLING, JD_SIZE_MISMATCH, JD_BAD_TABLE, JD_MISSING_TABLE,
    JD_BAD_SCAN, JD_RESTART_SEQUENCE, JD_BAD_CODE, JD_OVERRUN, JD_REASONS
};

constexpr int32_t JD_ERR_NONE = 0x7fffffff;      // an image's error word: the smallest (interval + 1) << 8 | reason wins; header and marker errors have interval -1

struct JdHuff {                                  // one Huffman table, 1416 bytes
    uint16_t lut[512];                           // the next 9 bits -> length << 8 | symbol, 0 = longer than 9 bits or no code
    int32_t maxcode[17];                         // [l] = the largest code of length l, -1 when there is none
    int32_t delta[17];                           // [l] = index into val of the first code of length l, minus that code
    uint8_t val[256];
};

struct JdTables {                                // one table set, deduplicated by content within a call
    uint16_t q[4][64];                           // natural order
    JdHuff h[4];                                 // DC0 AC0 DC1 AC1
    uint8_t zz[64];                              // the natural index of a zigzag position
};

struct JdImage {                                 // fixed-size record per image of a launch
    int64_t ent_off, ent_len;                    // the entropy data, relative to the launch's first file byte
    int64_t blk_off;                             // the image's first block in the launch's coefficient buffer (and plane buffer, * 64 bytes)
    int64_t ivl_off;                             // its first interval in the launch's interval table
    int32_t tabset, ncomp, hs, vs;
    int32_t mcus_x, mcus_y, ri, intervals;       // ri: MCUs per interval (the whole image without DRI)
    uint8_t tq[4], td[4], ta[4];                 // per component: quantisation table, DC and AC Huffman table (0 / 1)
    int32_t pad_;
};

// What stands at ent[p] (p < len): 0 = data, 1 = RSTm (m in *m), 2 = another marker, 3 = a fill byte or a lone 0xFF at the very end.
JD_HD inline int jd_marker_at(const uint8_t* ent, int64_t p, int64_t len, int* m) {
    if (ent[p] != 0xFF) return 0;
    if (p + 1 >= len) return 3;
    const int b = ent[p + 1];
    if (b == 0) return 0;
    if (b == 0xFF) return 3;
    if (b >= 0xD0 && b <= 0xD7) { *m = b & 7; return 1; }
    return 2;
}

// The bits of one interval [pos, end): up to the first 0xFF that no 0x00 follows, 0xFF 0x00 unstuffed.  Past the data the reader feeds
// zeros and counts them (pad): a symbol that consumed one of them is JD_OVERRUN -- no bits are invented.
struct JdBits {
    const uint8_t* p;
    int64_t pos, end;
    uint32_t acc;                                // n valid bits at the top
    int n, pad;

    JD_HD void fill() {
        while (n <= 24) {
            uint32_t b = 0;
            if (pos < end) {
                b = p[pos];
                if (b != 0xFF) ++pos;
                else if (pos + 1 < end && p[pos + 1] == 0) pos += 2;
                else end = pos, b = 0, pad += 8;
            } else pad += 8;
            acc |= b << (24 - n);
            n += 8;
        }
    }
    JD_HD uint32_t peek16() { fill(); return acc >> 16; }
    JD_HD void drop(int k) { acc <<= k; n -= k; }
    JD_HD bool over() const { return n < pad; }
    JD_HD int real() const { return n - pad; }
};

// One Huffman symbol: >= 0, or -reason.
JD_HD inline int jd_symbol(JdBits& br, const JdHuff& h) {
    const uint32_t v = br.peek16();
    const uint32_t e = h.lut[v >> 7];
    int sym = -1, len = 0;
    if (e) sym = e & 255, len = e >> 8;
    else
        for (int l = 10; l <= 16; ++l) {
            const int32_t code = (int32_t)(v >> (16 - l));
            if (code <= h.maxcode[l]) {
                sym = h.val[(code + h.delta[l]) & 255], len = l;
                break;
            }
        }
    if (sym < 0) return br.real() < 16 ? -JD_OVERRUN : -JD_BAD_CODE;
    br.drop(len);
    return br.over() ? -JD_OVERRUN : sym;
}

// s bits (1..11) as a signed value (Annex F EXTEND); *bad when they were not all there.
JD_HD inline int jd_extend(JdBits& br, int s, bool* bad) {
    br.fill();
    const int v = (int)(br.acc >> (32 - s));
    br.drop(s);
    *bad = br.over();
    return (v >> (s - 1)) ? v : v - (1 << s) + 1;
}

// One block into out[64] (natural order, zero before the call; only non-zero coefficients are stored).  Returns 0 or the reason.
JD_HD inline int jd_block(JdBits& br, const JdHuff& dc, const JdHuff& ac, const uint8_t* zz, int32_t* pred, int16_t* out) {
    bool bad = false;
    int s = jd_symbol(br, dc);
    if (s < 0) return -s;
    if (s > 11) return JD_BAD_CODE;
    if (s) {
        *pred += jd_extend(br, s, &bad);
        if (bad) return JD_OVERRUN;
    }
    if (*pred < -32768 || *pred > 32767) return JD_BAD_CODE;
    if (*pred) out[0] = (int16_t)*pred;
    for (int k = 1; k < 64;) {
        const int rs = jd_symbol(br, ac);
        if (rs < 0) return -rs;
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (run != 15) break;
            if (k + 16 > 64) return JD_BAD_CODE;
            k += 16;
            continue;
        }
        k += run;
        if (s > 10 || k > 63) return JD_BAD_CODE;
        const int v = jd_extend(br, s, &bad);
        if (bad) return JD_OVERRUN;
        out[zz[k]] = (int16_t)v;
        ++k;
    }
    return 0;
}

JD_HD inline int jd_bpm(const JdImage& im) { return im.ncomp == 1 ? 1 : im.hs * im.vs + 2; }

// Restart interval k of an image: its MCUs' blocks into coef (the image's [MCU, block, 64]).  ent: the image's entropy data,
// [lo, hi) the interval's bytes within it.  Returns 0 or the reason.
JD_HD inline int jd_interval(const JdImage& im, const JdTables& t, const uint8_t* ent, int64_t lo, int64_t hi, int k, int16_t* coef) {
    JdBits br{ent, lo, hi, 0u, 0, 0};
    int32_t p0 = 0, p1 = 0, p2 = 0;                                           // the DC predictors: scalars, not an indexed array
    const int bpm = jd_bpm(im), ny = bpm - (im.ncomp - 1), ri = im.ri;        // the record is read once: the stores below could alias it
    const int64_t n_mcu = (int64_t)im.mcus_x * im.mcus_y;
    const int64_t m0 = (int64_t)k * ri, m1 = m0 + ri < n_mcu ? m0 + ri : n_mcu;
    const JdHuff* const d0 = &t.h[2 * (im.td[0] & 1)];
    const JdHuff* const d1 = &t.h[2 * (im.td[1] & 1)];
    const JdHuff* const d2 = &t.h[2 * (im.td[2] & 1)];
    const JdHuff* const a0 = &t.h[2 * (im.ta[0] & 1) + 1];
    const JdHuff* const a1 = &t.h[2 * (im.ta[1] & 1) + 1];
    const JdHuff* const a2 = &t.h[2 * (im.ta[2] & 1) + 1];
    for (int64_t m = m0; m < m1; ++m)
        for (int b = 0; b < bpm; ++b) {
            const int c = b < ny ? 0 : b - ny + 1;
            int32_t pred = c == 0 ? p0 : c == 1 ? p1 : p2;
            const int r = jd_block(br, c == 0 ? *d0 : c == 1 ? *d1 : *d2, c == 0 ? *a0 : c == 1 ? *a1 : *a2, t.zz, &pred, coef + (m * bpm + b) * 64);
            if (r) return r;
            if (c == 0) p0 = pred;
            else if (c == 1) p1 = pred;
            else p2 = pred;
        }
    return 0;
}

}  // namespace aic
