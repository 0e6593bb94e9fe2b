// jpegdec_host.cpp -- the HIP-free half of the JPEG decoding stage (jpegdec_host.hpp).  The parse reads file[0, bytes) and nothing else:
// every access is preceded by a comparison with `bytes` or with the end of the segment it is in.
#include "jpegdec_host.hpp"

#include <cstring>

#include "jpeg_host.hpp"

namespace aic {

namespace {

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

bool huff_ok(const uint8_t counts[16]) {
    int code = 0;
    for (int l = 1; l <= 16; ++l) {
        code += counts[l - 1];
        if (code > (1 << l)) return false;
        code <<= 1;
    }
    return true;
}

// One DHT segment's payload into p.huff.  false: BAD_TABLE.
bool read_dht(const uint8_t* seg, int len, JdParsed& p, bool* any) {
    int k = 0;
    while (k < len) {
        const int tc = seg[k] >> 4, th = seg[k] & 15;
        if (tc > 1 || th > 1 || k + 17 > len) return false;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[k + 1 + i];
        if (total > 256 || k + 17 + total > len || !huff_ok(seg + k + 1)) return false;
        JdParsed::Huff& h = p.huff[2 * th + tc];
        std::memcpy(h.counts, seg + k + 1, 16);
        std::memset(h.val, 0, 256);
        std::memcpy(h.val, seg + k + 17, (size_t)total);
        h.have = true, *any = true;
        k += 17 + total;
    }
    return true;
}

// The Annex K tables, read back from the header the encoder writes (jpeg_host.cpp spells them out once for both stages).
void annex_k(JdParsed& p) {
    uint8_t hdr[JPEG_HEADER_BYTES];
    jpeg_header(jpeg_geometry(8, 8, 0, 444), 50, hdr);
    bool any = false;
    for (int pos = 2; pos + 4 <= JPEG_HEADER_BYTES;) {
        const int m = hdr[pos + 1], len = (hdr[pos + 2] << 8) | hdr[pos + 3];
        if (m == 0xC4) read_dht(hdr + pos + 4, len - 2, p, &any);
        if (m == 0xDA) break;
        pos += 2 + len;
    }
}

int refuse(JdParsed& out, int reason) {
    out.info = aic_jpegdec_info{};
    out.info.status = AIC_ERR_FORMAT, out.info.reason = reason;
    return reason;
}

}  // namespace

int jpegdec_parse(const uint8_t* f, int64_t n, int height, int width, JdParsed& out) {
    out.info = aic_jpegdec_info{};
    out.rec = JdImage{};
    for (int i = 0; i < 4; ++i) out.have_quant[i] = false, out.huff[i].have = false;
    if (n < 2 || f[0] != 0xFF || f[1] != 0xD8) return refuse(out, JD_NOT_JPEG);
    bool have_frame = false, any_dht = false;
    int ri = 0, adobe = -1, h = 0, w = 0, ncomp = 0;
    uint8_t cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0}, ctq[3] = {0, 0, 0};
    int64_t pos = 2;
    for (;;) {
        if (pos + 2 > n) return refuse(out, JD_TRUNCATED);
        if (f[pos] != 0xFF) return refuse(out, JD_NOT_JPEG);
        const int m = f[pos + 1];
        if (m == 0xFF) { ++pos; continue; }                                   // a fill byte
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
        if (m == 0xD8) return refuse(out, JD_NOT_JPEG);
        if (m == 0xD9) return refuse(out, JD_BAD_SCAN);
        if (pos + 2 > n) return refuse(out, JD_TRUNCATED);
        const int length = (f[pos] << 8) | f[pos + 1];
        if (length < 2) return refuse(out, JD_NOT_JPEG);
        if (pos + length > n) return refuse(out, JD_TRUNCATED);
        const uint8_t* seg = f + pos + 2;                                     // seg[0, len) is inside the file
        const int len = length - 2;
        pos += length;
        if (m == 0xC0) {
            if (have_frame) return refuse(out, JD_NOT_BASELINE);
            if (len < 6) return refuse(out, JD_NOT_JPEG);
            if (seg[0] != 8) return refuse(out, JD_PRECISION);
            if (seg[5] != 1 && seg[5] != 3) return refuse(out, JD_COMPONENTS);
            ncomp = seg[5];
            if (len != 6 + 3 * ncomp) return refuse(out, JD_NOT_JPEG);
            h = (seg[1] << 8) | seg[2], w = (seg[3] << 8) | seg[4];
            if (h < 1 || h > JPEGDEC_DIM_MAX || w < 1 || w > JPEGDEC_DIM_MAX || (height > 0 && h != height) || (width > 0 && w != width))
                return refuse(out, JD_SIZE_MISMATCH);
            for (int i = 0; i < ncomp; ++i) cid[i] = seg[6 + 3 * i], ch[i] = seg[7 + 3 * i] >> 4, cv[i] = seg[7 + 3 * i] & 15, ctq[i] = seg[8 + 3 * i];
            bool ok = ch[0] == 1 && cv[0] == 1;
            if (ncomp == 3)
                ok = (ok || (ch[0] == 2 && (cv[0] == 1 || cv[0] == 2))) && ch[1] == 1 && cv[1] == 1 && ch[2] == 1 && cv[2] == 1;
            if (!ok) return refuse(out, JD_SAMPLING);
            for (int i = 0; i < ncomp; ++i)
                if (ctq[i] > 3) return refuse(out, JD_BAD_TABLE);
            have_frame = true;
        } else if (m == 0xC1 || m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCF)) {
            return refuse(out, JD_NOT_BASELINE);
        } else if (m == 0xDB) {
            for (int k = 0; k < len; k += 65) {
                if ((seg[k] >> 4) || (seg[k] & 15) > 3 || k + 65 > len) return refuse(out, JD_BAD_TABLE);
                const int id = seg[k] & 15;
                for (int z = 0; z < 64; ++z) out.quant[id][ZIGZAG[z]] = seg[k + 1 + z];
                out.have_quant[id] = true;
            }
        } else if (m == 0xC4) {
            if (!read_dht(seg, len, out, &any_dht)) return refuse(out, JD_BAD_TABLE);
        } else if (m == 0xDD) {
            if (len != 2) return refuse(out, JD_NOT_JPEG);
            ri = (seg[0] << 8) | seg[1];
        } else if (m == 0xEE) {
            if (len >= 12 && std::memcmp(seg, "Adobe", 5) == 0) adobe = seg[11];
        } else if (m == 0xDA) {
            if (!have_frame) return refuse(out, JD_BAD_SCAN);
            if (len < 1 || seg[0] != ncomp || len != 4 + 2 * ncomp) return refuse(out, JD_BAD_SCAN);
            JdImage& r = out.rec;
            for (int i = 0; i < ncomp; ++i) {
                const int td = seg[2 + 2 * i] >> 4, ta = seg[2 + 2 * i] & 15;
                if (seg[1 + 2 * i] != cid[i] || td > 1 || ta > 1) return refuse(out, JD_BAD_SCAN);
                r.td[i] = (uint8_t)td, r.ta[i] = (uint8_t)ta, r.tq[i] = ctq[i];
            }
            if (seg[len - 3] != 0 || seg[len - 2] != 63 || seg[len - 1] != 0) return refuse(out, JD_BAD_SCAN);
            if (ncomp == 3 && adobe == 0) return refuse(out, JD_COMPONENTS);
            for (int i = 0; i < ncomp; ++i)
                if (!out.have_quant[ctq[i]]) return refuse(out, JD_MISSING_TABLE);
            if (!any_dht) annex_k(out);                                       // the Motion-JPEG convention: no DHT at all means Annex K
            for (int i = 0; i < ncomp; ++i)
                if (!out.huff[2 * r.td[i]].have || !out.huff[2 * r.ta[i] + 1].have) return refuse(out, JD_MISSING_TABLE);
            if (n - pos < 2 || f[n - 2] != 0xFF || f[n - 1] != 0xD9) return refuse(out, JD_TRUNCATED);
            r.ncomp = ncomp, r.hs = ch[0], r.vs = cv[0];
            r.mcus_x = (w + 8 * r.hs - 1) / (8 * r.hs), r.mcus_y = (h + 8 * r.vs - 1) / (8 * r.vs);
            const int64_t n_mcu = (int64_t)r.mcus_x * r.mcus_y;
            r.ri = ri ? ri : (int32_t)n_mcu;
            r.intervals = (int32_t)((n_mcu + r.ri - 1) / r.ri);
            aic_jpegdec_info& o = out.info;
            o.width = w, o.height = h, o.components = ncomp;
            o.sampling = ncomp == 1 ? 400 : r.hs == 1 ? 444 : r.vs == 1 ? 422 : 420;
            o.restart = ri, o.intervals = r.intervals, o.entropy_offset = pos, o.entropy_bytes = n - 2 - pos;
            return 0;
        }
        // APPn, COM and every other segment: skipped
    }
}

void jpegdec_build_huff(const uint8_t counts[16], const uint8_t* val, JdHuff& out) {
    std::memset(&out, 0, sizeof(out));
    std::memcpy(out.val, val, 256);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        out.delta[l] = k - code;
        for (int i = 0; i < counts[l - 1]; ++i, ++code, ++k)
            if (l <= 9)
                for (int x = code << (9 - l); x < (code + 1) << (9 - l); ++x) out.lut[x & 511] = (uint16_t)(l << 8 | val[k & 255]);
        out.maxcode[l] = counts[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    out.maxcode[0] = -1;
}

void jpegdec_build_tables(const JdParsed& p, JdTables& out) {
    std::memset(&out, 0, sizeof(out));
    for (int t = 0; t < 4; ++t) {
        if (p.have_quant[t])
            for (int i = 0; i < 64; ++i) out.q[t][i] = p.quant[t][i];
        if (p.huff[t].have) jpegdec_build_huff(p.huff[t].counts, p.huff[t].val, out.h[t]);
    }
    for (int k = 0; k < 64; ++k) out.zz[k] = ZIGZAG[k];
}

int JdTableSets::add(const JdParsed& p) {
    std::string key;
    for (int t = 0; t < 4; ++t) {
        key.push_back(p.have_quant[t] ? 1 : 0);
        if (p.have_quant[t]) key.append((const char*)p.quant[t], 64);
        key.push_back(p.huff[t].have ? 1 : 0);
        if (p.huff[t].have) key.append((const char*)p.huff[t].counts, 16), key.append((const char*)p.huff[t].val, 256);
    }
    auto it = index.find(key);
    if (it != index.end()) return it->second;
    sets.emplace_back();
    jpegdec_build_tables(p, sets.back());
    return index[key] = (int)sets.size() - 1;
}

void jpegdec_check_config(int device, const aic_jpegdec_config* c) {
    AIC_REQUIRE(c, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device must be >= 0");
    AIC_REQUIRE(c->max_images >= 1 && c->max_images <= JPEGDEC_IMAGES_MAX, AIC_ERR_INVALID, "max_images must be in 1..4096");
    AIC_REQUIRE(c->height >= 1 && c->height <= JPEGDEC_DIM_MAX && c->width >= 1 && c->width <= JPEGDEC_DIM_MAX, AIC_ERR_INVALID,
                "height and width must be in 1..16384");
}

void jpegdec_check_bank(const aic_jpegdec_config& c, const void* files, int files_mem, const int64_t* offsets, int n) {
    AIC_REQUIRE(n >= 0 && n <= c.max_images, AIC_ERR_INVALID, "n must be in 0..max_images");
    AIC_REQUIRE(files_mem == AIC_HOST || files_mem == AIC_DEVICE, AIC_ERR_INVALID, "files_mem must be AIC_HOST or AIC_DEVICE");
    if (n == 0) return;
    AIC_REQUIRE(offsets, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(offsets[0] >= 0, AIC_ERR_INVALID, "offsets must not be negative");
    for (int i = 0; i < n; ++i) {
        AIC_REQUIRE(offsets[i + 1] >= offsets[i], AIC_ERR_INVALID, "offsets must ascend");
        AIC_REQUIRE(offsets[i + 1] - offsets[i] <= JPEGDEC_FILE_MAX, AIC_ERR_INVALID, "a file may take 64 MB at the most");
    }
    AIC_REQUIRE(n == 0 || files || offsets[n] == offsets[0], AIC_ERR_INVALID, "NULL argument");
}

int jpegdec_host_intervals(const uint8_t* ent, int64_t len, int expected, std::vector<int64_t>& lo, std::vector<int64_t>& hi) {
    lo.assign(1, 0), hi.clear();
    bool foreign = false, seq = false;
    for (int64_t p = 0; p < len; ++p) {
        int m = 0;
        const int kind = jd_marker_at(ent, p, len, &m);
        if (kind == 2) foreign = true;
        if (kind == 1) {
            seq |= m != (int)(hi.size() & 7);
            hi.push_back(p), lo.push_back(p + 2);
        }
    }
    hi.push_back(len);
    if (foreign) return JD_BAD_SCAN;
    if ((int64_t)hi.size() != expected || seq) return JD_RESTART_SEQUENCE;
    return 0;
}

int jpegdec_host_decode(const uint8_t* file, int64_t bytes, int height, int width, std::vector<int16_t>& coef, aic_jpegdec_info* info) {
    JdParsed p;
    coef.clear();
    int reason = jpegdec_parse(file, bytes, height, width, p);
    if (!reason) {
        const uint8_t* ent = file + p.info.entropy_offset;
        std::vector<int64_t> lo, hi;
        reason = jpegdec_host_intervals(ent, p.info.entropy_bytes, p.rec.intervals, lo, hi);
        if (!reason) {
            JdTables t;
            jpegdec_build_tables(p, t);
            coef.assign((size_t)p.rec.mcus_x * p.rec.mcus_y * jd_bpm(p.rec) * 64, 0);
            for (int k = 0; k < p.rec.intervals && !reason; ++k) reason = jd_interval(p.rec, t, ent, lo[k], hi[k], k, coef.data());
        }
        if (reason) refuse(p, reason), coef.clear();
    }
    if (info) *info = p.info;
    return reason;
}

}  // namespace aic
