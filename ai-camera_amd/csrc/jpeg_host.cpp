// jpeg_host.cpp -- the HIP-free half of the JPEG stage (jpeg_host.hpp): checks, geometry, tables, header, packing.
#include "jpeg_host.hpp"

#include <algorithm>
#include <cstring>

namespace aic {

namespace {

const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
const uint8_t BASE_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61, 12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                               14, 17, 22, 29, 51,  87,  80,  62, 18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t BASE_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3: the 16 code counts by length, then the symbols in code order
const uint8_t DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

struct HuffSpec { const uint8_t* bits; const uint8_t* vals; int n; uint8_t cls_id; };
const HuffSpec HUFF[4] = {{DC_LUMA_BITS, DC_VALS, 12, 0x00}, {AC_LUMA_BITS, AC_LUMA_VALS, 162, 0x10},
                          {DC_CHROMA_BITS, DC_VALS, 12, 0x01}, {AC_CHROMA_BITS, AC_CHROMA_VALS, 162, 0x11}};    // the file's order

// code << 5 | length of every symbol of a table (Annex C); symbols without a code stay 0
void huffman_codes(const HuffSpec& s, uint32_t* out, int n_out) {
    std::fill(out, out + n_out, 0u);
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < s.bits[len - 1]; ++i, ++k, ++code)
            if (s.vals[k] < n_out) out[s.vals[k]] = code << 5 | (uint32_t)len;
        code <<= 1;
    }
}

}  // namespace

void jpeg_check_quality(int quality) { AIC_REQUIRE(quality >= 1 && quality <= 100, AIC_ERR_INVALID, "quality must be in 1..100"); }
void jpeg_check_restart(int restart) {
    AIC_REQUIRE(restart >= 0 && restart <= 65535, AIC_ERR_INVALID, "restart must be in 0..65535 (MCUs per interval; 0 = one MCU row)");
}

JpegGeom jpeg_geometry(int h, int w, int restart, int sub) {
    AIC_REQUIRE(h >= 1 && h <= JPEG_DIM_MAX && w >= 1 && w <= JPEG_DIM_MAX, AIC_ERR_INVALID, "height and width must be in 1..16384");
    jpeg_check_restart(restart);
    AIC_REQUIRE(sub == 420 || sub == 444, AIC_ERR_INVALID, "subsampling must be 420 or 444");
    JpegGeom g;
    g.h = h, g.w = w, g.sub = sub;
    g.mcu = sub == 420 ? 16 : 8, g.bpm = sub == 420 ? 6 : 3;
    g.mcus_x = (w + g.mcu - 1) / g.mcu, g.mcus_y = (h + g.mcu - 1) / g.mcu, g.n_mcu = g.mcus_x * g.mcus_y;
    g.ri = restart ? restart : g.mcus_x;
    g.intervals = (g.n_mcu + g.ri - 1) / g.ri;
    return g;
}

void jpeg_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    jpeg_check_quality(quality);
    AIC_REQUIRE(luma && chroma, AIC_ERR_INVALID, "NULL argument");
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 64; ++i) {
        luma[i] = (uint8_t)std::min(std::max((BASE_LUMA[i] * s + 50) / 100, 1), 255);
        chroma[i] = (uint8_t)std::min(std::max((BASE_CHROMA[i] * s + 50) / 100, 1), 255);
    }
}

void jpeg_header(const JpegGeom& g, int quality, uint8_t out[JPEG_HEADER_BYTES]) {
    uint8_t q[2][64];
    jpeg_tables(quality, q[0], q[1]);
    uint8_t* p = out;
    auto put = [&](std::initializer_list<int> v) { for (int b : v) *p++ = (uint8_t)b; };
    put({0xff, 0xd8});
    put({0xff, 0xe0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int t = 0; t < 2; ++t) {
        put({0xff, 0xdb, 0, 67, t});
        for (int k = 0; k < 64; ++k) *p++ = q[t][ZIGZAG[k]];
    }
    put({0xff, 0xc0, 0, 17, 8, g.h >> 8, g.h & 255, g.w >> 8, g.w & 255, 3, 1, g.sub == 420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (const HuffSpec& s : HUFF) {
        const int n = 2 + 1 + 16 + s.n;
        put({0xff, 0xc4, n >> 8, n & 255, s.cls_id});
        p = std::copy(s.bits, s.bits + 16, p);
        p = std::copy(s.vals, s.vals + s.n, p);
    }
    put({0xff, 0xdd, 0, 4, g.ri >> 8, g.ri & 255});
    put({0xff, 0xda, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    AIC_REQUIRE(p - out == JPEG_HEADER_BYTES, AIC_ERR_RUNTIME, "the JPEG header is not 629 bytes");
}

void jpeg_device_tables(const JpegGeom& g, int quality, std::vector<uint32_t>& words) {
    words.assign(JPEG_TAB_WORDS, 0u);
    uint8_t hdr[JPEG_TAB_HEADER * 4] = {0};
    jpeg_header(g, quality, hdr);
    std::memcpy(words.data(), hdr, sizeof hdr);
    uint8_t q[2][64];
    jpeg_tables(quality, q[0], q[1]);
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const uint64_t d = 8u * q[t][i];
            words[JPEG_TAB_RCP + t * 64 + i] = (uint32_t)(((1ull << 32) + d - 1) / d);   // exact for |F| + 4 Q < 2^32 / d: F stays below 2^15
            words[JPEG_TAB_ADD + t * 64 + i] = 4u * q[t][i];
        }
    huffman_codes(HUFF[0], &words[JPEG_TAB_DC], 16);
    huffman_codes(HUFF[2], &words[JPEG_TAB_DC + 16], 16);
    huffman_codes(HUFF[1], &words[JPEG_TAB_AC], 256);
    huffman_codes(HUFF[3], &words[JPEG_TAB_AC + 256], 256);
    uint8_t zz[64];
    for (int k = 0; k < 64; ++k) zz[ZIGZAG[k]] = (uint8_t)k;
    std::memcpy(&words[JPEG_TAB_ZZ], zz, sizeof zz);
}

int64_t jpeg_default_max_bytes(const JpegGeom& g) {
    return JPEG_HEADER_BYTES + 3ll * g.mcus_x * g.mcu * g.mcus_y * g.mcu + 2ll * g.intervals + 2;
}

int64_t jpeg_worst_case_bytes(const JpegGeom& g) {
    return JPEG_HEADER_BYTES + (int64_t)JPEG_BLOCK_WORST * g.bpm * g.n_mcu + 2ll * g.intervals + 2;
}

void jpeg_check_config(int device, const aic_jpeg_config* c) {
    AIC_REQUIRE(c, AIC_ERR_INVALID, "NULL argument");
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(c->max_images >= 1 && c->max_images <= JPEG_IMAGES_MAX, AIC_ERR_INVALID, "max_images must be in 1..4096");
    jpeg_check_quality(c->quality);
    (void)jpeg_geometry(c->height, c->width, c->restart, c->subsampling);
    AIC_REQUIRE(c->max_bytes == 0 || c->max_bytes >= JPEG_HEADER_BYTES + 2, AIC_ERR_INVALID,
                "max_bytes must be 0 (the default for the configuration) or at least 631");
}

void jpeg_check_encode(const aic_jpeg_config& c, const void* frames, int frames_mem, int n, const void* out, int out_mem, int64_t out_cap,
                       const int64_t* offsets, const int32_t* status) {
    AIC_REQUIRE(n >= 0 && n <= c.max_images, AIC_ERR_INVALID, "n must be in 0..max_images");
    AIC_REQUIRE(frames_mem == AIC_HOST || frames_mem == AIC_DEVICE, AIC_ERR_INVALID, "frames_mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(out_mem == AIC_HOST || out_mem == AIC_DEVICE, AIC_ERR_INVALID, "out_mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(out_cap >= 0, AIC_ERR_INVALID, "a negative out_cap");
    AIC_REQUIRE(offsets && status, AIC_ERR_INVALID, "NULL offsets or status");
    AIC_REQUIRE(n == 0 || frames, AIC_ERR_INVALID, "NULL frames");
    AIC_REQUIRE(out_cap == 0 || out, AIC_ERR_INVALID, "NULL out");
}

int64_t jpeg_pack(const int64_t* entropy_bytes, int n, const JpegGeom& g, int64_t max_bytes, int64_t* offsets, int32_t* status) {
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t size = JPEG_HEADER_BYTES + entropy_bytes[i] + 2ll * (g.intervals - 1) + 2;
        const bool fits = size <= max_bytes;
        offsets[i] = at, status[i] = fits ? AIC_OK : AIC_ERR_CAPACITY;
        if (fits) at += size;
    }
    offsets[n] = at;
    return at;
}

}  // namespace aic
