// jpeg_host.hpp -- the HIP-free half of the JPEG stage (jpeg_host.cpp; jpeg.hpp has the device half): the
// argument checks, the geometry, the quantisation and Huffman tables, the 629 header bytes and the packing of a bank's files.
// Compiles with plain g++ (tests/jpeg_host_probe.cpp runs it under the sanitizers).
#pragma once
#include <vector>

#include "assoc_host.hpp"

namespace aic {

constexpr int JPEG_IMAGES_MAX = 4096;
constexpr int JPEG_DIM_MAX = 16384;
constexpr int JPEG_HEADER_BYTES = 629;
constexpr int JPEG_BLOCK_WORST = 416;      // stuffed bytes of one block at the most: (20 + 63 * 26) bits, every byte 0xFF

struct JpegGeom {                          // what the kernels need of a configuration
    int h, w, sub;                         // sub: 420 / 444
    int mcu, bpm;                          // MCU side in pixels (16 / 8), blocks per MCU (6 / 3)
    int mcus_x, mcus_y, n_mcu;
    int ri, intervals;                     // MCUs per restart interval, intervals per image
};

// The device's tables, one upload per (size, quality, restart, subsampling), uint32 words:
// header (JPEG_TAB_HEADER words, 629 bytes) | rcp[2][64] | add[2][64] | dc[2][16] | ac[2][256] | zz (64 bytes)
// rcp / add in natural order: coef = sign(F) * umulhi(|F| + add, rcp), add = 4 Q, rcp = ceil(2^32 / (8 Q)); dc / ac = code << 5 | length;
// zz = the zigzag position of a natural index.
constexpr int JPEG_TAB_HEADER = 160;
constexpr int JPEG_TAB_RCP = JPEG_TAB_HEADER, JPEG_TAB_ADD = JPEG_TAB_RCP + 128, JPEG_TAB_DC = JPEG_TAB_ADD + 128, JPEG_TAB_AC = JPEG_TAB_DC + 32;
constexpr int JPEG_TAB_ZZ = JPEG_TAB_AC + 512, JPEG_TAB_WORDS = JPEG_TAB_ZZ + 16;

void jpeg_check_quality(int quality);
void jpeg_check_restart(int restart);
JpegGeom jpeg_geometry(int h, int w, int restart, int sub);                  // checks h, w, restart, sub
void jpeg_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);         // natural order
void jpeg_header(const JpegGeom& g, int quality, uint8_t out[JPEG_HEADER_BYTES]);
void jpeg_device_tables(const JpegGeom& g, int quality, std::vector<uint32_t>& words);
int64_t jpeg_default_max_bytes(const JpegGeom& g);
int64_t jpeg_worst_case_bytes(const JpegGeom& g);
void jpeg_check_config(int device, const aic_jpeg_config* c);
void jpeg_check_encode(const aic_jpeg_config& c, const void* frames, int frames_mem, int n, const void* out, int out_mem, int64_t out_cap,
                       const int64_t* offsets, const int32_t* status);
// sizes[n] = entropy bytes of every image (its intervals, stuffed) -> status[n] (0 / AIC_ERR_CAPACITY) and offsets[n + 1]; returns the total
int64_t jpeg_pack(const int64_t* entropy_bytes, int n, const JpegGeom& g, int64_t max_bytes, int64_t* offsets, int32_t* status);

}  // namespace aic
