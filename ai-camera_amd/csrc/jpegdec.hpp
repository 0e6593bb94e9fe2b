// jpegdec.hpp -- JPEG in: a bank of JPEG files of one picture size to [n, height, width, 3] BGR24 in one call (jpegdec.cpp, C ABI
// aic_jpegdec_*; kernels_jpegdec.hip; the HIP-free half is jpegdec_host.hpp, the bit reader and block decoder jpegdec_decode.hpp;
// DESIGN.md section 43).  Baseline sequential DCT, integer arithmetic only -- tests/jpegdec_oracle.py is the specification, byte for byte.
//
// The host parses every file's segments up to SOS into a fixed-size record and deduplicates the table sets; on the device the markers
// kernel finds every image's restart intervals, the entropy kernel decodes one interval per lane into int16 coefficients, the IDCT
// kernel turns them into u8 samples block by block, and the colour kernel upsamples, converts and writes tight BGR24.  An image that
// any step refuses carries its reason in its error word and is skipped by the steps after it; its output slot is never written.
//
// Memory, all grown on demand: the staged files of a launch (host files only), the coefficients (128 bytes per block) and the samples
// (64 bytes per block) of a launch, 16 bytes per restart interval, and the staged output (host output only).  A bank is cut into
// launches so that the staged files and the coefficients each stay below launch_budget_mb (option, default 1024), one image at the least.
#pragma once
#include "common.hpp"
#include "jpegdec_host.hpp"

namespace aic {

// kernels_jpegdec.hip.  files: the launch's first file byte (any alignment); recs / err [n_images]; err[i] == JD_ERR_NONE: image i is
// still good, anything else: every kernel leaves it alone.
// The restart intervals of every image: ivl_lo / ivl_hi [rec.ivl_off + k] = the bytes of interval k within the image's entropy data;
// a marker that is no RSTm is JD_BAD_SCAN, a wrong count or sequence JD_RESTART_SEQUENCE.
void launch_jpegdec_markers(const uint8_t* files, const JdImage* recs, int n_images, int32_t* err, int64_t* ivl_lo, int64_t* ivl_hi, hipStream_t s);
// One lane per restart interval: coef [blocks of the launch, 64] int16 in natural order, zero before the launch.
void launch_jpegdec_entropy(const uint8_t* files, const JdImage* recs, int n_images, int max_intervals, const JdTables* tabs, const int64_t* ivl_lo,
                            const int64_t* ivl_hi, int32_t* err, int16_t* coef, hipStream_t s);
// Dequantisation and libjpeg's ISLOW inverse DCT: samples [blocks of the launch, 8, 8] u8.
void launch_jpegdec_idct(const JdImage* recs, int n_images, int64_t max_blocks, const JdTables* tabs, const int32_t* err, const int16_t* coef,
                         uint8_t* samples, hipStream_t s);
// Upsampling and colour: image i to out + i * h * w * 3 (any alignment), only bytes inside the picture.
void launch_jpegdec_colour(const JdImage* recs, int n_images, int h, int w, const int32_t* err, const uint8_t* samples, uint8_t* out, hipStream_t s);

struct Jpegdec {
    int device_id;
    Device* dev = nullptr;                       // resolved by the first call that reaches the device
    aic_jpegdec_config cfg;
    int launch_budget_mb = 1024;
    int64_t n_images = 0, n_refused = 0, bytes_in = 0, bytes_out = 0;
    DevBuf<uint8_t> d_files, d_out, d_samples, d_tabs;
    DevBuf<int16_t> d_coef;
    DevBuf<JdImage> d_recs;
    DevBuf<int32_t> d_err;
    DevBuf<int64_t> d_ivl;
    std::vector<uint8_t> h_files;
    std::vector<JdImage> h_recs;
    std::vector<int32_t> h_err;
    std::vector<int64_t> h_ent;                  // entropy_offset of every image within its file
    JdTableSets sets;

    Jpegdec(int device, const aic_jpegdec_config& c) : device_id(device), cfg(c) {}
    void option(const char* key, int value);
    // out_mem AIC_HOST / AIC_DEVICE; coef_image >= 0: stop after the entropy kernel and copy that image's coefficients to coef_out
    void decode(const uint8_t* files, int files_mem, const int64_t* offsets, int n, uint8_t* out, int out_mem, int32_t* status, int32_t* reason,
                int coef_image = -1, int16_t* coef_out = nullptr);
};

}  // namespace aic

struct aic_jpegdec {
    aic::Jpegdec d;
    aic_jpegdec(int device, const aic_jpegdec_config& c) : d(device, c) {}
};
