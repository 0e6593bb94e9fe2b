// jpeg.hpp -- JPEG out: a bank of equally sized BGR24 images to complete JFIF files in one call (jpeg.cpp, C ABI aic_jpeg_*;
// kernels_jpeg.hip; the HIP-free half is jpeg_host.hpp).  Baseline sequential DCT, integer arithmetic only --
// tests/jpeg_oracle.py is the specification, bit for bit.
//
// Two passes over the quantised coefficients: the entropy kernel first only measures every restart interval's stuffed size, a scan
// per image turns the sizes into offsets, the host packs the images (max_bytes, out_cap), and the same kernel then writes every byte at
// its final address -- for the images that fit.  Nothing is written for an image that does not fit, or when the bank does not.
//
// Memory, all grown on demand by the first call that needs it: the staged frames of a launch (host frames only), the coefficients of a
// launch (128 bytes per block: 2.0x the frame bytes at 4:4:4, 1.0x at 4:2:0 before padding), 12 bytes per restart interval of the
// call, and the packed output (host output only).  A bank is cut into launches so that the staged frames and the coefficients each
// stay below launch_budget_mb (option, default 1024), one image at the least; with more than one cut the second pass stages and
// transforms each cut again.
#pragma once
#include "common.hpp"
#include "jpeg_host.hpp"

namespace aic {

// kernels_jpeg.hip
// Colour conversion, edge replication, chroma subsampling, both DCT passes and quantisation of n_images images: coef [n_images, n_mcu,
// bpm, 64] int16 in zigzag order.  frames: any alignment.
void launch_jpeg_transform(const uint8_t* frames, int n_images, const JpegGeom& g, const uint32_t* tab, int16_t* coef, hipStream_t s);
// One block per (restart interval, image).  out == nullptr: sizes [n_images, intervals] = the interval's stuffed bytes, nothing else is
// written.  Otherwise image i, when status[i] == 0, goes to out + img_off[i]: the header, every interval at 629 + ivl_off + 2 * index,
// the RSTm markers and EOI.
void launch_jpeg_entropy(const int16_t* coef, int n_images, const JpegGeom& g, const uint32_t* tab, int* sizes, const int64_t* ivl_off,
                         const int64_t* img_off, const int* status, uint8_t* out, hipStream_t s);
// Per image: ivl_off [n_images, intervals] = the exclusive scan of sizes, totals [n_images] = their sum.
void launch_jpeg_scan(const int* sizes, int n_images, const JpegGeom& g, int64_t* ivl_off, int64_t* totals, hipStream_t s);

struct Jpeg {
    int device_id;
    Device* dev = nullptr;                       // resolved by the first call that reaches the device
    aic_jpeg_config cfg;
    JpegGeom g;
    int launch_budget_mb = 1024;
    bool tab_stale = true;                       // quality / restart changed: the next call uploads the tables again
    int64_t n_images = 0, bytes_in = 0, bytes_out = 0;
    DevBuf<uint8_t> d_frames, d_out;
    DevBuf<int16_t> d_coef;
    DevBuf<uint32_t> d_tab;
    DevBuf<int> d_sizes, d_status;
    DevBuf<int64_t> d_ivl, d_tot, d_off;
    std::vector<int64_t> h_tot;
    std::vector<uint32_t> h_tab;

    Jpeg(int device, const aic_jpeg_config& c);
    void option(const char* key, int value);
    void encode(const uint8_t* frames, int frames_mem, int n, uint8_t* out, int out_mem, int64_t out_cap, int64_t* offsets, int32_t* status);
    void coefficients(const uint8_t* frames, int frames_mem, int n, int16_t* out);

private:
    void touch_device();
    int images_per_launch(int frames_mem) const;
    const uint8_t* stage(const uint8_t* frames, int frames_mem, int lo, int hi, hipStream_t st);
};

}  // namespace aic

struct aic_jpeg {
    aic::Jpeg j;
    aic_jpeg(int device, const aic_jpeg_config& c) : j(device, c) {}
};
