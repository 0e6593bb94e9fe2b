// jpeg.cpp -- the JPEG encoder object (jpeg.hpp) and its C ABI.  Every argument is checked before the device is touched (jpeg_host.cpp);
// the arithmetic runs in kernels_jpeg.hip or the call raises.
#include "jpeg.hpp"
#include "row_stage.hpp"

#include <algorithm>

namespace aic {

Jpeg::Jpeg(int device, const aic_jpeg_config& c) : device_id(device), cfg(c), g(jpeg_geometry(c.height, c.width, c.restart, c.subsampling)) {
    if (cfg.max_bytes == 0) cfg.max_bytes = jpeg_default_max_bytes(g);
}

void Jpeg::option(const char* key, int value) {
    AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
    const std::string k(key);
    if (k == "quality") {
        jpeg_check_quality(value);
        cfg.quality = value, tab_stale = true;
    } else if (k == "restart") {
        g = jpeg_geometry(cfg.height, cfg.width, value, cfg.subsampling);
        cfg.restart = value, tab_stale = true;
    } else if (k == "launch_budget_mb") {
        AIC_REQUIRE(value >= 1 && value <= 65536, AIC_ERR_INVALID, "launch_budget_mb must be in 1..65536");
        launch_budget_mb = value;
    } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown JPEG option: " + k);
}

void Jpeg::touch_device() {
    if (!dev) dev = &device(device_id);
    dev->use();
    if (tab_stale) {
        jpeg_device_tables(g, cfg.quality, h_tab);
        grow(d_tab, h_tab.size(), "the JPEG tables");
        HIP_CHECK(hipMemcpyAsync(d_tab.p, h_tab.data(), h_tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, dev->s_trk));
        HIP_CHECK(hipStreamSynchronize(dev->s_trk));                          // h_tab may be rebuilt by the next option
        tab_stale = false;
    }
}

int Jpeg::images_per_launch(int frames_mem) const {
    const size_t budget = (size_t)launch_budget_mb << 20, coef_bytes = (size_t)g.n_mcu * g.bpm * 128, frame_bytes = (size_t)g.h * g.w * 3;
    size_t k = budget / coef_bytes;
    if (frames_mem == AIC_HOST) k = std::min(k, budget / frame_bytes);
    return (int)std::min<size_t>(std::max<size_t>(k, 1), JPEG_IMAGES_MAX);
}

// the launch's images [lo, hi) on the device, and their coefficients
const uint8_t* Jpeg::stage(const uint8_t* frames, int frames_mem, int lo, int hi, hipStream_t st) {
    const size_t frame_bytes = (size_t)g.h * g.w * 3;
    const uint8_t* d_fr = frames + (size_t)lo * frame_bytes;
    if (frames_mem == AIC_HOST) {
        grow(d_frames, (size_t)(hi - lo) * frame_bytes, "the staged frames");
        HIP_CHECK(hipMemcpyAsync(d_frames.p, d_fr, (size_t)(hi - lo) * frame_bytes, hipMemcpyHostToDevice, st));
        d_fr = d_frames.p;
    }
    grow(d_coef, (size_t)(hi - lo) * g.n_mcu * g.bpm * 64, "the coefficients");
    launch_jpeg_transform(d_fr, hi - lo, g, d_tab.p, d_coef.p, st);
    return d_fr;
}

void Jpeg::encode(const uint8_t* frames, int frames_mem, int n, uint8_t* out, int out_mem, int64_t out_cap, int64_t* offsets, int32_t* status) {
    jpeg_check_encode(cfg, frames, frames_mem, n, out, out_mem, out_cap, offsets, status);
    offsets[0] = 0;
    if (n == 0) return;
    touch_device();
    hipStream_t st = dev->s_trk;
    const int per = images_per_launch(frames_mem);
    const size_t n_ivl = (size_t)n * g.intervals;
    grow(d_sizes, n_ivl, "the interval sizes");
    grow(d_ivl, n_ivl, "the interval offsets");
    grow(d_tot, n, "the image sizes");
    {
        Prof pr(*dev, PROF_MISC, st, 0, (double)n * g.h * g.w * 3);
        for (int lo = 0; lo < n; lo += per) {                                 // pass 1: the stuffed size of every interval
            const int hi = std::min(n, lo + per);
            stage(frames, frames_mem, lo, hi, st);
            launch_jpeg_entropy(d_coef.p, hi - lo, g, d_tab.p, d_sizes.p + (size_t)lo * g.intervals, nullptr, nullptr, nullptr, nullptr, st);
        }
        launch_jpeg_scan(d_sizes.p, n, g, d_ivl.p, d_tot.p, st);
    }
    h_tot.resize(n);
    HIP_CHECK(hipMemcpyAsync(h_tot.data(), d_tot.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    const int64_t total = jpeg_pack(h_tot.data(), n, g, cfg.max_bytes, offsets, status);
    n_images += n, bytes_in += (int64_t)n * g.h * g.w * 3;
    AIC_REQUIRE(total <= out_cap, AIC_ERR_CAPACITY,
                "the packed files take " + std::to_string(total) + " bytes, out_cap is " + std::to_string(out_cap) + " (offsets are filled)");
    if (total == 0) return;
    grow(d_off, (size_t)n + 1, "the image offsets");
    grow(d_status, n, "the image status");
    HIP_CHECK(hipMemcpyAsync(d_off.p, offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(d_status.p, status, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
    uint8_t* dst = out;
    if (out_mem == AIC_HOST) {
        grow(d_out, (size_t)total, "the packed files");
        dst = d_out.p;
    }
    {
        Prof pr(*dev, PROF_MISC, st, 0, (double)total);
        for (int lo = 0; lo < n; lo += per) {                                 // pass 2: every byte at its final address
            const int hi = std::min(n, lo + per);
            if (per < n) stage(frames, frames_mem, lo, hi, st);                // one launch: its coefficients are still there
            launch_jpeg_entropy(d_coef.p, hi - lo, g, d_tab.p, nullptr, d_ivl.p + (size_t)lo * g.intervals, d_off.p + lo, d_status.p + lo, dst, st);
        }
    }
    if (out_mem == AIC_HOST) HIP_CHECK(hipMemcpyAsync(out, d_out.p, (size_t)total, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    bytes_out += total;
}

void Jpeg::coefficients(const uint8_t* frames, int frames_mem, int n, int16_t* out) {
    AIC_REQUIRE(n >= 0 && n <= cfg.max_images, AIC_ERR_INVALID, "n must be in 0..max_images");
    AIC_REQUIRE(frames_mem == AIC_HOST || frames_mem == AIC_DEVICE, AIC_ERR_INVALID, "frames_mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(n == 0 || (frames && out), AIC_ERR_INVALID, "NULL argument");
    if (n == 0) return;
    touch_device();
    hipStream_t st = dev->s_trk;
    const int per = images_per_launch(frames_mem);
    const size_t image_coefs = (size_t)g.n_mcu * g.bpm * 64;
    for (int lo = 0; lo < n; lo += per) {
        const int hi = std::min(n, lo + per);
        stage(frames, frames_mem, lo, hi, st);
        HIP_CHECK(hipMemcpyAsync(out + (size_t)lo * image_coefs, d_coef.p, (size_t)(hi - lo) * image_coefs * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_jpeg_tables(int quality, uint8_t luma[64], uint8_t chroma[64]) {
    return guarded([&] { jpeg_tables(quality, luma, chroma); });
}

int aic_jpeg_header(int height, int width, int quality, int restart, int subsampling, uint8_t* out, int cap, int* n) {
    return guarded([&] {
        AIC_REQUIRE(out && n, AIC_ERR_INVALID, "NULL argument");
        jpeg_check_quality(quality);
        const JpegGeom g = jpeg_geometry(height, width, restart, subsampling);
        *n = JPEG_HEADER_BYTES;
        AIC_REQUIRE(cap >= JPEG_HEADER_BYTES, AIC_ERR_CAPACITY, "the header takes 629 bytes");
        jpeg_header(g, quality, out);
    });
}

int aic_jpeg_config_default(int height, int width, aic_jpeg_config* out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        *out = aic_jpeg_config{16, height, width, 85, 0, 420, 0};
        out->max_bytes = jpeg_default_max_bytes(jpeg_geometry(height, width, 0, 420));
    });
}

int aic_jpeg_create(int device, const aic_jpeg_config* config, aic_jpeg** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        jpeg_check_config(device, config);
        *out = new aic_jpeg(device, *config);
    });
}

int aic_jpeg_destroy(aic_jpeg* j) {
    return guarded([&] {
        if (j && j->j.dev) { j->j.dev->use(); (void)hipStreamSynchronize(j->j.dev->s_trk); }
        delete j;
    });
}

int aic_jpeg_option(aic_jpeg* j, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(j, AIC_ERR_INVALID, "NULL argument");
        j->j.option(key, value);
    });
}

int aic_jpeg_worst_case_bytes(aic_jpeg* j, int64_t* bytes) {
    return guarded([&] {
        AIC_REQUIRE(j && bytes, AIC_ERR_INVALID, "NULL argument");
        *bytes = jpeg_worst_case_bytes(j->j.g);
    });
}

int aic_jpeg_encode(aic_jpeg* j, const uint8_t* frames_bgr, int frames_mem, int n, uint8_t* out, int out_mem, int64_t out_cap, int64_t* offsets,
                    int32_t* status) {
    return guarded([&] {
        AIC_REQUIRE(j, AIC_ERR_INVALID, "NULL argument");
        j->j.encode(frames_bgr, frames_mem, n, out, out_mem, out_cap, offsets, status);
    });
}

int aic_jpeg_coefficients(aic_jpeg* j, const uint8_t* frames_bgr, int frames_mem, int n, int16_t* out) {
    return guarded([&] {
        AIC_REQUIRE(j, AIC_ERR_INVALID, "NULL argument");
        j->j.coefficients(frames_bgr, frames_mem, n, out);
    });
}

int aic_jpeg_counters(aic_jpeg* j, int64_t* images, int64_t* bytes_in, int64_t* bytes_out) {
    return guarded([&] {
        AIC_REQUIRE(j, AIC_ERR_INVALID, "NULL argument");
        if (images) *images = j->j.n_images;
        if (bytes_in) *bytes_in = j->j.bytes_in;
        if (bytes_out) *bytes_out = j->j.bytes_out;
    });
}

}  // extern "C"
