// jpegdec.cpp -- the JPEG decoder object (jpegdec.hpp) and its C ABI.  Every argument is checked before the device is touched
// (jpegdec_host.cpp); the arithmetic runs in kernels_jpegdec.hip or the call raises.
#include "jpegdec.hpp"
#include "row_stage.hpp"

#include <algorithm>

namespace aic {

void Jpegdec::option(const char* key, int value) {
    AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
    const std::string k(key);
    if (k == "launch_budget_mb") {
        AIC_REQUIRE(value >= 1 && value <= 65536, AIC_ERR_INVALID, "launch_budget_mb must be in 1..65536");
        launch_budget_mb = value;
    } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown JPEG decoder option: " + k);
}

void Jpegdec::decode(const uint8_t* files, int files_mem, const int64_t* offsets, int n, uint8_t* out, int out_mem, int32_t* status, int32_t* reason,
                     int coef_image, int16_t* coef_out) {
    jpegdec_check_bank(cfg, files, files_mem, offsets, n);
    const bool coef_only = coef_image >= 0;
    if (coef_only) AIC_REQUIRE(coef_image < n && coef_out, AIC_ERR_INVALID, "image must be in 0..n-1 and out not NULL");
    else {
        AIC_REQUIRE(out_mem == AIC_HOST || out_mem == AIC_DEVICE, AIC_ERR_INVALID, "out_mem must be AIC_HOST or AIC_DEVICE");
        AIC_REQUIRE(n == 0 || (out && status && reason), AIC_ERR_INVALID, "NULL argument");
    }
    if (n == 0) return;
    const int first = coef_only ? coef_image : 0, last = coef_only ? coef_image + 1 : n;   // the images this call decodes
    const int64_t base = offsets[first], total = offsets[last] - base;
    const size_t frame_bytes = (size_t)cfg.height * cfg.width * 3;

    // the headers are read on the host: files in device memory come over once for that
    const uint8_t* hb = files ? files + base : nullptr;
    if (!dev) dev = &device(device_id);
    dev->use();
    hipStream_t st = dev->s_trk;
    if (files_mem == AIC_DEVICE && total > 0) {
        h_files.resize((size_t)total);
        HIP_CHECK(hipMemcpy(h_files.data(), files + base, (size_t)total, hipMemcpyDeviceToHost));
        hb = h_files.data();
    }
    const int cnt = last - first;
    h_recs.assign(cnt, JdImage{});
    h_err.assign(cnt, JD_ERR_NONE);
    h_ent.assign(cnt, 0);
    sets = JdTableSets{};
    std::vector<int64_t> blocks(cnt, 0);
    {
        JdParsed p;
        for (int i = 0; i < cnt; ++i) {
            const int64_t off = offsets[first + i] - base, len = offsets[first + i + 1] - offsets[first + i];
            const int why = jpegdec_parse(len ? hb + off : nullptr, len, cfg.height, cfg.width, p);
            if (why) { h_err[i] = why; continue; }
            h_recs[i] = p.rec;
            h_recs[i].tabset = sets.add(p);
            h_recs[i].ent_len = p.info.entropy_bytes;
            h_ent[i] = p.info.entropy_offset;
            blocks[i] = (int64_t)p.rec.mcus_x * p.rec.mcus_y * jd_bpm(p.rec);
        }
    }
    if (!sets.sets.empty()) {
        grow(d_tabs, sets.sets.size() * sizeof(JdTables), "the JPEG table sets");
        HIP_CHECK(hipMemcpyAsync(d_tabs.p, sets.sets.data(), sets.sets.size() * sizeof(JdTables), hipMemcpyHostToDevice, st));
    }
    const JdTables* tabs = reinterpret_cast<const JdTables*>(d_tabs.p);
    const int64_t budget = (int64_t)launch_budget_mb << 20;
    for (int lo = 0; lo < cnt;) {
        // the launch [lo, hi): its staged files and its coefficients each stay below the budget, one image at the least
        int hi = lo;
        int64_t n_blk = 0, n_ivl = 0, max_blk = 0;
        int max_ivl = 0;
        const int64_t f0 = offsets[first + lo] - base;
        while (hi < cnt) {
            const int64_t fb = offsets[first + hi + 1] - base - f0;
            if (hi > lo && (fb > budget || (n_blk + blocks[hi]) * 128 > budget)) break;
            JdImage& r = h_recs[hi];
            r.ent_off = offsets[first + hi] - base - f0 + h_ent[hi];
            r.blk_off = n_blk, r.ivl_off = n_ivl;
            n_blk += blocks[hi], n_ivl += r.intervals;
            max_blk = std::max(max_blk, blocks[hi]), max_ivl = std::max(max_ivl, (int)r.intervals);
            ++hi;
        }
        const int k = hi - lo;
        const int64_t fbytes = offsets[first + hi] - base - f0;
        if (max_ivl > 0) {                                                    // else every image of the launch was refused by its header
            const uint8_t* d_f = files + base + f0;
            if (files_mem == AIC_HOST) {
                grow(d_files, (size_t)fbytes, "the staged files");
                HIP_CHECK(hipMemcpyAsync(d_files.p, hb + f0, (size_t)fbytes, hipMemcpyHostToDevice, st));
                d_f = d_files.p;
            }
            grow(d_recs, k, "the image records");
            grow(d_err, k, "the image status");
            grow(d_ivl, (size_t)n_ivl * 2, "the interval table");
            grow(d_coef, (size_t)n_blk * 64, "the coefficients");
            HIP_CHECK(hipMemcpyAsync(d_recs.p, h_recs.data() + lo, (size_t)k * sizeof(JdImage), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(d_err.p, h_err.data() + lo, (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemsetAsync(d_coef.p, 0, (size_t)n_blk * 128, st));
            uint8_t* dst = nullptr;
            {
                Prof pr(*dev, PROF_MISC, st, 0, (double)fbytes + (double)n_blk * 192 + (double)k * frame_bytes);
                launch_jpegdec_markers(d_f, d_recs.p, k, d_err.p, d_ivl.p, d_ivl.p + n_ivl, st);
                launch_jpegdec_entropy(d_f, d_recs.p, k, max_ivl, tabs, d_ivl.p, d_ivl.p + n_ivl, d_err.p, d_coef.p, st);
                if (!coef_only) {
                    grow(d_samples, (size_t)n_blk * 64, "the samples");
                    dst = out + (size_t)lo * frame_bytes;
                    if (out_mem == AIC_HOST) {
                        grow(d_out, (size_t)k * frame_bytes, "the staged frames");
                        dst = d_out.p;
                    }
                    launch_jpegdec_idct(d_recs.p, k, max_blk, tabs, d_err.p, d_coef.p, d_samples.p, st);
                    launch_jpegdec_colour(d_recs.p, k, cfg.height, cfg.width, d_err.p, d_samples.p, dst, st);
                }
            }
            HIP_CHECK(hipMemcpyAsync(h_err.data() + lo, d_err.p, (size_t)k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (coef_only && h_err[lo] == JD_ERR_NONE)
                HIP_CHECK(hipMemcpy(coef_out, d_coef.p, (size_t)n_blk * 128, hipMemcpyDeviceToHost));
            if (!coef_only && out_mem == AIC_HOST) {                           // only the images that were decoded: a refused slot is not written
                for (int a = lo; a < hi;) {
                    if (h_err[a] != JD_ERR_NONE) { ++a; continue; }
                    int b = a;
                    while (b < hi && h_err[b] == JD_ERR_NONE) ++b;
                    HIP_CHECK(hipMemcpyAsync(out + (size_t)a * frame_bytes, d_out.p + (size_t)(a - lo) * frame_bytes, (size_t)(b - a) * frame_bytes,
                                             hipMemcpyDeviceToHost, st));
                    a = b;
                }
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        lo = hi;
    }
    HIP_CHECK(hipStreamSynchronize(st));                                      // the table sets' upload, when no launch followed it
    if (coef_only) {
        const int why = h_err[0] == JD_ERR_NONE ? 0 : (h_err[0] & 255);
        AIC_REQUIRE(!why, AIC_ERR_FORMAT, "the image is refused, reason " + std::to_string(why));
        return;
    }
    for (int i = 0; i < n; ++i) {
        const bool ok = h_err[i] == JD_ERR_NONE;
        status[i] = ok ? AIC_OK : AIC_ERR_FORMAT, reason[i] = ok ? 0 : (h_err[i] & 255);
        n_refused += !ok;
        bytes_out += ok ? (int64_t)frame_bytes : 0;
    }
    n_images += n, bytes_in += total;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_jpegdec_probe(const uint8_t* file, int64_t bytes, aic_jpegdec_info* out) {
    return guarded([&] {
        AIC_REQUIRE(out && bytes >= 0 && (file || bytes == 0), AIC_ERR_INVALID, "NULL argument or negative size");
        AIC_REQUIRE(bytes <= JPEGDEC_FILE_MAX, AIC_ERR_INVALID, "a file may take 64 MB at the most");
        JdParsed p;
        jpegdec_parse(file, bytes, 0, 0, p);
        *out = p.info;
    });
}

int aic_jpegdec_create(int device, const aic_jpegdec_config* config, aic_jpegdec** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        jpegdec_check_config(device, config);
        *out = new aic_jpegdec(device, *config);
    });
}

int aic_jpegdec_destroy(aic_jpegdec* d) {
    return guarded([&] {
        if (d && d->d.dev) { d->d.dev->use(); (void)hipStreamSynchronize(d->d.dev->s_trk); }
        delete d;
    });
}

int aic_jpegdec_option(aic_jpegdec* d, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(d, AIC_ERR_INVALID, "NULL argument");
        d->d.option(key, value);
    });
}

int aic_jpegdec_decode(aic_jpegdec* d, const uint8_t* files, int files_mem, const int64_t* offsets, int n, uint8_t* out_bgr, int out_mem,
                       int32_t* status, int32_t* reason) {
    return guarded([&] {
        AIC_REQUIRE(d, AIC_ERR_INVALID, "NULL argument");
        d->d.decode(files, files_mem, offsets, n, out_bgr, out_mem, status, reason);
    });
}

int aic_jpegdec_coefficients(aic_jpegdec* d, const uint8_t* files, int files_mem, const int64_t* offsets, int n, int image, int16_t* out) {
    return guarded([&] {
        AIC_REQUIRE(d && image >= 0, AIC_ERR_INVALID, "NULL argument or negative image");
        d->d.decode(files, files_mem, offsets, n, nullptr, AIC_HOST, nullptr, nullptr, image, out);
    });
}

int aic_jpegdec_counters(aic_jpegdec* d, int64_t* images, int64_t* refused, int64_t* bytes_in, int64_t* bytes_out) {
    return guarded([&] {
        AIC_REQUIRE(d, AIC_ERR_INVALID, "NULL argument");
        if (images) *images = d->d.n_images;
        if (refused) *refused = d->d.n_refused;
        if (bytes_in) *bytes_in = d->d.bytes_in;
        if (bytes_out) *bytes_out = d->d.bytes_out;
    });
}

}  // extern "C"
