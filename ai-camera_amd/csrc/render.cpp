// render.cpp -- the redaction / annotation object (render.hpp) and its C ABI.  Every argument is checked in render_host.cpp before the
// device is touched; the pixels are written by kernels_render.hip or the call raises.
#include "render.hpp"

#include <algorithm>

namespace aic {

void Render::set_masks(int camera, int n_polys, const int32_t* n_verts, const int32_t* xy) {
    std::vector<int32_t> g(RENDER_GEO_INTS);
    render_pack_masks(n_cameras, camera, n_polys, n_verts, xy, g.data());          // throws before anything is changed
    std::copy(g.begin(), g.end(), h_geo.begin() + (size_t)camera * RENDER_GEO_INTS);
    has_masks[camera] = n_polys > 0;
    geo_dirty = true;
}

void Render::frames(uint8_t* frames_bgr, int F, int h, int w, int mem, const int32_t* rows6, const int32_t* row_counts, const int32_t* prims,
                    const int32_t* prim_counts, const uint8_t* text, int text_bytes, const int32_t* cameras) {
    render_pack_frames(opt, n_cameras, has_masks.data(), frames_bgr, F, h, w, mem, rows6, row_counts, prims, prim_counts, text, text_bytes, cameras, packed);
    if (!packed.anything) return;                 // nothing to draw: the frames stay as they are, wherever they live
    if (!dev) dev = &device(device_id);
    dev->use();
    hipStream_t st = dev->s_main;
    if (geo_dirty) {
        d_geo.ensure(h_geo.size());
        HIP_CHECK(hipMemcpyAsync(d_geo.p, h_geo.data(), h_geo.size() * sizeof(int), hipMemcpyHostToDevice, st));
    }
    d_lists.ensure(packed.buf.size());
    HIP_CHECK(hipMemcpyAsync(d_lists.p, packed.buf.data(), packed.buf.size() * sizeof(int), hipMemcpyHostToDevice, st));
    const int* L = d_lists.p;
    const size_t fb = (size_t)h * w * 3;
    const int step = render_frames_per_launch(opt, F, h, w);
    if (mem == AIC_HOST) d_frames.ensure((size_t)step * fb);
    for (int f0 = 0; f0 < F; f0 += step) {
        const int n = std::min(step, F - f0);
        uint8_t* target = mem == AIC_HOST ? d_frames.p : frames_bgr + (size_t)f0 * fb;
        if (mem == AIC_HOST) HIP_CHECK(hipMemcpyAsync(target, frames_bgr + (size_t)f0 * fb, (size_t)n * fb, hipMemcpyHostToDevice, st));
        launch_render_tiles(target, n, h, w, L + packed.o_rect_off + f0, L + packed.o_prim_off + f0, L + packed.o_cam + f0, L + packed.o_rects,
                            L + packed.o_prims, reinterpret_cast<const unsigned char*>(L + packed.o_text), d_geo.p, opt.style, opt.cell,
                            opt.fill_color, opt.mask_color, st);
        if (mem == AIC_HOST) HIP_CHECK(hipMemcpyAsync(frames_bgr + (size_t)f0 * fb, target, (size_t)n * fb, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    geo_dirty = false;
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_render_create(int device_id, int cameras, aic_render** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        render_check_create(device_id, cameras);
        *out = new aic_render(device_id, cameras);
    });
}

int aic_render_destroy(aic_render* r) {
    return guarded([&] {
        if (r && r->r.dev) { r->r.dev->use(); (void)hipStreamSynchronize(r->r.dev->s_main); }
        delete r;
    });
}

int aic_render_option(aic_render* r, const char* key, int64_t value) {
    return guarded([&] {
        AIC_REQUIRE(r && key, AIC_ERR_INVALID, "NULL argument");
        render_set_option(r->r.opt, key, value);
    });
}

int aic_render_set_masks(aic_render* r, int camera, int n_polys, const int32_t* n_verts, const int32_t* xy) {
    return guarded([&] {
        AIC_REQUIRE(r, AIC_ERR_INVALID, "NULL argument");
        r->r.set_masks(camera, n_polys, n_verts, xy);
    });
}

int aic_render_rects(aic_render* r, const int32_t* rows6, int n_rows, int32_t* rects4, int* n_rects) {
    return guarded([&] {
        AIC_REQUIRE(r && n_rects, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(n_rows <= RENDER_ROWS_MAX, AIC_ERR_CAPACITY, "more than 512 rows");
        *n_rects = render_rects(r->r.opt, rows6, n_rows, rects4);
    });
}

int aic_render_frames(aic_render* r, uint8_t* frames_bgr, int n_frames, int h, int w, int mem, const int32_t* rows6, const int32_t* row_counts,
                      const int32_t* prims, const int32_t* prim_counts, const uint8_t* text, int text_bytes, const int32_t* cameras) {
    return guarded([&] {
        AIC_REQUIRE(r, AIC_ERR_INVALID, "NULL argument");
        r->r.frames(frames_bgr, n_frames, h, w, mem, rows6, row_counts, prims, prim_counts, text, text_bytes, cameras);
    });
}

}  // extern "C"
