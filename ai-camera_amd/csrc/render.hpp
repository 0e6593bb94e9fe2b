// render.hpp -- privacy redaction, static masks and annotation of a bank of frames in one launch (render.cpp, C ABI aic_render_*;
// kernels_render.hip).  A tracker-agnostic stage after the path: a batch of u8 BGR frames, the rows every tracker
// here delivers (x1 y1 x2 y2 id cls, int32) and per-camera mask polygons; tests/render_oracle.py is the specification, bit for bit.
//
// A call costs one upload of the packed lists, then per chunk of frames one upload, one launch and one download (host frames) or the
// launch alone (device frames, in place), and one stream synchronise.  The handle owns its buffers and grows them.  The options, the
// argument checks and the packing live in render_host.hpp, HIP-free; the device is first touched by a call that has something to draw.
#pragma once
#include "common.hpp"
#include "render_host.hpp"

namespace aic {

// kernels_render.hip: frames [n_frames, h, w, 3] in place; rect_off / prim_off / cam are the launch's first frame's entries, their
// offsets absolute into rects [.., 4] and prims [.., 8]; geo [cameras][RENDER_GEO_INTS]
void launch_render_tiles(unsigned char* frames, int n_frames, int h, int w, const int* rect_off, const int* prim_off, const int* cam, const int* rects,
                         const int* prims, const unsigned char* text, const int* geo, int style, int cell, int fill_color, int mask_color,
                         hipStream_t s);

struct Render {
    int device_id, n_cameras;
    Device* dev = nullptr;                       // resolved by the first call that draws
    RenderOptions opt;
    std::vector<int32_t> h_geo;                  // [cameras][RENDER_GEO_INTS]
    std::vector<char> has_masks;
    bool geo_dirty = true;
    RenderPacked packed;
    DevBuf<int> d_geo, d_lists;
    DevBuf<uint8_t> d_frames;

    Render(int device, int cameras) : device_id(device), n_cameras(cameras), h_geo((size_t)cameras * RENDER_GEO_INTS, 0), has_masks(cameras, 0) {}
    void set_masks(int camera, int n_polys, const int32_t* n_verts, const int32_t* xy);
    void frames(uint8_t* frames_bgr, int n_frames, int h, int w, int mem, const int32_t* rows6, const int32_t* row_counts, const int32_t* prims,
                const int32_t* prim_counts, const uint8_t* text, int text_bytes, const int32_t* cameras);
};

}  // namespace aic

struct aic_render {
    aic::Render r;
    aic_render(int device, int cameras) : r(device, cameras) {}
};
