// render_host.hpp -- the HIP-free half of the redaction / annotation stage (render.hpp, C ABI aic_render_*):
// options, every argument check, the rows-to-rectangles step and the packing of a call's lists.  Compiles with plain g++
// (tests/render_host_probe.cpp runs it under the sanitizers); nothing here touches the device.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "assoc_host.hpp"

namespace aic {

constexpr int RENDER_CAMERAS_MAX = 256;
constexpr int RENDER_ROWS_MAX = 512;          // rows (= redaction rectangles) per frame
constexpr int RENDER_PRIMS_MAX = 1500;        // primitives per frame, as aic_overlay
constexpr int RENDER_POLYS_MAX = 32;          // mask polygons per camera
constexpr int RENDER_VERTS_MAX = 32;
constexpr int RENDER_COORD_MAX = 1 << 20;
constexpr int RENDER_DIM_MAX = 16384;         // frame height and width
constexpr int RENDER_FRAMES_MAX = 1 << 16;    // frames per call
constexpr int RENDER_PAD_MAX = 4096;
constexpr int RENDER_TILE_W = 64, RENDER_TILE_H = 32;
constexpr long RENDER_BLOCKS_MAX = (1L << 23) - 1;   // blocks per launch: 256 threads each, the launch stays below 2^31 threads

// mask geometry of one camera, ints: n_polys, 7 unused | n_vert[32] | bounding box [32][4] = x0 y0 x1 y1 | xy [32][32][2]
constexpr int RENDER_GEO_NVERT = 8;
constexpr int RENDER_GEO_BOX = RENDER_GEO_NVERT + RENDER_POLYS_MAX;
constexpr int RENDER_GEO_XY = RENDER_GEO_BOX + RENDER_POLYS_MAX * 4;
constexpr int RENDER_GEO_INTS = RENDER_GEO_XY + RENDER_POLYS_MAX * RENDER_VERTS_MAX * 2;

enum { RENDER_MODE_OFF = 0, RENDER_MODE_BOX = 1, RENDER_MODE_HEAD = 2 };
enum { RENDER_STYLE_FILL = 0, RENDER_STYLE_MOSAIC = 1 };

struct RenderOptions {
    int mode = RENDER_MODE_OFF, style = RENDER_STYLE_MOSAIC, cell = 16;
    int fill_color = 0, mask_color = 0;       // B | G << 8 | R << 16
    int pad = 0, head_q8 = 64;
    int class_all = 1;                        // 1: every row is redacted; 0: rows whose cls bit is set in class_mask, and cls outside 0..63
    uint64_t class_mask = 0;
    int chunk_frames = 0;                     // 0: a call's frames in one device buffer; k: at most k frames per upload / launch / download
};

void render_check_create(int device, int cameras);
void render_set_option(RenderOptions& o, const char* key, int64_t value);
// checks a camera's polygons and writes its RENDER_GEO_INTS ints
void render_pack_masks(int cameras, int camera, int n_polys, const int32_t* n_verts, const int32_t* xy, int32_t* geo);
// rows [n, 6] = x1 y1 x2 y2 id cls -> rects [<= n, 4] = x0 y0 x1 y1 inclusive, in row order; returns their number
int render_rects(const RenderOptions& o, const int32_t* rows6, int n_rows, int32_t* rects4);

// A call's lists, packed for one upload: rect_off[F + 1] | prim_off[F + 1] | camera[F] | rects [n_rects, 4] | prims [n_prims, 8] | text
struct RenderPacked {
    std::vector<int32_t> buf;
    size_t o_rect_off = 0, o_prim_off = 0, o_cam = 0, o_rects = 0, o_prims = 0, o_text = 0;
    int n_rects = 0, n_prims = 0;
    bool anything = false;                    // a rectangle, a primitive, or a mask polygon of a camera a frame names
};
// every argument check of aic_render_frames, then the packing; has_masks[cameras] = the camera has a polygon
void render_pack_frames(const RenderOptions& o, int cameras, const char* has_masks, const void* frames, int n_frames, int h, int w, int mem,
                        const int32_t* rows6, const int32_t* row_counts, const int32_t* prims, const int32_t* prim_counts, const uint8_t* text,
                        int text_bytes, const int32_t* frame_cameras, RenderPacked& out);
// frames per launch for a call of n_frames frames of h x w
int render_frames_per_launch(const RenderOptions& o, int n_frames, int h, int w);

}  // namespace aic
