// render_host.cpp -- render_host.hpp: options, argument checks, rows to rectangles, list packing.  HIP-free.
#include "render_host.hpp"

#include <algorithm>
#include <cstring>

namespace aic {

static bool coord_ok(int32_t v) { return v >= -RENDER_COORD_MAX && v <= RENDER_COORD_MAX; }
static int32_t saturate(int32_t v) { return std::min(std::max(v, (int32_t)-RENDER_COORD_MAX), (int32_t)RENDER_COORD_MAX); }

void render_check_create(int device, int cameras) {
    AIC_REQUIRE(device >= 0, AIC_ERR_INVALID, "device id out of range");
    AIC_REQUIRE(cameras >= 1 && cameras <= RENDER_CAMERAS_MAX, AIC_ERR_INVALID, "cameras must be in 1..256");
}

void render_set_option(RenderOptions& o, const char* key, int64_t v) {
    AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
    const std::string k(key);
    if (k == "mode") {
        AIC_REQUIRE(v >= 0 && v <= 2, AIC_ERR_INVALID, "mode: 0 = off, 1 = box, 2 = head");
        o.mode = (int)v;
    } else if (k == "style") {
        AIC_REQUIRE(v == 0 || v == 1, AIC_ERR_INVALID, "style: 0 = fill, 1 = mosaic");
        o.style = (int)v;
    } else if (k == "cell") {
        AIC_REQUIRE(v == 4 || v == 8 || v == 16 || v == 32, AIC_ERR_INVALID, "cell must be 4, 8, 16 or 32");
        o.cell = (int)v;
    } else if (k == "fill_color" || k == "mask_color") {
        AIC_REQUIRE(v >= 0 && v <= 0xffffff, AIC_ERR_INVALID, k + " is B | G << 8 | R << 16 in 0..0xffffff");
        (k == "fill_color" ? o.fill_color : o.mask_color) = (int)v;
    } else if (k == "pad") {
        AIC_REQUIRE(v >= 0 && v <= RENDER_PAD_MAX, AIC_ERR_INVALID, "pad must be in 0..4096");
        o.pad = (int)v;
    } else if (k == "head_q8") {
        AIC_REQUIRE(v >= 1 && v <= 256, AIC_ERR_INVALID, "head_q8 must be in 1..256");
        o.head_q8 = (int)v;
    } else if (k == "class_mask") {                       // bit c = rows of class c are redacted; any 64-bit pattern
        o.class_mask = (uint64_t)v;
        o.class_all = 0;
    } else if (k == "class_all") {
        AIC_REQUIRE(v == 0 || v == 1, AIC_ERR_INVALID, "class_all must be 0 or 1");
        o.class_all = (int)v;
    } else if (k == "chunk_frames") {
        AIC_REQUIRE(v >= 0 && v <= RENDER_FRAMES_MAX, AIC_ERR_INVALID, "chunk_frames: 0 = a call's frames at once, or 1..65536");
        o.chunk_frames = (int)v;
    } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown renderer option: " + k);
}

void render_pack_masks(int cameras, int camera, int n_polys, const int32_t* n_verts, const int32_t* xy, int32_t* geo) {
    AIC_REQUIRE(camera >= 0 && camera < cameras, AIC_ERR_INVALID, "camera outside the renderer");
    AIC_REQUIRE(n_polys >= 0 && n_polys <= RENDER_POLYS_MAX, AIC_ERR_INVALID, "n_polys must be in 0..32");
    AIC_REQUIRE(n_polys == 0 || (n_verts && xy), AIC_ERR_INVALID, "NULL polygon arrays");
    AIC_REQUIRE(geo, AIC_ERR_INVALID, "NULL argument");
    size_t nv = 0;
    for (int p = 0; p < n_polys; ++p) {
        AIC_REQUIRE(n_verts[p] >= 3 && n_verts[p] <= RENDER_VERTS_MAX, AIC_ERR_INVALID, "a mask polygon must have 3..32 vertices");
        nv += n_verts[p];
    }
    for (size_t i = 0; i < 2 * nv; ++i) AIC_REQUIRE(coord_ok(xy[i]), AIC_ERR_INVALID, "a mask coordinate is outside +-2^20");
    std::fill(geo, geo + RENDER_GEO_INTS, 0);
    geo[0] = n_polys;
    const int32_t* v = xy;
    for (int p = 0; p < n_polys; ++p) {
        geo[RENDER_GEO_NVERT + p] = n_verts[p];
        int32_t* box = geo + RENDER_GEO_BOX + p * 4;
        box[0] = box[2] = v[0], box[1] = box[3] = v[1];
        for (int i = 0; i < n_verts[p]; ++i, v += 2) {
            geo[RENDER_GEO_XY + (p * RENDER_VERTS_MAX + i) * 2] = v[0], geo[RENDER_GEO_XY + (p * RENDER_VERTS_MAX + i) * 2 + 1] = v[1];
            box[0] = std::min(box[0], v[0]), box[1] = std::min(box[1], v[1]);
            box[2] = std::max(box[2], v[0]), box[3] = std::max(box[3], v[1]);
        }
    }
}

int render_rects(const RenderOptions& o, const int32_t* rows6, int n_rows, int32_t* rects4) {
    AIC_REQUIRE(n_rows >= 0, AIC_ERR_INVALID, "a negative row count");
    AIC_REQUIRE(n_rows == 0 || (rows6 && rects4), AIC_ERR_INVALID, "NULL argument");
    if (o.mode == RENDER_MODE_OFF) return 0;
    int n = 0;
    for (int i = 0; i < n_rows; ++i) {
        const int32_t* r = rows6 + (size_t)i * 6;
        const int32_t x1 = saturate(r[0]), y1 = saturate(r[1]), x2 = saturate(r[2]), y2 = saturate(r[3]), cls = r[5];
        if (x2 < x1 || y2 < y1) continue;
        if (!o.class_all && cls >= 0 && cls <= 63 && !((o.class_mask >> cls) & 1)) continue;      // an unknown class fails safe: redacted
        int32_t* q = rects4 + (size_t)n++ * 4;
        q[0] = x1 - o.pad, q[1] = y1 - o.pad, q[2] = x2 + o.pad;
        q[3] = o.mode == RENDER_MODE_BOX ? y2 + o.pad : y1 + (int32_t)(((int64_t)(y2 - y1) * o.head_q8) >> 8);
    }
    return n;
}

int render_frames_per_launch(const RenderOptions& o, int n_frames, int h, int w) {
    const long tiles = (long)((w + RENDER_TILE_W - 1) / RENDER_TILE_W) * ((h + RENDER_TILE_H - 1) / RENDER_TILE_H);
    long k = std::min<long>(std::min<long>(n_frames, 65535), std::max<long>(1, RENDER_BLOCKS_MAX / tiles));
    if (o.chunk_frames > 0) k = std::min<long>(k, o.chunk_frames);
    return (int)std::max<long>(k, 1);
}

void render_pack_frames(const RenderOptions& o, int cameras, const char* has_masks, const void* frames, int F, int h, int w, int mem,
                        const int32_t* rows6, const int32_t* row_counts, const int32_t* prims, const int32_t* prim_counts, const uint8_t* text,
                        int text_bytes, const int32_t* frame_cameras, RenderPacked& out) {
    AIC_REQUIRE(F >= 0 && F <= RENDER_FRAMES_MAX, AIC_ERR_INVALID, "n_frames must be in 0..65536");
    AIC_REQUIRE(h >= 1 && h <= RENDER_DIM_MAX && w >= 1 && w <= RENDER_DIM_MAX, AIC_ERR_INVALID, "height and width must be in 1..16384");
    AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(F == 0 || frames, AIC_ERR_INVALID, "NULL frames");
    AIC_REQUIRE(text_bytes >= 0 && (text || text_bytes == 0), AIC_ERR_INVALID, "NULL text");
    long n_rows = 0, n_prims = 0;
    for (int f = 0; f < F; ++f) {
        if (row_counts) {
            AIC_REQUIRE(row_counts[f] >= 0, AIC_ERR_INVALID, "a negative row count");
            AIC_REQUIRE(row_counts[f] <= RENDER_ROWS_MAX, AIC_ERR_CAPACITY, "frame " + std::to_string(f) + " has more than 512 rows");
            n_rows += row_counts[f];
        }
        if (prim_counts) {
            AIC_REQUIRE(prim_counts[f] >= 0, AIC_ERR_INVALID, "a negative primitive count");
            AIC_REQUIRE(prim_counts[f] <= RENDER_PRIMS_MAX, AIC_ERR_CAPACITY, "frame " + std::to_string(f) + " has more than 1500 primitives");
            n_prims += prim_counts[f];
        }
        if (frame_cameras) AIC_REQUIRE(frame_cameras[f] >= 0 && frame_cameras[f] < cameras, AIC_ERR_INVALID, "a frame's camera is outside the renderer");
    }
    AIC_REQUIRE(n_rows == 0 || rows6, AIC_ERR_INVALID, "NULL rows");
    AIC_REQUIRE(n_prims == 0 || prims, AIC_ERR_INVALID, "NULL prims");
    for (long i = 0; i < n_prims; ++i) {
        const int32_t* p = prims + (size_t)i * 8;
        AIC_REQUIRE(p[0] >= 0 && p[0] <= 3, AIC_ERR_INVALID, "unknown primitive kind");
        AIC_REQUIRE(coord_ok(p[1]) && coord_ok(p[2]), AIC_ERR_INVALID, "a primitive coordinate is outside +-2^20");
        if (p[0] != 2) AIC_REQUIRE(coord_ok(p[3]) && coord_ok(p[4]), AIC_ERR_INVALID, "a primitive coordinate is outside +-2^20");
        if (p[0] == 2) AIC_REQUIRE(p[6] >= 0 && (p[7] >> 16) >= 1 && (int64_t)p[6] + (p[7] & 0xffff) <= text_bytes, AIC_ERR_INVALID, "text range outside the buffer");
        if (p[0] == 3) AIC_REQUIRE(p[6] >= 1 && p[6] <= 8, AIC_ERR_INVALID, "segment thickness must be in 1..8");
    }

    const size_t text_ints = ((size_t)text_bytes + 3) / 4;
    out.o_rect_off = 0, out.o_prim_off = (size_t)F + 1, out.o_cam = 2 * ((size_t)F + 1);
    out.o_rects = (out.o_cam + F + 3) / 4 * 4;                          // 16-byte aligned rectangles and primitives
    const size_t rect_cap = o.mode == RENDER_MODE_OFF ? 0 : (size_t)n_rows;
    out.o_prims = out.o_rects + rect_cap * 4;
    out.o_text = out.o_prims + (size_t)n_prims * 8;
    out.buf.assign(out.o_text + text_ints + 1, 0);
    int32_t* b = out.buf.data();
    bool masks = false;
    long row = 0, prim = 0;
    int n_rects = 0;
    for (int f = 0; f < F; ++f) {
        b[out.o_rect_off + f] = n_rects, b[out.o_prim_off + f] = (int32_t)prim;
        const int cam = frame_cameras ? frame_cameras[f] : f % cameras;
        b[out.o_cam + f] = cam;
        masks |= has_masks && has_masks[cam];
        if (row_counts) {
            if (rect_cap) n_rects += render_rects(o, rows6 + (size_t)row * 6, row_counts[f], b + out.o_rects + (size_t)n_rects * 4);
            row += row_counts[f];
        }
        if (prim_counts) prim += prim_counts[f];
    }
    b[out.o_rect_off + F] = n_rects, b[out.o_prim_off + F] = (int32_t)prim;
    if (n_prims) std::memcpy(b + out.o_prims, prims, (size_t)n_prims * 32);
    if (text_bytes) std::memcpy(b + out.o_text, text, (size_t)text_bytes);
    out.n_rects = n_rects, out.n_prims = (int)n_prims;
    out.anything = F > 0 && (n_rects > 0 || n_prims > 0 || masks);
}

}  // namespace aic
