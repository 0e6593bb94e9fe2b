// Test-only program: the HIP-free half of the renderer (ai-camera_amd/csrc/render_host.cpp) built with the system g++ and run stand-alone
// under -fsanitize=address,undefined (tests/test_render_host.py).  It drives the option setter, the mask packer, rows-to-rectangles
// and the list packer at their limits and through every rejection, and checks what they return; exit code 0 and "probe ok" = clean.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ai-camera_amd/csrc/render_host.hpp"

namespace aic {
void set_last_error(const std::string&) {}
}  // namespace aic

using namespace aic;

static int g_checks = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        ++g_checks;                                                      \
        if (!(c)) {                                                      \
            std::printf("probe failed at line %d: %s\n", __LINE__, #c); \
            return 1;                                                    \
        }                                                                \
    } while (0)

template <class F>
static int code_of(F&& f) {
    try {
        f();
        return AIC_OK;
    } catch (const Error& e) {
        return e.code;
    }
}

int main() {
    RenderOptions o;
    // options: the limits and one step past them
    const struct { const char* key; int64_t good_lo, good_hi, bad_lo, bad_hi; } keys[] = {
        {"mode", 0, 2, -1, 3},       {"style", 0, 1, -1, 2},        {"fill_color", 0, 0xffffff, -1, 0x1000000}, {"mask_color", 0, 0xffffff, -1, 0x1000000},
        {"pad", 0, 4096, -1, 4097},  {"head_q8", 1, 256, 0, 257},   {"class_all", 0, 1, -1, 2},                 {"chunk_frames", 0, 65536, -1, 65537}};
    for (const auto& k : keys) {
        CHECK(code_of([&] { render_set_option(o, k.key, k.good_lo); }) == AIC_OK);
        CHECK(code_of([&] { render_set_option(o, k.key, k.good_hi); }) == AIC_OK);
        CHECK(code_of([&] { render_set_option(o, k.key, k.bad_lo); }) == AIC_ERR_INVALID);
        CHECK(code_of([&] { render_set_option(o, k.key, k.bad_hi); }) == AIC_ERR_INVALID);
    }
    for (int c : {4, 8, 16, 32}) CHECK(code_of([&] { render_set_option(o, "cell", c); }) == AIC_OK);
    for (int c : {0, 2, 5, 12, 64, -4}) CHECK(code_of([&] { render_set_option(o, "cell", c); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_set_option(o, "nonsense", 1); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_set_option(o, nullptr, 1); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_check_create(0, 0); }) == AIC_ERR_INVALID && code_of([&] { render_check_create(0, 257); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_check_create(-1, 1); }) == AIC_ERR_INVALID && code_of([&] { render_check_create(0, 256); }) == AIC_OK);

    // rows to rectangles: saturation at INT32 extremes, the head shift at the widest box, a class mask with bit 63
    o = RenderOptions();
    o.mode = RENDER_MODE_HEAD, o.pad = 4096, o.head_q8 = 256;
    const int32_t big = 2147483647, m = 1 << 20;
    std::vector<int32_t> rows = {-big - 1, -big - 1, big, big, 1, 0, 5, 5, 4, 9, 2, 0, 3, 4, 3, 4, 3, 63, 3, 4, 3, 4, 4, 64, 3, 4, 3, 4, 5, -big - 1};
    std::vector<int32_t> out(rows.size() / 6 * 4);
    CHECK(render_rects(o, rows.data(), 5, out.data()) == 4);
    CHECK(out[0] == -m - 4096 && out[1] == -m - 4096 && out[2] == m + 4096 && out[3] == m);
    render_set_option(o, "class_mask", (int64_t)(1ull << 63));
    CHECK(o.class_all == 0 && render_rects(o, rows.data(), 5, out.data()) == 3);          // class 63, and cls 64 / INT32_MIN fail safe
    render_set_option(o, "class_mask", 0);
    CHECK(render_rects(o, rows.data(), 5, out.data()) == 2);
    o.mode = RENDER_MODE_OFF;
    CHECK(render_rects(o, rows.data(), 5, out.data()) == 0 && render_rects(o, nullptr, 0, nullptr) == 0);
    CHECK(code_of([&] { render_rects(o, rows.data(), -1, out.data()); }) == AIC_ERR_INVALID);
    o.mode = RENDER_MODE_BOX;
    CHECK(code_of([&] { render_rects(o, nullptr, 2, out.data()); }) == AIC_ERR_INVALID);

    // masks: 32 polygons of 32 vertices fill the camera's block exactly
    std::vector<int32_t> geo(2 * RENDER_GEO_INTS, -7), nv(32, 32), xy(32 * 32 * 2);
    for (size_t i = 0; i < xy.size(); ++i) xy[i] = (int32_t)((i * 7919) % (2 * m + 1)) - m;
    render_pack_masks(2, 1, 32, nv.data(), xy.data(), geo.data() + RENDER_GEO_INTS);
    CHECK(geo[RENDER_GEO_INTS - 1] == -7 && geo[RENDER_GEO_INTS] == 32 && geo[2 * RENDER_GEO_INTS - 1] == xy.back());
    for (int p = 0; p < 32; ++p) {
        const int32_t* b = geo.data() + RENDER_GEO_INTS + RENDER_GEO_BOX + p * 4;
        for (int i = 0; i < 32; ++i) CHECK(b[0] <= xy[(p * 32 + i) * 2] && xy[(p * 32 + i) * 2] <= b[2] && b[1] <= xy[(p * 32 + i) * 2 + 1] && xy[(p * 32 + i) * 2 + 1] <= b[3]);
    }
    nv[3] = 2;
    CHECK(code_of([&] { render_pack_masks(2, 0, 32, nv.data(), xy.data(), geo.data()); }) == AIC_ERR_INVALID);
    nv[3] = 33;
    CHECK(code_of([&] { render_pack_masks(2, 0, 32, nv.data(), xy.data(), geo.data()); }) == AIC_ERR_INVALID);
    nv[3] = 32, xy[100] = m + 1;
    CHECK(code_of([&] { render_pack_masks(2, 0, 32, nv.data(), xy.data(), geo.data()); }) == AIC_ERR_INVALID && geo[0] == -7);
    CHECK(code_of([&] { render_pack_masks(2, 2, 0, nullptr, nullptr, geo.data()); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_pack_masks(2, 0, 33, nv.data(), xy.data(), geo.data()); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_pack_masks(2, 0, 1, nullptr, xy.data(), geo.data()); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { render_pack_masks(2, 0, 0, nullptr, nullptr, geo.data()); }) == AIC_OK && geo[0] == 0);

    // packing at the per-frame limits: 512 rows and 1500 primitives in the middle frame of three, text of an odd length
    o = RenderOptions();
    o.mode = RENDER_MODE_BOX;
    const int F = 3;
    std::vector<int32_t> rc = {1, 512, 0}, pc = {0, 1500, 2}, r6(513 * 6), pr(1502 * 8, 0), cams = {1, 0, 1};
    for (int i = 0; i < 513; ++i) r6[i * 6] = i, r6[i * 6 + 1] = i, r6[i * 6 + 2] = i + (i % 3) - 1, r6[i * 6 + 3] = i + 2;     // every third row is dropped
    std::vector<uint8_t> text = {'a', 'b', 'c', 'd', 'e'};
    for (int i = 0; i < 1502; ++i) {
        int32_t* p = pr.data() + i * 8;
        p[0] = i % 4;
        if (p[0] == 2) p[6] = i % 5, p[7] = (5 - i % 5) | 2 << 16;
        if (p[0] == 3) p[6] = 1 + i % 8;
    }
    std::vector<uint8_t> frames(F * 2 * 3 * 3);
    char has[2] = {0, 1};
    RenderPacked pk;
    render_pack_frames(o, 2, has, frames.data(), F, 2, 3, AIC_HOST, r6.data(), rc.data(), pr.data(), pc.data(), text.data(), 5, cams.data(), pk);
    const int32_t* b = pk.buf.data();
    CHECK(pk.anything && pk.n_prims == 1502 && pk.n_rects == 342 && b[pk.o_rect_off + 3] == 342 && b[pk.o_prim_off + 1] == 0 && b[pk.o_prim_off + 2] == 1500);
    CHECK(b[pk.o_cam] == 1 && b[pk.o_cam + 1] == 0 && pk.o_rects % 4 == 0 && pk.o_prims % 4 == 0 && pk.buf.size() > pk.o_text + 1);
    CHECK(b[pk.o_prims + 1501 * 8] == 1501 % 4 && reinterpret_cast<const uint8_t*>(b + pk.o_text)[4] == 'e');
    render_pack_frames(o, 2, has, frames.data(), F, 2, 3, AIC_DEVICE, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pk);
    CHECK(pk.anything && pk.n_rects == 0 && pk.buf[pk.o_cam + 1] == 1);      // frame 1 is camera 1 % 2: its masks
    has[1] = 0;
    render_pack_frames(o, 2, has, frames.data(), F, 2, 3, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pk);
    CHECK(!pk.anything);
    render_pack_frames(o, 2, has, nullptr, 0, 2, 3, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, pk);
    CHECK(!pk.anything);

    // every rejection of the packer
    auto pack = [&](int f, int h, int w, int mem, const int32_t* rows6, const int32_t* rcnt, const int32_t* prims, const int32_t* pcnt, const uint8_t* tx, int tb,
                    const int32_t* cm) {
        return code_of([&] { render_pack_frames(o, 2, has, frames.data(), f, h, w, mem, rows6, rcnt, prims, pcnt, tx, tb, cm, pk); });
    };
    CHECK(pack(F, 2, 3, AIC_HOST, r6.data(), rc.data(), pr.data(), pc.data(), text.data(), 5, cams.data()) == AIC_OK);
    CHECK(pack(-1, 2, 3, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(65537, 2, 3, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 0, 3, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 2, 16385, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 2, 3, 2, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, rc.data(), nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, nullptr, pc.data(), nullptr, 0, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), nullptr, 5, nullptr) == AIC_ERR_INVALID);
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), text.data(), 4, nullptr) == AIC_ERR_INVALID);      // a text range past the buffer
    rc[1] = 513;
    CHECK(pack(F, 2, 3, AIC_HOST, r6.data(), rc.data(), nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_CAPACITY);
    rc[1] = -1;
    CHECK(pack(F, 2, 3, AIC_HOST, r6.data(), rc.data(), nullptr, nullptr, nullptr, 0, nullptr) == AIC_ERR_INVALID);
    pc[1] = 1501;
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), text.data(), 5, nullptr) == AIC_ERR_CAPACITY);
    pc[1] = 1500, cams[2] = 2;
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, nullptr, nullptr, nullptr, 0, cams.data()) == AIC_ERR_INVALID);
    pr[0] = 4;
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), text.data(), 5, nullptr) == AIC_ERR_INVALID);
    pr[0] = 0, pr[3 * 8 + 6] = 9;
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), text.data(), 5, nullptr) == AIC_ERR_INVALID);      // thickness 9
    pr[3 * 8 + 6] = 8, pr[8 + 3] = m + 1;
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), text.data(), 5, nullptr) == AIC_ERR_INVALID);      // a coordinate past 2^20
    pr[8 + 3] = m;
    CHECK(pack(F, 2, 3, AIC_HOST, nullptr, nullptr, pr.data(), pc.data(), text.data(), 5, nullptr) == AIC_OK);

    // frames per launch: the block bound and the chunk option
    o.chunk_frames = 0;
    CHECK(render_frames_per_launch(o, 300, 720, 1280) == 300 && render_frames_per_launch(o, 100, 16384, 16384) == 63 && render_frames_per_launch(o, 65536, 1, 1) == 65535);
    o.chunk_frames = 7;
    CHECK(render_frames_per_launch(o, 300, 720, 1280) == 7 && render_frames_per_launch(o, 3, 720, 1280) == 3);
    std::printf("probe ok: %d checks\n", g_checks);
    return 0;
}
