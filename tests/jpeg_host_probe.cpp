// Test-only program: the HIP-free half of the JPEG stage (ai-camera_amd/csrc/jpeg_host.cpp) built with the system g++ and run stand-alone
// under -fsanitize=address,undefined (tests/test_jpeg_host.py).  It drives the geometry, the tables, the header, the device's table
// words and the packer at their limits and through every rejection, and checks what they return; exit code 0 and "probe ok" = clean.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../ai-camera_amd/csrc/jpeg_host.hpp"

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
    // geometry: the limits and one step past them
    for (int sub : {420, 444}) {
        CHECK(code_of([&] { jpeg_geometry(1, 1, 0, sub); }) == AIC_OK && code_of([&] { jpeg_geometry(16384, 16384, 65535, sub); }) == AIC_OK);
        CHECK(code_of([&] { jpeg_geometry(0, 1, 0, sub); }) == AIC_ERR_INVALID && code_of([&] { jpeg_geometry(1, 16385, 0, sub); }) == AIC_ERR_INVALID);
        CHECK(code_of([&] { jpeg_geometry(8, 8, -1, sub); }) == AIC_ERR_INVALID && code_of([&] { jpeg_geometry(8, 8, 65536, sub); }) == AIC_ERR_INVALID);
    }
    CHECK(code_of([&] { jpeg_geometry(8, 8, 0, 422); }) == AIC_ERR_INVALID && code_of([&] { jpeg_geometry(8, 8, 0, 0); }) == AIC_ERR_INVALID);
    JpegGeom g = jpeg_geometry(17, 33, 0, 420);
    CHECK(g.mcu == 16 && g.bpm == 6 && g.mcus_x == 3 && g.mcus_y == 2 && g.n_mcu == 6 && g.ri == 3 && g.intervals == 2);
    g = jpeg_geometry(17, 33, 4, 444);
    CHECK(g.mcu == 8 && g.bpm == 3 && g.mcus_x == 5 && g.mcus_y == 3 && g.n_mcu == 15 && g.ri == 4 && g.intervals == 4);
    g = jpeg_geometry(16384, 16384, 1, 444);                                 // the most intervals there can be
    CHECK(g.n_mcu == 2048 * 2048 && g.intervals == g.n_mcu);
    CHECK(jpeg_worst_case_bytes(g) == 629 + 416ll * 3 * g.n_mcu + 2ll * g.intervals + 2);
    CHECK(jpeg_default_max_bytes(g) == 629 + 3ll * 16384 * 16384 + 2ll * g.intervals + 2);

    // tables
    uint8_t ql[64], qc[64];
    CHECK(code_of([&] { jpeg_tables(0, ql, qc); }) == AIC_ERR_INVALID && code_of([&] { jpeg_tables(101, ql, qc); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { jpeg_tables(50, nullptr, qc); }) == AIC_ERR_INVALID && code_of([&] { jpeg_tables(50, ql, nullptr); }) == AIC_ERR_INVALID);
    jpeg_tables(1, ql, qc);
    for (int i = 0; i < 64; ++i) CHECK(ql[i] == 255 && qc[i] == 255);
    jpeg_tables(100, ql, qc);
    for (int i = 0; i < 64; ++i) CHECK(ql[i] == 1 && qc[i] == 1);
    jpeg_tables(75, ql, qc);
    CHECK(ql[0] == 8 && ql[1] == 6 && ql[63] == 50 && qc[0] == 9 && qc[63] == 50);

    // the header: 629 bytes exactly, into a buffer of exactly that size
    for (int q : {1, 50, 100}) {
        std::vector<uint8_t> hdr(JPEG_HEADER_BYTES);
        g = jpeg_geometry(16384, 16383, 65535, 420);
        jpeg_header(g, q, hdr.data());
        CHECK(hdr[0] == 0xff && hdr[1] == 0xd8 && hdr[2] == 0xff && hdr[3] == 0xe0 && hdr[627] == 63 && hdr[628] == 0);
        CHECK(hdr[163] == 0x40 && hdr[164] == 0x00 && hdr[165] == 0x3f && hdr[166] == 0xff);   // SOF0's height and width, big endian
    }

    // the device's words: every reciprocal divides exactly over the whole range of |F| + 4 Q, the Huffman codes are prefix-free and complete
    for (int q : {1, 37, 50, 100}) {
        std::vector<uint32_t> w;
        g = jpeg_geometry(720, 1280, 0, 420);
        jpeg_device_tables(g, q, w);
        CHECK((int)w.size() == JPEG_TAB_WORDS);
        jpeg_tables(q, ql, qc);
        for (int t = 0; t < 2; ++t)
            for (int i = 0; i < 64; ++i) {
                const uint32_t Q = t ? qc[i] : ql[i], rcp = w[JPEG_TAB_RCP + t * 64 + i];
                CHECK(w[JPEG_TAB_ADD + t * 64 + i] == 4 * Q);
                for (uint32_t n = 0; n < (1u << 15) + 4 * 255; n += (n < 4096 * Q ? 1 : 7)) CHECK((uint32_t)(((uint64_t)n * rcp) >> 32) == n / (8 * Q));
            }
        const uint8_t* zz = reinterpret_cast<const uint8_t*>(&w[JPEG_TAB_ZZ]);
        CHECK(zz[0] == 0 && zz[1] == 1 && zz[8] == 2 && zz[16] == 3 && zz[9] == 4 && zz[63] == 63 && zz[7] == 28 && zz[56] == 35);
        for (int t = 0; t < 4; ++t) {
            const uint32_t* codes = t < 2 ? &w[JPEG_TAB_DC + t * 16] : &w[JPEG_TAB_AC + (t - 2) * 256];
            const int n = t < 2 ? 16 : 256, want = t < 2 ? 12 : 162;
            int used = 0;
            double kraft = 0;
            for (int a = 0; a < n; ++a) {
                const uint32_t la = codes[a] & 31u, ca = codes[a] >> 5;
                if (!la) continue;
                ++used;
                kraft += 1.0 / (double)(1u << la);
                CHECK(la <= 16 && ca < (1u << la));
                for (int b = 0; b < n; ++b) {
                    const uint32_t lb = codes[b] & 31u, cb = codes[b] >> 5;
                    if (b != a && lb && lb >= la) CHECK((cb >> (lb - la)) != ca);
                }
            }
            CHECK(used == want && kraft < 1.0);                              // (the all-ones code word stays free)
            if (t >= 2) CHECK((codes[0x00] & 31u) && (codes[0xF0] & 31u) && (codes[0xFA] & 31u) && !(codes[0x0B] & 31u));
        }
    }

    // configuration and call checks
    aic_jpeg_config c{16, 720, 1280, 85, 0, 420, 0};
    CHECK(code_of([&] { jpeg_check_config(0, &c); }) == AIC_OK && code_of([&] { jpeg_check_config(-1, &c); }) == AIC_ERR_INVALID);
    CHECK(code_of([&] { jpeg_check_config(0, nullptr); }) == AIC_ERR_INVALID);
    auto bad = [&](auto&& edit) {
        aic_jpeg_config d = c;
        edit(d);
        return code_of([&] { jpeg_check_config(0, &d); });
    };
    CHECK(bad([](aic_jpeg_config& d) { d.max_images = 0; }) == AIC_ERR_INVALID && bad([](aic_jpeg_config& d) { d.max_images = 4097; }) == AIC_ERR_INVALID);
    CHECK(bad([](aic_jpeg_config& d) { d.max_images = 4096; }) == AIC_OK && bad([](aic_jpeg_config& d) { d.quality = 0; }) == AIC_ERR_INVALID);
    CHECK(bad([](aic_jpeg_config& d) { d.quality = 101; }) == AIC_ERR_INVALID && bad([](aic_jpeg_config& d) { d.height = 0; }) == AIC_ERR_INVALID);
    CHECK(bad([](aic_jpeg_config& d) { d.width = 16385; }) == AIC_ERR_INVALID && bad([](aic_jpeg_config& d) { d.subsampling = 422; }) == AIC_ERR_INVALID);
    CHECK(bad([](aic_jpeg_config& d) { d.restart = -1; }) == AIC_ERR_INVALID && bad([](aic_jpeg_config& d) { d.restart = 65536; }) == AIC_ERR_INVALID);
    CHECK(bad([](aic_jpeg_config& d) { d.max_bytes = 630; }) == AIC_ERR_INVALID && bad([](aic_jpeg_config& d) { d.max_bytes = 631; }) == AIC_OK);
    CHECK(bad([](aic_jpeg_config& d) { d.max_bytes = -1; }) == AIC_ERR_INVALID);
    uint8_t byte = 0;
    int64_t off[17];
    int32_t st[16];
    auto call = [&](const void* fr, int fm, int n, const void* out, int om, int64_t cap, const int64_t* o, const int32_t* s) {
        return code_of([&] { jpeg_check_encode(c, fr, fm, n, out, om, cap, o, s); });
    };
    CHECK(call(&byte, AIC_HOST, 16, &byte, AIC_DEVICE, 1, off, st) == AIC_OK && call(nullptr, AIC_HOST, 0, nullptr, AIC_HOST, 0, off, st) == AIC_OK);
    CHECK(call(&byte, AIC_HOST, 17, &byte, AIC_HOST, 1, off, st) == AIC_ERR_INVALID && call(&byte, AIC_HOST, -1, &byte, AIC_HOST, 1, off, st) == AIC_ERR_INVALID);
    CHECK(call(&byte, 2, 1, &byte, AIC_HOST, 1, off, st) == AIC_ERR_INVALID && call(&byte, AIC_HOST, 1, &byte, -1, 1, off, st) == AIC_ERR_INVALID);
    CHECK(call(&byte, AIC_HOST, 1, &byte, AIC_HOST, -1, off, st) == AIC_ERR_INVALID && call(nullptr, AIC_HOST, 1, &byte, AIC_HOST, 1, off, st) == AIC_ERR_INVALID);
    CHECK(call(&byte, AIC_HOST, 1, nullptr, AIC_HOST, 1, off, st) == AIC_ERR_INVALID && call(&byte, AIC_HOST, 1, &byte, AIC_HOST, 1, nullptr, st) == AIC_ERR_INVALID);
    CHECK(call(&byte, AIC_HOST, 1, &byte, AIC_HOST, 1, off, nullptr) == AIC_ERR_INVALID);

    // packing: an image beyond max_bytes takes no room, its neighbours keep their order; sizes beyond 32 bits
    g = jpeg_geometry(32, 16, 0, 420);                                       // 2 intervals: 629 + entropy + 2 + 2
    const int64_t ent[4] = {10, 100, 0, 10};
    CHECK(jpeg_pack(ent, 4, g, 643, off, st) == 3 * 633 + 10 + 0 + 10);
    CHECK(off[0] == 0 && off[1] == 643 && off[2] == 643 && off[3] == 643 + 633 && off[4] == 643 + 633 + 643);
    CHECK(st[0] == 0 && st[1] == AIC_ERR_CAPACITY && st[2] == 0 && st[3] == 0);
    CHECK(jpeg_pack(ent, 4, g, 642, off, st) == 633 && st[0] == AIC_ERR_CAPACITY && st[3] == AIC_ERR_CAPACITY && off[4] == 633);
    CHECK(jpeg_pack(ent, 0, g, 642, off, st) == 0 && off[0] == 0);
    const int64_t big[3] = {3ll << 30, 3ll << 30, 3ll << 30};
    CHECK(jpeg_pack(big, 3, g, 1ll << 40, off, st) == 3 * ((3ll << 30) + 633) && off[2] == 2 * ((3ll << 30) + 633));

    std::printf("probe ok: %d checks\n", g_checks);
    return 0;
}
