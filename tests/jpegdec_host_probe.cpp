// Test-only program: the HIP-free half of the JPEG decoding stage (ai-camera_amd/csrc/jpegdec_host.cpp) and the bit reader and block
// decoder the kernels compile (jpegdec_decode.hpp), built with the system g++ and run stand-alone under -fsanitize=address,undefined
// (tests/test_jpegdec_host.py).  It reads the cases tests/jpegdec_cases.py dumped -- well-formed files, refused files and seeded
// mutations, each with the oracle's reason and coefficients --, decodes every file from a heap buffer of exactly its size, so that one
// byte read outside it stops the program, and compares.  Exit code 0 and "probe ok" = clean.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ai-camera_amd/csrc/jpegdec_host.hpp"

namespace aic {
void set_last_error(const std::string&) {}
}  // namespace aic

using namespace aic;

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: jpegdec_host_probe cases.bin\n"), 2;
    std::FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return std::printf("cannot open %s\n", argv[1]), 2;
    int32_t n_cases = 0, accepted = 0, reasons[JD_REASONS] = {0};
    if (std::fread(&n_cases, 4, 1, fh) != 1) return std::printf("short file\n"), 2;
    for (int i = 0; i < n_cases; ++i) {
        int32_t head[5];                                                     // height, width, reason, file bytes, coefficients
        if (std::fread(head, 4, 5, fh) != 5) return std::printf("short file at case %d\n", i), 2;
        uint8_t* file = (uint8_t*)std::malloc((size_t)head[3] ? (size_t)head[3] : 1);      // exactly to size (one spare byte for an empty file, never handed over)
        std::vector<int16_t> want((size_t)head[4]), got;
        if (head[3] && std::fread(file, 1, (size_t)head[3], fh) != (size_t)head[3]) return std::printf("short file at case %d\n", i), 2;
        if (head[4] && std::fread(want.data(), 2, (size_t)head[4], fh) != (size_t)head[4]) return std::printf("short file at case %d\n", i), 2;
        aic_jpegdec_info info;
        const int reason = jpegdec_host_decode(head[3] ? file : nullptr, head[3], head[0], head[1], got, &info);
        std::free(file);
        if (reason != head[2]) return std::printf("case %d: reason %d, the oracle's is %d\n", i, reason, head[2]), 1;
        if ((reason != 0) != (info.status == AIC_ERR_FORMAT) || info.reason != reason) return std::printf("case %d: info disagrees\n", i), 1;
        if (got.size() != want.size() || (got.size() && std::memcmp(got.data(), want.data(), got.size() * 2)))
            return std::printf("case %d: coefficients differ from the oracle's\n", i), 1;
        accepted += reason == 0, ++reasons[reason];
    }
    std::fclose(fh);
    // the probe entry's own checks: a header that ends anywhere
    JdParsed p;
    const uint8_t soi[2] = {0xFF, 0xD8};
    if (jpegdec_parse(soi, 2, 0, 0, p) != JD_TRUNCATED || jpegdec_parse(soi, 1, 0, 0, p) != JD_NOT_JPEG || jpegdec_parse(nullptr, 0, 0, 0, p) != JD_NOT_JPEG)
        return std::printf("parse of a bare SOI\n"), 1;
    std::printf("probe ok: %d cases, %d accepted", n_cases, accepted);
    for (int r = 1; r < JD_REASONS; ++r) std::printf(" %d", reasons[r]);
    std::printf("\n");
    return 0;
}
