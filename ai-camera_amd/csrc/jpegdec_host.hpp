// jpegdec_host.hpp -- the HIP-free half of the JPEG decoding stage (jpegdec_host.cpp; jpegdec.hpp has the device half; DESIGN.md
// section 43): the argument checks, the parse of a file's segments up to SOS, the device's Huffman tables and the deduplication of
// table sets, the cut of a bank into launches, and a CPU decode of the coefficients through the very header the kernels compile
// (jpegdec_decode.hpp).  Compiles with plain g++ (tests/jpegdec_host_probe.cpp runs it under the sanitizers).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "assoc_host.hpp"
#include "jpegdec_decode.hpp"

namespace aic {

constexpr int JPEGDEC_IMAGES_MAX = 4096;
constexpr int JPEGDEC_DIM_MAX = 16384;
constexpr int64_t JPEGDEC_FILE_MAX = 64ll << 20;

struct JdParsed {                                // what the header of one file says
    aic_jpegdec_info info;                       // status / reason and the public fields
    JdImage rec;                                 // geometry, sampling, restart, table selectors; offsets are filled by the caller
    uint8_t quant[4][64];                        // natural order, by table id
    bool have_quant[4];
    struct Huff { uint8_t counts[16]; uint8_t val[256]; bool have; } huff[4];   // DC0 AC0 DC1 AC1
};

// Reads file[0, bytes) only.  height / width > 0: the picture must have that size.  Returns the reason (0 = accepted); info is filled
// either way (every field zero but status and reason when refused).
int jpegdec_parse(const uint8_t* file, int64_t bytes, int height, int width, JdParsed& out);
void jpegdec_build_huff(const uint8_t counts[16], const uint8_t* val, JdHuff& out);
void jpegdec_build_tables(const JdParsed& p, JdTables& out);

// The table sets of a call, deduplicated by content.
struct JdTableSets {
    std::vector<JdTables> sets;
    std::map<std::string, int> index;
    int add(const JdParsed& p);
};

void jpegdec_check_config(int device, const aic_jpegdec_config* c);
void jpegdec_check_bank(const aic_jpegdec_config& c, const void* files, int files_mem, const int64_t* offsets, int n);
// the interval table of one image's entropy data, found by its RSTm markers: lo / hi [intervals].  Returns 0 or the reason.
int jpegdec_host_intervals(const uint8_t* ent, int64_t len, int expected, std::vector<int64_t>& lo, std::vector<int64_t>& hi);
// One file on the CPU: the reason, and for an accepted file its coefficients [MCUs, blocks per MCU, 64] in natural order.
int jpegdec_host_decode(const uint8_t* file, int64_t bytes, int height, int width, std::vector<int16_t>& coef, aic_jpegdec_info* info);

}  // namespace aic
