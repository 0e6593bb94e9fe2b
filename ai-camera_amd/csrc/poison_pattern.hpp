// poison_pattern.hpp -- what AICAM_POISON_ALLOC fills a fresh allocation with (common.hpp: DevBuf<T>::alloc, PinBuf<T>::alloc).
// Plain C++, no HIP: tests/poison_pattern_probe.cpp prints this table on the CPU.
//
//   T                                             zero   big                                  nan
//   float, double                                 0      every byte 0x7B (fp32 ~1.3e36)       every byte 0xFF
//   integer types of 4 or 8 bytes                 0      the VALUE 0x7B7B (31611)             every byte 0xFF (-1)
//   everything else (char, u8, 16-bit, structs)   0      every byte 0x7B (fp16 61280, u8 123) every byte 0xFF (fp16 NaN, u8 255)
//
// zero is what a fresh process usually gets: the baseline.  nan shows an uninitialised float read wherever arithmetic carries a NaN
// on; fminf / fmaxf and comparisons drop it, so big is a finite, ordinary-looking float that passes those as a value.  A typed
// integer buffer gets a small positive value under big: a stale count or index is then wrong but close by -- a wrong result, not a
// wild address.  An untyped char arena that kernels carve into integers cannot be given that: under big its ints read 0x7B7B7B7B.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <type_traits>

namespace aic {
namespace poison {

enum Mode { OFF = 0, ZERO = 1, BIG = 2, NANS = 3, BAD = -1 };

// AICAM_POISON_ALLOC's value: NULL -> OFF, "zero" / "big" / "nan" -> the mode, anything else -> BAD (the caller refuses it)
inline Mode parse(const char* s) {
    if (!s) return OFF;
    if (!std::strcmp(s, "zero")) return ZERO;
    if (!std::strcmp(s, "big")) return BIG;
    if (!std::strcmp(s, "nan")) return NANS;
    return BAD;
}

// the buffer is `width`-byte units, each holding `value`'s low `width` bytes; width is 1, 4 or 8
struct Fill {
    int width;
    uint64_t value;
};

inline Fill pattern(bool is_float, bool is_int, size_t size, Mode m) {
    if (m == ZERO) return {1, 0};
    if (m == NANS) return {1, 0xFF};
    if (!is_float && is_int && (size == 4 || size == 8)) return {(int)size, 0x7B7B};
    return {1, 0x7B};
}

template <class T>
inline Fill pattern(Mode m) {
    return pattern(std::is_floating_point<T>::value, std::is_integral<T>::value, sizeof(T), m);
}

// the fill on host memory (a pinned buffer; the staging copy of a device fill of width 8)
inline void fill_host(void* p, size_t bytes, Fill f) {
    if (f.width == 1) {
        std::memset(p, (int)f.value, bytes);
        return;
    }
    unsigned char* q = static_cast<unsigned char*>(p);
    for (size_t i = 0; i + f.width <= bytes; i += f.width) std::memcpy(q + i, &f.value, f.width);   // (little endian: the low bytes)
}

}  // namespace poison
}  // namespace aic
