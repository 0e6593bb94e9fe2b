// poison_pattern_probe.cpp -- prints what ai-camera_amd/csrc/poison_pattern.hpp chooses for AICAM_POISON_ALLOC: the fill width and value
// per type and mode, the bytes fill_host() leaves in a buffer of that type and its first element read back, and what parse() makes of
// the variable's values.  tests/test_poison_pattern_host.py builds it with the system compiler under the address and undefined-behaviour
// sanitizers and runs it as a child process.  No HIP, no GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../ai-camera_amd/csrc/poison_pattern.hpp"

using namespace aic::poison;

struct Pod { float a; int b; char c; };

template <class T>
static void first_value(const char* name, const T& v) {
    if (std::is_floating_point<T>::value) std::printf(" first=%.17g", (double)v);
    else std::printf(" first=%lld", (long long)v);
}
template <>
void first_value<unsigned long long>(const char*, const unsigned long long& v) { std::printf(" first=%llu", v); }
template <>
void first_value<Pod>(const char*, const Pod& v) { std::printf(" first=%.9g/%d/%d", (double)v.a, v.b, (int)(unsigned char)v.c); }

template <class T>
static void show(const char* name) {
    static const struct { Mode m; const char* s; } MODES[] = {{ZERO, "zero"}, {BIG, "big"}, {NANS, "nan"}};
    for (const auto& md : MODES) {
        const Fill f = pattern<T>(md.m);
        std::vector<T> buf(5);                                   // five elements: an odd count, filled to its last byte
        fill_host(buf.data(), buf.size() * sizeof(T), f);
        std::printf("type=%s size=%zu mode=%s | width=%d value=0x%llx | bytes=", name, sizeof(T), md.s, f.width, (unsigned long long)f.value);
        const unsigned char* b = reinterpret_cast<const unsigned char*>(buf.data());
        for (size_t i = 0; i < buf.size() * sizeof(T); ++i) std::printf("%02x", b[i]);
        std::printf(" |");
        first_value<T>(name, buf[4]);
        std::printf("\n");
    }
}

int main() {
    show<float>("float");
    show<double>("double");
    show<int>("int");
    show<long long>("long long");
    show<unsigned long long>("unsigned long long");
    show<uint8_t>("uint8_t");
    show<int16_t>("int16_t");
    show<char>("char");
    show<Pod>("struct");
    const char* VALUES[] = {nullptr, "zero", "big", "nan", "", "1", "NaN", "zero "};
    for (const char* v : VALUES) std::printf("parse value=%s | mode=%d\n", v ? (*v ? v : "(empty)") : "(unset)", (int)parse(v));
    return 0;
}
