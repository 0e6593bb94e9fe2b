// common.hpp -- error handling, device context, buffers and event profiling for libaicam.so.
// MI355X / gfx950 only; no CPU fallback anywhere in this library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/aicam.h"
#include "assoc_host.hpp"
#include "poison_pattern.hpp"

namespace aic {

#define HIP_CHECK(expr)                                                                        \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            throw ::aic::Error(AIC_ERR_RUNTIME, std::string(#expr) + ": " + hipGetErrorString(_e) + \
                                                    " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

// AICAM_POISON_ALLOC=zero|big|nan (poison_pattern.hpp; tests): every fresh DevBuf / PinBuf allocation is filled before alloc returns,
// so that a read of memory nobody wrote gives the same wrong bytes in every process.  Unset: nothing is filled.
inline poison::Mode poison_mode() {
    static const poison::Mode m = poison::parse(getenv("AICAM_POISON_ALLOC"));
    return m;
}

// the device synchronise keeps every stream behind the fill: a buffer's intended initialisation still lands after it
inline void poison_fill_device(void* p, size_t bytes, poison::Fill f) {
    if (f.width == 1) {
        HIP_CHECK(hipMemset(p, (int)f.value, bytes));
    } else if (f.width == 4) {
        HIP_CHECK(hipMemsetD32((hipDeviceptr_t)p, (int)f.value, bytes / 4));
    } else {
        std::vector<unsigned char> h(bytes);
        poison::fill_host(h.data(), bytes, f);
        HIP_CHECK(hipMemcpy(p, h.data(), bytes, hipMemcpyHostToDevice));
    }
    HIP_CHECK(hipDeviceSynchronize());
}

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void alloc(size_t count) {
        release();
        n = count;
        if (count) HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T)));
        if (count && poison_mode() != poison::OFF) {
            AIC_REQUIRE(poison_mode() != poison::BAD, AIC_ERR_INVALID, "AICAM_POISON_ALLOC: zero, big or nan");
            poison_fill_device(p, count * sizeof(T), poison::pattern<T>(poison_mode()));
        }
    }
    void ensure(size_t count) { if (count > n) alloc(count); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; } n = 0; }
    size_t bytes() const { return n * sizeof(T); }
};

template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t n = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { release(); }
    void alloc(size_t count) {
        release();
        n = count;
        if (count) HIP_CHECK(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault));
        if (count && poison_mode() != poison::OFF) {
            AIC_REQUIRE(poison_mode() != poison::BAD, AIC_ERR_INVALID, "AICAM_POISON_ALLOC: zero, big or nan");
            poison::fill_host(p, count * sizeof(T), poison::pattern<T>(poison_mode()));
        }
    }
    void ensure(size_t count) { if (count > n) alloc(count); }
    void release() { if (p) { (void)hipHostFree(p); p = nullptr; } n = 0; }
};

enum ProfClass { PROF_CONV = 0, PROF_CONV_DIRECT = 1, PROF_MISC = 2, PROF_LETTERBOX = 3, PROF_CROP = 4,
                 PROF_DET = 5, PROF_TRK = 6 };

// One per visible GPU, created on first use. Owns the streams every handle on that GPU uses.
struct Device {
    int id = 0;
    hipStream_t s_main = nullptr;  // detection + ReID launch groups
    hipStream_t s_trk = nullptr;   // per-frame association chain
    hipStream_t s_reid = nullptr;  // crop + ReID launch group (runs beside YOLO's thin layers, which leave CUs idle)
    hipStream_t s_det = nullptr;   // decode + NMS + detection read-back (overlaps the ReID launch group)
    int n_cu = 256;
    unsigned prof_mask = 0;   // bit c set = class c is timed with HIP events
    struct Pair { hipEvent_t a, b; };
    std::vector<Pair> pending[AIC_PROF_CLASSES];
    std::vector<Pair> pool;
    std::mutex prof_mu;            // launches come from two host threads (pipeline producer / tracker)
    double ms[AIC_PROF_CLASSES] = {0};
    // length of the UNION of a class's bracketed intervals on the device clock (ms): with brackets open on two streams at once
    // (split_streams: YOLO's convs beside ReID's) the summed durations count the overlap twice and say nothing about the class's
    // rate; FLOPs / union does.  Equal to ms[] while one stream carries the class.  0 when the cross-stream timestamps are unavailable
    double ms_union[AIC_PROF_CLASSES] = {0};
    hipEvent_t prof_ref = nullptr;     // time origin of the intervals, recorded by prof_reset
    int64_t launches[AIC_PROF_CLASSES] = {0};
    double flops[AIC_PROF_CLASSES] = {0};
    double bytes[AIC_PROF_CLASSES] = {0};

    // (No frame is shared between engines: the per-frame plugin loop hands the same frame to two engines, and each call uploads the
    // frame it is handed into its own engine's staging buffer -- a result depends on the call's arguments only.  DESIGN.md section 53.)

    void use() const { HIP_CHECK(hipSetDevice(id)); }
    void prof_begin(int cls, hipStream_t s, double fl, double by);
    void prof_end(int cls, hipStream_t s);
    void prof_account(int cls, double fl, double by);   // one more launch inside the open bracket
    void prof_collect();
    void prof_reset();
};

Device& device(int id);
int device_count();

// RAII bracket around one kernel launch of a profiled class.
struct Prof {
    Device& d;
    int cls;
    hipStream_t s;
    bool on;
    Prof(Device& dev, int c, hipStream_t st, double fl = 0, double by = 0) : d(dev), cls(c), s(st), on((dev.prof_mask >> c) & 1u) {
        if (on) d.prof_begin(cls, s, fl, by);
    }
    ~Prof() {
        if (on) d.prof_end(cls, s);
    }
};

static inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

#define KCHECK() HIP_CHECK(hipGetLastError())

// Raises kernel kfn's dynamic-LDS limit to `bytes`: once per (kernel, current device), from any thread.
void set_lds_limit(const void* kfn, size_t bytes);
template <class K> inline void set_lds_limit(K* kfn, size_t bytes) { set_lds_limit(reinterpret_cast<const void*>(kfn), bytes); }

}  // namespace aic
