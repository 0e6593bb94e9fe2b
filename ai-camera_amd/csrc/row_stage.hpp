// row_stage.hpp -- the small steps every stage with row lists or growing device buffers takes (bank_stage.hpp and through it zones.cpp,
// bestshot.cpp, colours.cpp, scene.cpp, left.cpp; jpeg.cpp, jpegdec.cpp): the check of the per-frame counts, the fetch of counts that lie in
// device memory, and the buffer growth that reports a capacity error.  Where the rows lie in a staging buffer is bank_call.hpp's.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

namespace aic {

// counts[F]: every frame has 0..rows_max rows, and rows6 is there when any frame has one.  Returns the call's rows.
inline long check_row_counts(const int32_t* counts, long F, int rows_max, const void* rows6) {
    long total = 0;
    for (long f = 0; f < F; ++f) {
        AIC_REQUIRE(counts[f] >= 0, AIC_ERR_INVALID, "a negative row count");
        AIC_REQUIRE(counts[f] <= rows_max, AIC_ERR_CAPACITY, "frame " + std::to_string(f) + " has more than " + std::to_string(rows_max) + " rows");
        total += counts[f];
    }
    AIC_REQUIRE(total == 0 || rows6, AIC_ERR_INVALID, "NULL rows");
    return total;
}

// counts in device memory decide the launches: one small copy brings them over
inline const int32_t* fetch_counts(std::vector<int>& h, const int32_t* d_counts, long F, hipStream_t st) {
    h.resize(F);
    HIP_CHECK(hipMemcpyAsync(h.data(), d_counts, F * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return h.data();
}

// grows a device buffer; a failed allocation is a capacity error of the call, not a runtime fault
template <class B>
inline void grow(B& buf, size_t count, const char* what) {
    if (count <= buf.n) return;
    try {
        buf.alloc(count);
    } catch (const Error&) {
        (void)hipGetLastError();
        throw Error(AIC_ERR_CAPACITY, std::string("the device has no room for ") + what + " (" + std::to_string(count * sizeof(*buf.p) >> 20) + " MiB)");
    }
}

}  // namespace aic
