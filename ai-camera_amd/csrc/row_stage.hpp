// row_stage.hpp -- what the analytics stages (zones.cpp, bestshot.cpp, scene.cpp) share around a call's row lists: the check of the per-frame
// counts, their prefix sums in the stage's int staging buffer with host rows riding behind, and the buffer growth that reports a capacity error.
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

// frame_off[F + 1] at int o_off of a stage's staging buffer and, for rows in host memory, the rows at o_rows (the buffer's end)
struct RowStage {
    size_t o_off, o_rows, n_ints;   // n_ints: the whole staging buffer
    bool staged;
    RowStage(size_t off, size_t rows, long total, bool host_rows)
        : o_off(off), o_rows(rows), n_ints(rows + (host_rows ? (size_t)total * 6 : 0)), staged(host_rows) {}
    void fill(int* h, const int32_t* counts, long F, const int32_t* rows6) const {   // counts NULL: a call without rows
        h[o_off] = 0;
        for (long i = 0; i < F; ++i) h[o_off + i + 1] = h[o_off + i] + (counts ? counts[i] : 0);
        if (n_ints > o_rows) std::memcpy(h + o_rows, rows6, (n_ints - o_rows) * sizeof(int));
    }
    // the rows on the device: the staged copy, or the caller's pointer
    const int* d_rows(const int* d_stage, const int32_t* rows6) const { return staged ? d_stage + o_rows : rows6; }
};

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
