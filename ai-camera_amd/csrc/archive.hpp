// archive.hpp -- the identity archive (archive.cpp, C ABI aic_archive_index_* / aic_archive_*; kernels_archive.hip):
// appearance rows of tracks that have ended, as int8 codes with one scale a row, searched by int8 MFMA.  ArchiveIndex is the slot
// bookkeeping on the host (HIP-free); Archive adds the device arrays and the three kernels.
//
// Device memory, allocated at the first call that needs it: capacity * (pitch + 24) bytes, pitch = dim rounded up to 64.
#pragma once
#include <cstdint>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace aic {

constexpr int64_t ARCHIVE_MAX_CAPACITY = 1 << 24;
constexpr int ARCHIVE_MAX_K = 32;
constexpr int ARCHIVE_MAX_QUERIES = 1 << 17;               // of one search call (a full pass of a 256 x 512 bank)

struct ArchiveIndex {
    int64_t cap;
    int hw = 0;                                            // high-water mark: slots [0, hw) have been handed out; the per-slot arrays have hw entries
    std::vector<int64_t> key, t_first, t_last;             // key < 0: free
    std::vector<int32_t> cam;
    std::unordered_map<int64_t, int> slot_of;
    std::set<int> free_slots;                              // below hw
    std::set<std::pair<int64_t, int>> by_age;              // (t_last, slot) of the occupied slots: begin() is evicted

    explicit ArchiveIndex(int64_t capacity) : cap(capacity) {}
    void assign(const int64_t* keys, const int32_t* cameras, int64_t tick, int n, int32_t* slots, int64_t* evicted);
    int find(int64_t k) const {
        auto it = slot_of.find(k);
        return it == slot_of.end() ? -1 : it->second;
    }
    int remove(int64_t k);
    void clear();
    // the contents from export's arrays (checked first: nothing changes on an error)
    void load(const int64_t* keys, const int32_t* cameras, const int64_t* tf, const int64_t* tl, int64_t n);
};

void archive_check_params(int64_t capacity, int dim);

struct Archive {
    Device* dev;
    int dim, pitch;
    ArchiveIndex ix;
    DevBuf<signed char> d_rows;                            // [cap16, pitch] + 128
    DevBuf<float> d_scale;                                 // [cap16]
    DevBuf<int> d_cam;
    DevBuf<long long> d_tlast, d_key;                      // d_key < 0: free (all of cap16 from the start)
    DevBuf<char> d_stage;                                  // a call's uploads: rows / queries fp32, keys, cameras, slots, filters
    DevBuf<signed char> d_qrows;
    DevBuf<float> d_qscale;
    DevBuf<unsigned long long> d_part;
    DevBuf<char> d_out;                                    // flag (16 bytes) | slots [n, k] | dist [n, k] | keys [n, k]
    PinBuf<char> h_out;

    Archive(Device& d, int64_t capacity, int dim_) : dev(&d), dim(dim_), pitch((dim_ + 63) / 64 * 64), ix(capacity) {}
    size_t cap16() const { return ((size_t)ix.cap + 15) / 16 * 16; }
    void ensure();
    // rows: fp32, row i at rows + i * row_stride + offset, host or device memory; keys[i] < 0 skips row i.  Check, one synchronisation,
    // then the index and the stores.  Host arrays keys / cameras.
    void put(const int64_t* keys, const int32_t* cameras, int64_t tick, const float* rows, long row_stride, int offset, int n, int mem);
    void remove(int64_t key);
    // queries as put's rows, query i = row src_index[i] (host list; NULL: i; device memory only); filters on the host (NULL = none).
    // Results in h_out until the next call: slots, dist, keys [n, k]
    void search(const float* q, long row_stride, int offset, int n, int mem, int k, const aic_archive_filter* filters,
                const int32_t* src_index = nullptr);
    const int32_t* res_slots() const { return reinterpret_cast<const int32_t*>(h_out.p + 16); }
    const float* res_dist(int n, int k) const { return reinterpret_cast<const float*>(h_out.p + 16 + (size_t)n * k * 4); }
    const int64_t* res_keys(int n, int k) const { return reinterpret_cast<const int64_t*>(h_out.p + 16 + (size_t)n * k * 8); }
    void clear();
};

}  // namespace aic

struct aic_archive_index {
    aic::ArchiveIndex ix;
    explicit aic_archive_index(int64_t c) : ix(c) {}
};

struct aic_archive {
    aic::Archive a;
    aic_archive(aic::Device& d, int64_t c, int dim) : a(d, c, dim) {}
};
