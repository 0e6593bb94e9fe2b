// archive.cpp -- the identity archive (archive.hpp) and its C ABI.  The index is integer bookkeeping on the host; quantisation, search and
// merge run in kernels_archive.hip or the call raises.
#include "archive.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

namespace aic {

// ------------------------------------------------------------------------------------------------ index
void ArchiveIndex::assign(const int64_t* keys, const int32_t* cameras, int64_t tick, int n, int32_t* slots, int64_t* evicted) {
    for (int i = 0; i < n; ++i) AIC_REQUIRE(keys[i] >= 0, AIC_ERR_INVALID, "an archive key must be >= 0");
    std::unordered_map<int, int> last;                     // slot -> the row of this call that holds it so far
    for (int i = 0; i < n; ++i) {
        if (evicted) evicted[i] = -1;
        int s = find(keys[i]);
        if (s >= 0) {                                      // upsert: the slot and t_first stay
            by_age.erase({t_last[s], s});
        } else {
            if (!free_slots.empty()) {
                s = *free_slots.begin();
                free_slots.erase(free_slots.begin());
            } else if (hw < cap) {
                s = hw++;
                key.push_back(-1), t_first.push_back(0), t_last.push_back(0), cam.push_back(0);
            } else {                                       // full: the smallest (t_last, slot) goes
                s = by_age.begin()->second;
                by_age.erase(by_age.begin());
                slot_of.erase(key[s]);
                if (evicted) evicted[i] = key[s];
            }
            key[s] = keys[i], t_first[s] = tick;
            slot_of[keys[i]] = s;
        }
        t_last[s] = tick, cam[s] = cameras[i];
        by_age.insert({tick, s});
        auto it = last.find(s);
        if (it != last.end()) slots[it->second] = -1;      // the later row of the call keeps the slot
        last[s] = i;
        slots[i] = s;
    }
}

int ArchiveIndex::remove(int64_t k) {
    const int s = find(k);
    if (s < 0) return -1;
    by_age.erase({t_last[s], s});
    slot_of.erase(k);
    key[s] = -1;
    free_slots.insert(s);
    return s;
}

void ArchiveIndex::clear() {
    hw = 0;
    key.clear(), t_first.clear(), t_last.clear(), cam.clear(), slot_of.clear(), free_slots.clear(), by_age.clear();
}

void ArchiveIndex::load(const int64_t* keys, const int32_t* cameras, const int64_t* tf, const int64_t* tl, int64_t n) {
    AIC_REQUIRE(n >= 0 && n <= cap, AIC_ERR_CAPACITY, "more rows than the archive's capacity");
    std::unordered_map<int64_t, int> seen;
    for (int64_t s = 0; s < n; ++s)
        if (keys[s] >= 0) AIC_REQUIRE(seen.emplace(keys[s], (int)s).second, AIC_ERR_INVALID, "a key occurs twice in the imported rows");
    clear();
    hw = (int)n;
    key.assign(keys, keys + n), cam.assign(cameras, cameras + n), t_first.assign(tf, tf + n), t_last.assign(tl, tl + n);
    slot_of = std::move(seen);
    for (int s = 0; s < hw; ++s) {
        if (key[s] >= 0) by_age.insert({t_last[s], s});
        else key[s] = -1, free_slots.insert(s);
    }
}

// ------------------------------------------------------------------------------------------------ device side
void archive_check_params(int64_t capacity, int dim) {
    AIC_REQUIRE(capacity >= 1 && capacity <= ARCHIVE_MAX_CAPACITY, AIC_ERR_INVALID, "capacity must be in 1..2^24");
    AIC_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, AIC_ERR_INVALID, "dim must be a multiple of 4 in 4..1024 (what aic_xcam_create accepts)");
}

void Archive::ensure() {
    dev->use();
    if (d_key.p) return;
    const size_t c = cap16();
    d_rows.alloc(c * pitch + 128);
    d_scale.alloc(c), d_cam.alloc(c), d_tlast.alloc(c), d_key.alloc(c);
    hipStream_t s = dev->s_trk;
    HIP_CHECK(hipMemsetAsync(d_rows.p, 0, d_rows.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_scale.p, 0, d_scale.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_cam.p, 0, d_cam.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_tlast.p, 0, d_tlast.bytes(), s));
    HIP_CHECK(hipMemsetAsync(d_key.p, 0xff, d_key.bytes(), s));
    d_out.alloc(16);
    h_out.alloc(16);
}

static inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

void Archive::put(const int64_t* keys, const int32_t* cameras, int64_t tick, const float* rows, long row_stride, int offset, int n, int mem) {
    if (n == 0) return;
    ensure();
    hipStream_t s = dev->s_trk;
    const size_t o_cam = up16((size_t)n * 8), o_slot = o_cam + up16((size_t)n * 4), o_rows = o_slot + up16((size_t)n * 4);
    d_stage.ensure(o_rows + (mem == AIC_HOST ? (size_t)n * row_stride * 4 : 0));
    long long* dk = reinterpret_cast<long long*>(d_stage.p);
    int* dc = reinterpret_cast<int*>(d_stage.p + o_cam);
    int* ds = reinterpret_cast<int*>(d_stage.p + o_slot);
    const float* dr = rows;
    HIP_CHECK(hipMemcpyAsync(dk, keys, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(dc, cameras, (size_t)n * 4, hipMemcpyHostToDevice, s));
    if (mem == AIC_HOST) {
        HIP_CHECK(hipMemcpyAsync(d_stage.p + o_rows, rows, (size_t)n * row_stride * 4, hipMemcpyHostToDevice, s));
        dr = reinterpret_cast<const float*>(d_stage.p + o_rows);
    }
    int* flag = reinterpret_cast<int*>(d_out.p);
    HIP_CHECK(hipMemsetAsync(flag, 0, 16, s));
    {   // the check: a row without a code fails the call before the index or a slot changes
        Prof pr(*dev, PROF_TRK, s, 0, (double)n * dim * 4);
        launch_archive_put(dr, nullptr, row_stride, offset, dim, pitch, n, nullptr, dk, nullptr, tick, 0, nullptr, nullptr, nullptr, nullptr, nullptr, flag, s);
    }
    HIP_CHECK(hipMemcpyAsync(h_out.p, flag, 16, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    AIC_REQUIRE(!*reinterpret_cast<const int*>(h_out.p), AIC_ERR_INVALID, "a row is all zero or holds a non-finite element: nothing was stored");
    // the rows that take part, packed for the index; the others keep slot -1
    std::vector<int64_t> k2;
    std::vector<int32_t> c2, s2, at;
    for (int i = 0; i < n; ++i)
        if (keys[i] >= 0) k2.push_back(keys[i]), c2.push_back(cameras[i]), at.push_back(i);
    s2.resize(k2.size());
    ix.assign(k2.data(), c2.data(), tick, (int)k2.size(), s2.data(), nullptr);
    std::vector<int32_t> slots(n, -1);
    for (size_t j = 0; j < at.size(); ++j) slots[at[j]] = s2[j];
    HIP_CHECK(hipMemcpyAsync(ds, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    {
        Prof pr(*dev, PROF_TRK, s, 0, (double)n * (dim * 4 + pitch));
        launch_archive_put(dr, nullptr, row_stride, offset, dim, pitch, n, ds, dk, dc, tick, 1, d_rows.p, d_scale.p, d_cam.p, d_tlast.p, d_key.p, flag, s);
    }
    HIP_CHECK(hipStreamSynchronize(s));                    // `slots` and the caller's arrays are free again
}

void Archive::remove(int64_t k) {
    const int slot = ix.remove(k);
    if (slot < 0 || !d_key.p) return;
    dev->use();
    HIP_CHECK(hipMemsetAsync(d_key.p + slot, 0xff, 8, dev->s_trk));
}

void Archive::clear() {
    ix.clear();
    if (!d_key.p) return;
    dev->use();
    HIP_CHECK(hipMemsetAsync(d_key.p, 0xff, d_key.bytes(), dev->s_trk));
}

void Archive::search(const float* q, long row_stride, int offset, int n, int mem, int k, const aic_archive_filter* filters, const int32_t* src_index) {
    ensure();
    hipStream_t s = dev->s_trk;
    const size_t o_ix = (size_t)n * sizeof(aic_archive_filter), o_q = o_ix + up16(src_index ? (size_t)n * 4 : 0);
    d_stage.ensure(o_q + (mem == AIC_HOST ? (size_t)n * row_stride * 4 : 0));
    const int* dix = nullptr;
    if (src_index) {
        dix = reinterpret_cast<const int*>(d_stage.p + o_ix);
        HIP_CHECK(hipMemcpyAsync(d_stage.p + o_ix, src_index, (size_t)n * 4, hipMemcpyHostToDevice, s));
    }
    std::vector<aic_archive_filter> none;
    if (!filters) {
        none.assign(n, aic_archive_filter{-1, std::numeric_limits<float>::infinity(), std::numeric_limits<int64_t>::min(),
                                          std::numeric_limits<int64_t>::max(), -1});
        filters = none.data();
    }
    aic_archive_filter* df = reinterpret_cast<aic_archive_filter*>(d_stage.p);
    HIP_CHECK(hipMemcpyAsync(df, filters, o_ix, hipMemcpyHostToDevice, s));
    const float* dq = q;
    if (mem == AIC_HOST) {
        HIP_CHECK(hipMemcpyAsync(d_stage.p + o_q, q, (size_t)n * row_stride * 4, hipMemcpyHostToDevice, s));
        dq = reinterpret_cast<const float*>(d_stage.p + o_q);
    }
    const size_t nk = (size_t)n * k, out_bytes = 16 + nk * 16;
    d_qrows.ensure((size_t)n * pitch), d_qscale.ensure(n);
    d_part.ensure(archive_partial_keys(ix.hw, n, k));
    if (d_out.n < out_bytes) d_out.alloc(out_bytes);
    h_out.ensure(out_bytes);
    int* flag = reinterpret_cast<int*>(d_out.p);
    HIP_CHECK(hipMemsetAsync(flag, 0, 16, s));
    {
        Prof pr(*dev, PROF_TRK, s, 2.0 * ix.hw * (double)n * pitch, (double)ix.hw * (pitch + 4) * ((n + 63) / 64));
        launch_archive_put(dq, dix, row_stride, offset, dim, pitch, n, nullptr, nullptr, nullptr, 0, 1, d_qrows.p, d_qscale.p, nullptr, nullptr, nullptr, flag, s);
        launch_archive_search(d_rows.p, d_scale.p, d_cam.p, d_tlast.p, d_key.p, ix.hw, pitch, d_qrows.p, d_qscale.p, df, n, k, d_part.p,
                              reinterpret_cast<int*>(d_out.p + 16), reinterpret_cast<float*>(d_out.p + 16 + nk * 4),
                              reinterpret_cast<long long*>(d_out.p + 16 + nk * 8), s);
    }
    HIP_CHECK(hipMemcpyAsync(h_out.p, d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    AIC_REQUIRE(!*reinterpret_cast<const int*>(h_out.p), AIC_ERR_INVALID, "a query is all zero or holds a non-finite element");
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_archive_index_create(int64_t capacity, aic_archive_index** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(capacity >= 1 && capacity <= ARCHIVE_MAX_CAPACITY, AIC_ERR_INVALID, "capacity must be in 1..2^24");
        *out = new aic_archive_index(capacity);
    });
}

int aic_archive_index_destroy(aic_archive_index* ix) {
    return guarded([&] { delete ix; });
}

int aic_archive_index_assign(aic_archive_index* ix, const int64_t* keys, const int32_t* cameras, int64_t tick, int n, int32_t* slots,
                             int64_t* evicted) {
    return guarded([&] {
        AIC_REQUIRE(ix && n >= 0 && (n == 0 || (keys && cameras && slots)), AIC_ERR_INVALID, "bad argument");
        ix->ix.assign(keys, cameras, tick, n, slots, evicted);
    });
}

int aic_archive_index_find(aic_archive_index* ix, int64_t key, int32_t* slot) {
    return guarded([&] {
        AIC_REQUIRE(ix && slot, AIC_ERR_INVALID, "NULL argument");
        *slot = ix->ix.find(key);
    });
}

int aic_archive_index_remove(aic_archive_index* ix, int64_t key, int32_t* slot) {
    return guarded([&] {
        AIC_REQUIRE(ix, AIC_ERR_INVALID, "NULL argument");
        const int s = ix->ix.remove(key);
        if (slot) *slot = s;
    });
}

int aic_archive_index_size(aic_archive_index* ix, int64_t* n_rows, int64_t* high_water) {
    return guarded([&] {
        AIC_REQUIRE(ix, AIC_ERR_INVALID, "NULL argument");
        if (n_rows) *n_rows = (int64_t)ix->ix.slot_of.size();
        if (high_water) *high_water = ix->ix.hw;
    });
}

int aic_archive_create(int device_id, int64_t capacity, int dim, aic_archive** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        archive_check_params(capacity, dim);
        *out = new aic_archive(device(device_id), capacity, dim);
    });
}

int aic_archive_destroy(aic_archive* a) {
    return guarded([&] {
        if (a) { a->a.dev->use(); (void)hipStreamSynchronize(a->a.dev->s_trk); }
        delete a;
    });
}

int aic_archive_put(aic_archive* a, const int64_t* keys, const int32_t* cameras, int64_t tick, const float* rows, int n, int mem) {
    return guarded([&] {
        AIC_REQUIRE(a && n >= 0 && (n == 0 || (keys && cameras && rows)), AIC_ERR_INVALID, "bad argument");
        AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
        for (int i = 0; i < n; ++i) AIC_REQUIRE(keys[i] >= 0, AIC_ERR_INVALID, "an archive key must be >= 0");
        a->a.put(keys, cameras, tick, rows, a->a.dim, 0, n, mem);
    });
}

int aic_archive_remove(aic_archive* a, int64_t key) {
    return guarded([&] {
        AIC_REQUIRE(a, AIC_ERR_INVALID, "NULL argument");
        a->a.remove(key);
    });
}

int aic_archive_search(aic_archive* a, const float* queries, int n, int mem, int k, const aic_archive_filter* filters, int64_t* out_keys,
                       int32_t* out_slots, float* out_dist) {
    return guarded([&] {
        AIC_REQUIRE(k >= 1 && k <= ARCHIVE_MAX_K, AIC_ERR_INVALID, "k must be in 1..32");
        AIC_REQUIRE(a && n >= 0 && (n == 0 || queries), AIC_ERR_INVALID, "bad argument");
        AIC_REQUIRE(n <= ARCHIVE_MAX_QUERIES, AIC_ERR_CAPACITY, "at most 2^17 queries a call");
        AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
        if (filters)
            for (int i = 0; i < n; ++i) AIC_REQUIRE(!std::isnan(filters[i].max_distance), AIC_ERR_INVALID, "max_distance is NaN");
        if (n == 0) return;
        Archive& A = a->a;
        A.search(queries, A.dim, 0, n, mem, k, filters);
        const size_t nk = (size_t)n * k;
        if (out_slots) std::copy(A.res_slots(), A.res_slots() + nk, out_slots);
        if (out_dist) std::copy(A.res_dist(n, k), A.res_dist(n, k) + nk, out_dist);
        if (out_keys) std::copy(A.res_keys(n, k), A.res_keys(n, k) + nk, out_keys);
    });
}

int aic_archive_size(aic_archive* a, int64_t* n_rows, int64_t* high_water) {
    return guarded([&] {
        AIC_REQUIRE(a, AIC_ERR_INVALID, "NULL argument");
        if (n_rows) *n_rows = (int64_t)a->a.ix.slot_of.size();
        if (high_water) *high_water = a->a.ix.hw;
    });
}

int aic_archive_export(aic_archive* a, int64_t* keys, int32_t* cameras, int64_t* t_first, int64_t* t_last, float* scales, int8_t* rows,
                       int64_t* n) {
    return guarded([&] {
        AIC_REQUIRE(a, AIC_ERR_INVALID, "NULL argument");
        Archive& A = a->a;
        const ArchiveIndex& ix = A.ix;
        const size_t hw = ix.hw;
        if (n) *n = ix.hw;
        if (keys) std::copy(ix.key.begin(), ix.key.end(), keys);
        if (cameras) std::copy(ix.cam.begin(), ix.cam.end(), cameras);
        if (t_first) std::copy(ix.t_first.begin(), ix.t_first.end(), t_first);
        if (t_last) std::copy(ix.t_last.begin(), ix.t_last.end(), t_last);
        if (!hw || (!scales && !rows)) return;
        A.ensure();
        HIP_CHECK(hipStreamSynchronize(A.dev->s_trk));
        if (scales) HIP_CHECK(hipMemcpy(scales, A.d_scale.p, hw * 4, hipMemcpyDeviceToHost));
        if (rows) HIP_CHECK(hipMemcpy(rows, A.d_rows.p, hw * A.pitch, hipMemcpyDeviceToHost));
    });
}

int aic_archive_import(aic_archive* a, const int64_t* keys, const int32_t* cameras, const int64_t* t_first, const int64_t* t_last,
                       const float* scales, const int8_t* rows, int64_t n) {
    return guarded([&] {
        AIC_REQUIRE(a && n >= 0 && (n == 0 || (keys && cameras && t_first && t_last && scales && rows)), AIC_ERR_INVALID, "bad argument");
        Archive& A = a->a;
        for (int64_t s = 0; s < n; ++s)
            AIC_REQUIRE(keys[s] < 0 || (std::isfinite(scales[s]) && scales[s] > 0.f), AIC_ERR_INVALID, "an occupied slot's scale must be finite and > 0");
        A.ix.load(keys, cameras, t_first, t_last, n);
        A.ensure();
        hipStream_t s = A.dev->s_trk;
        HIP_CHECK(hipMemsetAsync(A.d_key.p, 0xff, A.d_key.bytes(), s));
        if (n) {
            std::vector<long long> tl(t_last, t_last + n), kk(A.ix.key.begin(), A.ix.key.end());
            HIP_CHECK(hipMemcpyAsync(A.d_key.p, kk.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(A.d_tlast.p, tl.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(A.d_cam.p, cameras, (size_t)n * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(A.d_scale.p, scales, (size_t)n * 4, hipMemcpyHostToDevice, s));
            HIP_CHECK(hipMemcpyAsync(A.d_rows.p, rows, (size_t)n * A.pitch, hipMemcpyHostToDevice, s));
        }
        HIP_CHECK(hipStreamSynchronize(s));
    });
}

int aic_archive_clear(aic_archive* a) {
    return guarded([&] {
        AIC_REQUIRE(a, AIC_ERR_INVALID, "NULL argument");
        a->a.clear();
    });
}

int aic_archive_block_rows(aic_archive* a, int n_queries, int32_t* rows) {
    return guarded([&] {
        AIC_REQUIRE(a && rows && n_queries >= 1, AIC_ERR_INVALID, "bad argument");
        *rows = archive_block_rows(a->a.ix.hw, n_queries);
    });
}

}  // extern "C"
