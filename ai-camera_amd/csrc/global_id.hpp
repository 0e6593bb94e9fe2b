// global_id.hpp -- the cross-camera global-id table (global_id.cpp: policy and C ABI aic_gid_*), shared with the bank pass of xcam.cpp.
// HOST code, HIP-free (tools/asan_host.sh).
#pragma once
#include <cstdint>
#include <map>

namespace aic {

struct GidTable {
    int world;
    std::map<uint64_t, uint64_t> first;     // (generation << 44 | rank << 32 | track id) -> global id given at its first sighting
    std::map<uint64_t, uint64_t> parent;    // global id -> smaller global id it was merged into
    std::map<int, uint32_t> gen;            // rank -> its current generation (absent = 0: the keys are (rank << 32 | track id))
    long links = 0, updates = 0;
    static constexpr int kRankBits = 12;    // world <= 4096; the generation sits in the bits above the rank
    static constexpr uint32_t kGenMax = (1u << 19) - 1;   // a global id stays a positive int64
    uint32_t generation(int rank) const {
        auto it = gen.find(rank);
        return it == gen.end() ? 0u : it->second;
    }
    // the key of (rank, track id) in the rank's CURRENT generation: what update() files sightings under and lookup() resolves
    uint64_t key(int rank, int id) const {
        return ((uint64_t)generation(rank) << (32 + kRankBits)) | ((uint64_t)(uint32_t)rank << 32) | (uint32_t)id;
    }
    uint64_t find(uint64_t g) {
        uint64_t r = g;
        for (auto it = parent.find(r); it != parent.end(); it = parent.find(r)) r = it->second;
        while (g != r) {                      // path compression
            auto it = parent.find(g);
            const uint64_t nx = it->second;
            it->second = r;
            g = nx;
        }
        return r;
    }
    bool unite(uint64_t a, uint64_t b) {
        a = find(a), b = find(b);
        if (a == b) return false;
        if (a < b) parent[b] = a; else parent[a] = b;
        return true;
    }
    // The rank's local ids start over (a camera reset): its (rank, id) keys of now are never met again.  Sightings from here on are filed
    // under the next generation; what the old keys were merged into -- and what adopted them -- keeps its number.
    // Nothing is erased: the old keys stay in `first` / `parent` (they may be roots of identities other ranks still carry), so the sizes
    // count them and the table grows with every reconnect.
    void forget_rank(int rank);
    // one nearest-neighbour table (aic_gallery_annotate's arrays, or the bank pass of xcam.cpp) -> new links
    int update(int world_, int t_max, const int32_t* track_id, const int32_t* near_row, const float* near_dist, double max_cosine_distance);
    int64_t lookup(int rank, int track_id);
    // by the key itself, whatever the rank's generation is now (the archive keeps keys of generations past): -1 = never filed
    int64_t find_key(int64_t k);
    // two filed keys become one identity under the smaller root; true = two identities were merged
    bool link_keys(int64_t a, int64_t b);
};

}  // namespace aic
