// global_id.cpp -- cross-camera global-ID policy of configs[4] (BASELINE.json; the reference lists "smarter gallery management
// in ReID" as future work, README.md:209).  HOST code, HIP-free (built under ASan/UBSan by
// tools/asan_host.sh): integer bookkeeping on top of the nearest-neighbour table the HIP pass (aic_gallery_annotate,
// kernels_trk_dev.hip::gallery_nearest_kernel) computes from the all-gathered gallery shards.
//
// Policy.  A track is known by (rank, track id).  Its global id is the (rank, track id) of the FIRST sighting of the identity: a
// track seen for the first time gets its own key, and when two tracks of different cameras are each other's nearest neighbour
// within the cosine threshold, both adopt the smaller of their two global ids (and so does everything that adopted either
// earlier: union-find with the smaller id as the root).  Per-stream association never reads this table (per-stream rows are
// those of configs[3]).
//
// Determinism across ranks.  Every rank holds the table for ALL ranks' tracks and updates it from the SAME all-gathered bytes:
// the distances are bit-symmetric (d(i, j) == d(j, i): same products, same summation order), ties go to the lowest row, links are
// applied in ascending row order.  No rank-dependent input enters, so after exchange e every rank has the same table without
// any further communication.
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#include "assoc_host.hpp"
#include "global_id.hpp"

namespace aic {

void GidTable::forget_rank(int rank) {
    AIC_REQUIRE(rank >= 0 && rank < world, AIC_ERR_INVALID, "rank outside the table's world");
    const uint32_t g = generation(rank);
    AIC_REQUIRE(g < kGenMax, AIC_ERR_CAPACITY, "rank forgotten too often (2^19 generations)");
    gen[rank] = g + 1;
}

int GidTable::update(int world_, int t_max, const int32_t* track_id, const int32_t* near_row, const float* near_dist, double max_cosine_distance) {
    AIC_REQUIRE(world_ == world, AIC_ERR_INVALID, "world size differs from the table's");
    const int n = world * t_max;
    const float thr = (float)max_cosine_distance;
    for (int i = 0; i < n; ++i) {
        if (track_id[i] < 0) continue;
        const uint64_t k = key(i / t_max, track_id[i]);
        first.emplace(k, k);                   // first sighting: its own (rank, track id)
    }
    int n_new = 0;
    for (int i = 0; i < n; ++i) {              // mutual nearest neighbours within the threshold, ascending row order
        const int j = near_row[i];
        if (track_id[i] < 0 || j <= i || j >= n || track_id[j] < 0) continue;
        if (near_row[j] != i || !(near_dist[i] <= thr)) continue;
        AIC_REQUIRE(i / t_max != j / t_max, AIC_ERR_INVALID, "nearest-neighbour table links two tracks of one camera");
        if (unite(first[key(i / t_max, track_id[i])], first[key(j / t_max, track_id[j])])) ++n_new;
    }
    links += n_new, updates += 1;
    return n_new;
}

int64_t GidTable::lookup(int rank, int track_id) {
    auto it = first.find(key(rank, track_id));
    return it == first.end() ? -1 : (int64_t)find(it->second);
}

int64_t GidTable::find_key(int64_t k) {
    auto it = k < 0 ? first.end() : first.find((uint64_t)k);
    return it == first.end() ? -1 : (int64_t)find(it->second);
}

bool GidTable::link_keys(int64_t a, int64_t b) {
    auto ia = a < 0 ? first.end() : first.find((uint64_t)a), ib = b < 0 ? first.end() : first.find((uint64_t)b);
    AIC_REQUIRE(ia != first.end() && ib != first.end(), AIC_ERR_INVALID, "link_keys: a key that was never filed");
    if (!unite(ia->second, ib->second)) return false;
    links += 1;
    return true;
}

}  // namespace aic

using namespace aic;

struct aic_gid { GidTable t; };

extern "C" {

int aic_gid_create(int world, aic_gid** out) {
    return guarded([&] {
        AIC_REQUIRE(out && world >= 1 && world <= 4096, AIC_ERR_INVALID, "bad argument");
        *out = new aic_gid();
        (*out)->t.world = world;
    });
}

int aic_gid_destroy(aic_gid* g) {
    return guarded([&] { delete g; });
}

int aic_gid_update(aic_gid* g, int world, int t_max, const int32_t* track_id, const int32_t* near_row, const float* near_dist,
                   double max_cosine_distance, int32_t* n_links) {
    return guarded([&] {
        AIC_REQUIRE(g && track_id && near_row && near_dist && t_max > 0, AIC_ERR_INVALID, "bad argument");
        const int links = g->t.update(world, t_max, track_id, near_row, near_dist, max_cosine_distance);
        if (n_links) *n_links = links;
    });
}

int aic_gid_lookup(aic_gid* g, int rank, int track_id, int64_t* global_id) {
    return guarded([&] {
        AIC_REQUIRE(g && global_id, AIC_ERR_INVALID, "NULL argument");
        *global_id = g->t.lookup(rank, track_id);
    });
}

int aic_gid_forget_rank(aic_gid* g, int rank) {
    return guarded([&] {
        AIC_REQUIRE(g, AIC_ERR_INVALID, "NULL argument");
        g->t.forget_rank(rank);
    });
}

int aic_gid_find_key(aic_gid* g, int64_t key, int64_t* global_id) {
    return guarded([&] {
        AIC_REQUIRE(g && global_id, AIC_ERR_INVALID, "NULL argument");
        *global_id = g->t.find_key(key);
    });
}

int aic_gid_link_keys(aic_gid* g, int64_t key_a, int64_t key_b, int32_t* linked) {
    return guarded([&] {
        AIC_REQUIRE(g, AIC_ERR_INVALID, "NULL argument");
        const bool l = g->t.link_keys(key_a, key_b);
        if (linked) *linked = l;
    });
}

int aic_gid_size(aic_gid* g, int64_t* n_tracks, int64_t* n_identities, int64_t* n_links) {
    return guarded([&] {
        AIC_REQUIRE(g, AIC_ERR_INVALID, "NULL argument");
        if (n_tracks) *n_tracks = (int64_t)g->t.first.size();
        if (n_identities) *n_identities = (int64_t)g->t.first.size() - (int64_t)g->t.parent.size();
        if (n_links) *n_links = g->t.links;
    });
}

}  // extern "C"
