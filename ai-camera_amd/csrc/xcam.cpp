// xcam.cpp -- the cross-camera object of a tracker bank (xcam.hpp) and its C ABI.  The pack and the nearest rows run in kernels_xcam.hip
// or the call raises; the policy on top is GidTable's (global_id.cpp), the one the rank exchange uses.
#include "xcam.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>

namespace aic {

void xcam_check_params(int streams, int t_max, int dim, double max_cosine_distance) {
    AIC_REQUIRE(streams >= 1 && streams <= BANK_STREAMS_MAX_XCAM, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(t_max >= 1 && t_max <= XCAM_TMAX, AIC_ERR_INVALID, "t_max must be in 1..512");
    AIC_REQUIRE(dim >= 4 && dim <= 1024 && dim % 4 == 0, AIC_ERR_INVALID, "dim must be a multiple of 4 in 4..1024 (what both banks accept)");
    AIC_REQUIRE(std::isfinite(max_cosine_distance) && max_cosine_distance >= 0.0, AIC_ERR_INVALID, "max_cosine_distance must be finite and >= 0");
}

XCam::XCam(Device& d, int streams, int t_max_, int dim_, double max_cosine_distance)
    : dev(&d), n_streams(streams), t_max(t_max_), dim(dim_), n(streams * t_max_), max_cos(max_cosine_distance) {
    gid.world = streams;
}

void XCam::ensure() {
    dev->use();
    if (d_tab.p) return;
    d_shards.alloc((size_t)n * (2 + dim));
    // the pack kernels write a row's embedding only when the row is valid: aic_xcam_shards returns every row, so the rows no pass has
    // packed yet hold zeros, not what the allocation held
    HIP_CHECK(hipMemset(d_shards.p, 0, d_shards.bytes()));
    d_tab.alloc(3 * (size_t)n + 2 * (size_t)n_streams);
    d_best.alloc(n);
    h_tab.alloc(3 * (size_t)n + 2 * (size_t)n_streams);
}

int XCam::pass(hipStream_t s, const int32_t* expect) {
    has_pass = false;
    {
        Prof pr(*dev, PROF_TRK, s, 2.0 * n * (double)(n - t_max) * dim, (double)n * (2 + dim) * 4);
        launch_xcam_nearest(d_shards.p, d_nvalid(), n_streams, t_max, dim, tile, d_best.p, d_tab.p, d_tab.p + n, reinterpret_cast<float*>(d_tab.p + 2 * (size_t)n), s);
    }
    HIP_CHECK(hipMemcpyAsync(h_tab.p, d_tab.p, d_tab.bytes(), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    const int* nv = h_tab.p + 3 * (size_t)n;
    const int* fl = nv + n_streams;
    for (int q = 0; q < n_streams; ++q) {
        AIC_REQUIRE(!(fl[q] & 1), AIC_ERR_INVALID, "stream " + std::to_string(q) + ": the valid rows of the shard are not a prefix of its slice");
        AIC_REQUIRE(!(fl[q] & 2), AIC_ERR_CAPACITY, "stream " + std::to_string(q) + ": a track id >= 2^24 does not travel as fp32 in the shard");
    }
    if (expect)
        for (int q = 0; q < n_streams; ++q)
            AIC_REQUIRE(nv[q] == expect[q], AIC_ERR_INVALID, "stream " + std::to_string(q) + ": n_valid differs from the shard's valid column");
    const int links = gid.update(n_streams, t_max, ids(), near_row(), near_dist(), max_cos);
    has_pass = true;
    if (archive) archive_step();
    return links;
}

void XCam::archive_step() {
    const int64_t tick = passes;
    returning.clear();
    std::vector<int64_t> keys(n, -1);
    std::vector<int32_t> cams(n, 0), fresh;
    for (int i = 0; i < n; ++i) {
        if (ids()[i] < 0) continue;
        keys[i] = (int64_t)gid.key(i / t_max, ids()[i]);
        cams[i] = i / t_max;
        if (archive->ix.find(keys[i]) < 0) fresh.push_back(i);
    }
    const int nf = (int)fresh.size();
    if (nf && archive->ix.hw > 0) {
        const aic_archive_filter f{-1, (float)max_cos, std::numeric_limits<int64_t>::min(), tick - 1 - min_gap, -1};
        const std::vector<aic_archive_filter> flt(nf, f);
        archive->search(d_shards.p, 2 + dim, 2, nf, AIC_DEVICE, 1, flt.data(), fresh.data());
        const int32_t* rs = archive->res_slots();
        const float* rd = archive->res_dist(nf, 1);
        const int64_t* rk = archive->res_keys(nf, 1);
        std::map<int32_t, int> winner;                 // archived slot -> index into fresh
        for (int j = 0; j < nf; ++j) {
            if (rs[j] < 0) continue;
            auto it = winner.find(rs[j]);
            if (it == winner.end()) winner.emplace(rs[j], j);
            else if (rd[j] < rd[it->second]) it->second = j;   // distances are >= +0: the bits order like the values; a tie keeps the lower shard row
        }
        std::vector<int> won;
        for (auto& w : winner) won.push_back(w.second);
        std::sort(won.begin(), won.end());
        for (int j : won) {
            const int i = fresh[j];
            gid.first.emplace((uint64_t)rk[j], (uint64_t)rk[j]);   // an imported archive may hold keys this table never saw
            gid.link_keys(keys[i], rk[j]);
            returning.push_back({i / t_max, ids()[i], rk[j], rd[j]});
        }
    }
    archive->put(keys.data(), cams.data(), tick, d_shards.p, 2 + dim, 2, n, AIC_DEVICE);
    passes = tick + 1;
}

template <class Bank>
static void check_bank(const XCam& x, const Bank& b, int b_dim, const char* what) {
    AIC_REQUIRE(b.n_streams == x.n_streams, AIC_ERR_INVALID, std::string(what) + ": the bank's stream count differs from the cross-camera object's");
    AIC_REQUIRE(b_dim == x.dim, AIC_ERR_INVALID, std::string(what) + ": the bank's feature dimension differs from the cross-camera object's");
    AIC_REQUIRE(b.dev == x.dev, AIC_ERR_INVALID, std::string(what) + ": the bank lives on another device");
    for (int q = 0; q < b.n_streams; ++q)
        AIC_REQUIRE(!b.stop_code[q], AIC_ERR_INVALID, std::string(what) + ": stream " + std::to_string(q) + " is stopped by an earlier error (reset it first): " + b.stop_msg[q]);
}

int XCam::link(DeepSortBank& b) {
    check_bank(*this, b, b.dim, "DeepSORT bank");
    ensure();
    hipStream_t s = dev->s_trk;
    {
        Prof pr(*dev, PROF_TRK, s, 0, 0);
        launch_xcam_pack_deepsort(b.d_tbl.p, b.tbl_stride, b.d_gal_n.p, b.gal_stride, b.gmax, dim, n_streams, t_max, d_shards.p, d_nvalid(), d_flags(), s);
    }
    return pass(s);
}

int XCam::link(BotSortTracker& b) {
    check_bank(*this, b, b.prm.dim, "BoT-SORT bank");
    ensure();
    hipStream_t s = dev->s_trk;
    {
        Prof pr(*dev, PROF_TRK, s, 0, 0);
        launch_xcam_pack_botsort(b.d_tbl.p, b.stride, b.d_feat.p, b.feat_stride, b.prm.cap, dim, n_streams, t_max, d_shards.p, d_nvalid(), d_flags(), s);
    }
    return pass(s);
}

int XCam::link_shards(const float* shards, const int32_t* n_valid, int mem) {
    const int w = 2 + dim;
    if (n_valid)
        for (int q = 0; q < n_streams; ++q)
            AIC_REQUIRE(n_valid[q] >= 0 && n_valid[q] <= t_max, AIC_ERR_INVALID, "n_valid outside 0..t_max");
    if (mem == AIC_HOST) {                            // the valid column against the prefix, before the device is touched
        for (int q = 0; q < n_streams; ++q) {
            int cnt = 0, last = -1;
            for (int r = 0; r < t_max; ++r)
                if (shards[((size_t)q * t_max + r) * w] > 0.5f) ++cnt, last = r;
            AIC_REQUIRE(last + 1 == cnt, AIC_ERR_INVALID, "stream " + std::to_string(q) + ": the valid rows of the shard are not a prefix of its slice");
            AIC_REQUIRE(!n_valid || n_valid[q] == cnt, AIC_ERR_INVALID, "stream " + std::to_string(q) + ": n_valid differs from the shard's valid column");
        }
    }
    ensure();
    hipStream_t s = dev->s_trk;
    HIP_CHECK(hipMemcpyAsync(d_shards.p, shards, d_shards.bytes(), mem == AIC_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    // the counts always come from the valid column; the caller's n_valid is held against them after the read-back, before the policy
    launch_xcam_count(d_shards.p, n_streams, t_max, dim, d_nvalid(), d_flags(), s);
    return pass(s, n_valid);
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_xcam_create(int device_id, int streams, int t_max, int dim, double max_cosine_distance, aic_xcam** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        xcam_check_params(streams, t_max, dim, max_cosine_distance);
        *out = new aic_xcam(device(device_id), streams, t_max, dim, max_cosine_distance);
    });
}

int aic_xcam_destroy(aic_xcam* x) {
    return guarded([&] {
        if (x) { x->x.dev->use(); (void)hipStreamSynchronize(x->x.dev->s_trk); }
        delete x;
    });
}

int aic_xcam_option(aic_xcam* x, const char* key, int value) {
    return guarded([&] {
        AIC_REQUIRE(x && key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        if (k == "tile") {
            AIC_REQUIRE(value == 0 || value == 32 || value == 64, AIC_ERR_INVALID, "tile: 0 by size, 32 or 64 rows");
            x->x.tile = value;
        } else if (k == "min_gap") {
            AIC_REQUIRE(value >= 0, AIC_ERR_INVALID, "min_gap must be >= 0");
            x->x.min_gap = value;
        } else AIC_REQUIRE(false, AIC_ERR_INVALID, "unknown cross-camera option: " + k);
    });
}

int aic_xcam_link_deepsort_bank(aic_xcam* x, aic_deepsort_bank* bank, int32_t* n_links) {
    return guarded([&] {
        AIC_REQUIRE(x && bank, AIC_ERR_INVALID, "NULL argument");
        const int l = x->x.link(bank->t);
        if (n_links) *n_links = l;
    });
}

int aic_xcam_link_botsort_bank(aic_xcam* x, aic_botsort_bank* bank, int32_t* n_links) {
    return guarded([&] {
        AIC_REQUIRE(x && bank, AIC_ERR_INVALID, "NULL argument");
        const int l = x->x.link(bank->t);
        if (n_links) *n_links = l;
    });
}

int aic_xcam_link_shards(aic_xcam* x, const float* shards, const int32_t* n_valid, int mem, int32_t* n_links) {
    return guarded([&] {
        AIC_REQUIRE(x && shards, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
        const int l = x->x.link_shards(shards, n_valid, mem);
        if (n_links) *n_links = l;
    });
}

int aic_xcam_tables(aic_xcam* x, int32_t* track_id, int32_t* near_row, float* near_dist) {
    return guarded([&] {
        AIC_REQUIRE(x, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(x->x.has_pass, AIC_ERR_INVALID, "no link pass has completed yet");
        const XCam& c = x->x;
        if (track_id) std::copy(c.ids(), c.ids() + c.n, track_id);
        if (near_row) std::copy(c.near_row(), c.near_row() + c.n, near_row);
        if (near_dist) std::copy(c.near_dist(), c.near_dist() + c.n, near_dist);
    });
}

int aic_xcam_shards(aic_xcam* x, float* out) {
    return guarded([&] {
        AIC_REQUIRE(x && out, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(x->x.has_pass, AIC_ERR_INVALID, "no link pass has completed yet");
        x->x.dev->use();
        HIP_CHECK(hipStreamSynchronize(x->x.dev->s_trk));
        HIP_CHECK(hipMemcpy(out, x->x.d_shards.p, x->x.d_shards.bytes(), hipMemcpyDeviceToHost));
    });
}

int aic_xcam_global_ids(aic_xcam* x, int stream, const int32_t* track_ids, int n, int64_t* global_ids) {
    return guarded([&] {
        AIC_REQUIRE(x && n >= 0 && (n == 0 || (track_ids && global_ids)), AIC_ERR_INVALID, "bad argument");
        AIC_REQUIRE(stream >= 0 && stream < x->x.n_streams, AIC_ERR_INVALID, "stream outside the cross-camera object");
        for (int i = 0; i < n; ++i) global_ids[i] = x->x.gid.lookup(stream, track_ids[i]);
    });
}

int aic_xcam_size(aic_xcam* x, int64_t* n_tracks, int64_t* n_identities, int64_t* n_links) {
    return guarded([&] {
        AIC_REQUIRE(x, AIC_ERR_INVALID, "NULL argument");
        const GidTable& t = x->x.gid;
        if (n_tracks) *n_tracks = (int64_t)t.first.size();
        if (n_identities) *n_identities = (int64_t)t.first.size() - (int64_t)t.parent.size();
        if (n_links) *n_links = t.links;
    });
}

int aic_xcam_attach_archive(aic_xcam* x, aic_archive* a) {
    return guarded([&] {
        AIC_REQUIRE(x, AIC_ERR_INVALID, "NULL argument");
        if (a) {
            AIC_REQUIRE(a->a.dim == x->x.dim, AIC_ERR_INVALID, "the archive's dimension differs from the cross-camera object's");
            AIC_REQUIRE(a->a.dev == x->x.dev, AIC_ERR_INVALID, "the archive lives on another device");
        }
        x->x.archive = a ? &a->a : nullptr;
        if (!a) return;
        // rows of an earlier run (an imported archive): the clock goes on behind their last deposit, and a camera whose archived keys this
        // table never filed starts a generation above them, so that this run's (stream, track id) keys are not taken for theirs
        const ArchiveIndex& ix = a->a.ix;
        GidTable& g = x->x.gid;
        if (!ix.by_age.empty()) x->x.passes = std::max(x->x.passes, ix.by_age.rbegin()->first + 1);
        for (int s = 0; s < ix.hw; ++s) {
            const int64_t k = ix.key[s];
            if (k < 0 || g.first.count((uint64_t)k)) continue;
            const int rank = (int)((k >> 32) & ((1 << GidTable::kRankBits) - 1));
            const uint32_t gen = (uint32_t)(k >> (32 + GidTable::kRankBits));
            if (rank < g.world && gen < GidTable::kGenMax && g.generation(rank) <= gen) g.gen[rank] = gen + 1;
        }
    });
}

int aic_xcam_returning(aic_xcam* x, int32_t* stream, int32_t* track_id, int64_t* archived_key, float* dist, int cap, int32_t* n) {
    return guarded([&] {
        AIC_REQUIRE(x && cap >= 0, AIC_ERR_INVALID, "bad argument");
        const auto& r = x->x.returning;
        if (n) *n = (int32_t)r.size();
        for (int i = 0; i < cap && i < (int)r.size(); ++i) {
            if (stream) stream[i] = r[i].stream;
            if (track_id) track_id[i] = r[i].track_id;
            if (archived_key) archived_key[i] = r[i].archived_key;
            if (dist) dist[i] = r[i].dist;
        }
    });
}

int aic_xcam_forget_stream(aic_xcam* x, int stream) {
    return guarded([&] {
        AIC_REQUIRE(x, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(stream >= 0 && stream < x->x.n_streams, AIC_ERR_INVALID, "stream outside the cross-camera object");
        x->x.gid.forget_rank(stream);
    });
}

}  // extern "C"
