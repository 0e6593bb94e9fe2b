// zones.cpp -- the zone / line counting object (zones.hpp) and its C ABI.  Every argument is checked before the device is touched; the
// arithmetic runs in kernels_zones.hip or the call raises.
#include "zones.hpp"
#include "bank_stage.hpp"

#include <algorithm>
#include <cstdlib>

namespace aic {

void zones_check_params(int streams, int max_tracks, int forget_after, int anchor) {
    AIC_REQUIRE(streams >= 1 && streams <= ZONES_STREAMS_MAX, AIC_ERR_INVALID, "streams must be in 1..256");
    AIC_REQUIRE(max_tracks >= 1 && max_tracks <= ZONES_TRACKS_MAX, AIC_ERR_INVALID, "max_tracks must be in 1..512");
    AIC_REQUIRE(forget_after >= 0 && forget_after <= (1 << 24), AIC_ERR_INVALID, "forget_after must be in 0..2^24");
    AIC_REQUIRE(anchor == 0 || anchor == 1, AIC_ERR_INVALID, "anchor must be 0 (bottom centre) or 1 (box centre)");
}

Zones::Zones(int device, int streams, int max_tracks_, int forget_after_, int anchor_)
    : device_id(device), n_streams(streams), max_tracks(max_tracks_), forget_after(forget_after_), anchor(anchor_),
      h_geo((size_t)streams * ZONES_GEO_INTS, 0), geo_dirty(streams, 1), reset_pending(streams, 1), stop(streams, 0) {}

static bool coord_ok(int32_t v) { return v >= -ZONES_COORD_MAX && v <= ZONES_COORD_MAX; }

void Zones::set(int stream, int n_zones, const int32_t* zone_nvert, const int32_t* zone_xy, int n_lines, const int32_t* line_xy) {
    AIC_REQUIRE(stream >= 0 && stream < n_streams, AIC_ERR_INVALID, "stream outside the zone counter");
    AIC_REQUIRE(n_zones >= 0 && n_zones <= ZONES_MAX, AIC_ERR_INVALID, "n_zones must be in 0..32");
    AIC_REQUIRE(n_lines >= 0 && n_lines <= ZONES_LINES_MAX, AIC_ERR_INVALID, "n_lines must be in 0..32");
    AIC_REQUIRE(n_zones == 0 || (zone_nvert && zone_xy), AIC_ERR_INVALID, "NULL zone arrays");
    AIC_REQUIRE(n_lines == 0 || line_xy, AIC_ERR_INVALID, "NULL line array");
    AIC_REQUIRE(!stop[stream], AIC_ERR_INVALID, "stream " + std::to_string(stream) + " is stopped by an earlier error (reset it first)");
    size_t nv = 0;
    for (int z = 0; z < n_zones; ++z) {
        AIC_REQUIRE(zone_nvert[z] >= 3 && zone_nvert[z] <= ZONES_VERTS_MAX, AIC_ERR_INVALID, "a zone must have 3..32 vertices");
        nv += zone_nvert[z];
    }
    for (size_t i = 0; i < 2 * nv; ++i) AIC_REQUIRE(coord_ok(zone_xy[i]), AIC_ERR_INVALID, "a zone coordinate is outside +-2^20");
    for (int i = 0; i < 4 * n_lines; ++i) AIC_REQUIRE(coord_ok(line_xy[i]), AIC_ERR_INVALID, "a line coordinate is outside +-2^20");
    int* g = h_geo.data() + (size_t)stream * ZONES_GEO_INTS;
    std::fill(g, g + ZONES_GEO_INTS, 0);
    g[0] = n_zones, g[1] = n_lines;
    const int32_t* v = zone_xy;
    for (int z = 0; z < n_zones; ++z) {
        g[ZONES_GEO_NVERT + z] = zone_nvert[z];
        for (int i = 0; i < 2 * zone_nvert[z]; ++i) g[ZONES_GEO_XY + z * ZONES_VERTS_MAX * 2 + i] = 2 * *v++;
    }
    for (int i = 0; i < 4 * n_lines; ++i) g[ZONES_GEO_LINES + i] = 2 * line_xy[i];
    geo_dirty[stream] = 1;
    reset_pending[stream] = 1;
}

void Zones::reset(int stream) {
    AIC_REQUIRE(stream >= 0 && stream < n_streams, AIC_ERR_INVALID, "stream outside the zone counter");
    stop[stream] = 0;
    reset_pending[stream] = 1;
}

void Zones::update(const int32_t* fps, const int32_t* counts, const int32_t* rows6, int mem, int cap, int32_t* n_events, int32_t* events,
                   int32_t* occupancy, int32_t* status) {
    AIC_REQUIRE(fps, AIC_ERR_INVALID, "NULL frames_per_stream");
    AIC_REQUIRE(mem == AIC_HOST || mem == AIC_DEVICE, AIC_ERR_INVALID, "mem must be AIC_HOST or AIC_DEVICE");
    AIC_REQUIRE(cap >= 0 && cap <= ZONES_CAP_EVENTS_MAX, AIC_ERR_INVALID, "cap_events must be in 0..65536");
    long F = 0;
    int max_fps = 0;
    for (int s = 0; s < n_streams; ++s) {
        AIC_REQUIRE(fps[s] >= 0 && fps[s] <= (1 << 20), AIC_ERR_INVALID, "frames_per_stream outside 0..2^20");
        F += fps[s];
        max_fps = std::max(max_fps, (int)fps[s]);
    }
    AIC_REQUIRE(F <= (1 << 20), AIC_ERR_INVALID, "more than 2^20 frames in one call");
    AIC_REQUIRE(F == 0 || (counts && n_events && occupancy), AIC_ERR_INVALID, "NULL counts, n_events or occupancy");
    AIC_REQUIRE(F == 0 || cap == 0 || events, AIC_ERR_INVALID, "NULL events");
    const long total = check_row_counts(counts, F, ZONES_ROWS_MAX, rows6);
    AIC_REQUIRE((size_t)F * (size_t)cap * 8 <= ((size_t)1 << 28), AIC_ERR_INVALID, "frames * cap_events * 8 exceeds 2^28 ints");

    if (!dev) dev = &device(device_id);
    dev->use();
    hipStream_t st = dev->s_trk;
    const int S = n_streams;
    if (!d_state.p) {
        d_state.alloc((size_t)S * ZONES_ST_INTS);
        d_cnt.alloc((size_t)S * ZONES_CNT);
        d_geo.alloc((size_t)S * ZONES_GEO_INTS);
        h_cnt.alloc(ZONES_CNT);
    }
    // ---- staging: fps[S] | fstart[S] | reset[S] | frame_off[F + 1] | frame_stream[F] | rows (host memory only; bank_call.hpp)
    const size_t o_fstart = S, o_reset = 2 * (size_t)S, o_off = 3 * (size_t)S, o_fs = o_off + F + 1;
    const BankStage rs(S, F, o_off, o_fs + F, total, mem == AIC_HOST);
    h_stage.ensure(rs.n_ints);
    d_stage.ensure(rs.n_ints);
    d_cls4.ensure(std::max<size_t>(4, (size_t)total * 4));
    int* h = h_stage.p;
    long f = 0;
    for (int s = 0; s < S; ++s) {
        h[s] = fps[s], h[o_fstart + s] = (int)f, h[o_reset + s] = reset_pending[s];
        for (int k = 0; k < fps[s]; ++k) h[o_fs + f++] = s;
    }
    rs.fill(h, counts, rows6);
    HIP_CHECK(hipMemcpyAsync(d_stage.p, h, rs.n_ints * sizeof(int), hipMemcpyHostToDevice, st));
    // ---- geometry that changed since the last update
    const long n_dirty = std::count(geo_dirty.begin(), geo_dirty.end(), (char)1);
    if (n_dirty > 8) HIP_CHECK(hipMemcpyAsync(d_geo.p, h_geo.data(), h_geo.size() * sizeof(int), hipMemcpyHostToDevice, st));
    else
        for (int s = 0; s < S; ++s)
            if (geo_dirty[s])
                HIP_CHECK(hipMemcpyAsync(d_geo.p + (size_t)s * ZONES_GEO_INTS, h_geo.data() + (size_t)s * ZONES_GEO_INTS, ZONES_GEO_INTS * sizeof(int),
                                         hipMemcpyHostToDevice, st));
    // ---- outputs: n_events[F] | occupancy[F, 32] | status[S] | (16-byte aligned) events[F, cap, 8]
    const size_t o_occ = F, o_status = o_occ + (size_t)F * ZONES_MAX, o_ev = (o_status + S + 3) / 4 * 4;
    const size_t n_out = o_ev + (size_t)F * cap * 8;
    d_out.ensure(n_out);
    h_out.ensure(n_out);
    HIP_CHECK(hipMemsetAsync(d_out.p, 0, n_out * sizeof(int), st));
    const int* d_rows = rs.d_rows(d_stage.p, rows6);
    {
        Prof pr(*dev, PROF_TRK, st, 0, (double)total * 40);
        if (total) launch_zones_classify(d_stage.p + o_off, d_stage.p + o_fs, (int)F, d_rows, d_geo.p, anchor, d_cls4.p, st);
        const int step = frames_per_launch > 0 ? frames_per_launch : std::max(max_fps, 1);
        for (int lo = 0, first = 1; first || lo < max_fps; lo += step, first = 0)
            launch_zones_walk(d_stage.p, d_stage.p + o_fstart, d_stage.p + o_reset, d_stage.p + o_off, d_rows, d_cls4.p, d_geo.p, d_state.p, d_cnt.p, S,
                              max_tracks, forget_after, first, lo, lo + step, cap, d_out.p, d_out.p + o_ev, d_out.p + o_occ, d_out.p + o_status, st);
    }
    HIP_CHECK(hipMemcpyAsync(h_out.p, d_out.p, n_out * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::fill(geo_dirty.begin(), geo_dirty.end(), (char)0);
    std::fill(reset_pending.begin(), reset_pending.end(), (char)0);
    const int* o = h_out.p;
    if (F) {
        std::copy(o, o + F, n_events);
        std::copy(o + o_occ, o + o_occ + (size_t)F * ZONES_MAX, occupancy);
        if (cap) std::copy(o + o_ev, o + o_ev + (size_t)F * cap * 8, events);
    }
    for (int s = 0; s < S; ++s) {
        stop[s] = o[o_status + s];
        if (status) status[s] = stop[s];
    }
}

void Zones::counters(int stream, int64_t* zone_in, int64_t* zone_out, int64_t* line_pos, int64_t* line_neg) {
    AIC_REQUIRE(stream >= 0 && stream < n_streams, AIC_ERR_INVALID, "stream outside the zone counter");
    int64_t* out[4] = {zone_in, zone_out, line_pos, line_neg};
    if (!d_cnt.p || reset_pending[stream]) {                 // nothing counted yet, or a reset the next update applies
        for (int64_t* p : out)
            if (p) std::fill(p, p + ZONES_MAX, (int64_t)0);
        return;
    }
    dev->use();
    HIP_CHECK(hipMemcpyAsync(h_cnt.p, d_cnt.p + (size_t)stream * ZONES_CNT, ZONES_CNT * sizeof(long long), hipMemcpyDeviceToHost, dev->s_trk));
    HIP_CHECK(hipStreamSynchronize(dev->s_trk));
    for (int k = 0; k < 4; ++k)
        if (out[k]) std::copy(h_cnt.p + k * ZONES_MAX, h_cnt.p + (k + 1) * ZONES_MAX, out[k]);
}

}  // namespace aic

using namespace aic;

extern "C" {

int aic_zones_create(int device_id, int streams, int max_tracks, int forget_after, int anchor, aic_zones** out) {
    return guarded([&] {
        AIC_REQUIRE(out, AIC_ERR_INVALID, "NULL argument");
        AIC_REQUIRE(device_id >= 0, AIC_ERR_INVALID, "device id out of range");
        zones_check_params(streams, max_tracks, forget_after, anchor);
        *out = new aic_zones(device_id, streams, max_tracks, forget_after, anchor);
    });
}

int aic_zones_destroy(aic_zones* z) { return destroy_handle(z, z ? z->z.dev : nullptr); }

int aic_zones_set(aic_zones* z, int stream, int n_zones, const int32_t* zone_nvert, const int32_t* zone_xy, int n_lines, const int32_t* line_xy) {
    return with_handle(z, [&] { z->z.set(stream, n_zones, zone_nvert, zone_xy, n_lines, line_xy); });
}

int aic_zones_update(aic_zones* z, const int32_t* frames_per_stream, const int32_t* counts, const int32_t* rows6, int mem, int cap_events,
                     int32_t* n_events, int32_t* events, int32_t* occupancy, int32_t* status) {
    return with_handle(z, [&] { z->z.update(frames_per_stream, counts, rows6, mem, cap_events, n_events, events, occupancy, status); });
}

int aic_zones_counters(aic_zones* z, int stream, int64_t* zone_in, int64_t* zone_out, int64_t* line_pos, int64_t* line_neg) {
    return with_handle(z, [&] { z->z.counters(stream, zone_in, zone_out, line_pos, line_neg); });
}

int aic_zones_reset(aic_zones* z, int stream) {
    return with_handle(z, [&] { z->z.reset(stream); });
}

int aic_zones_option(aic_zones* z, const char* key, int value) {
    return with_handle(z, [&] {
        AIC_REQUIRE(key, AIC_ERR_INVALID, "NULL argument");
        const std::string k(key);
        AIC_REQUIRE(k == "frames_per_launch", AIC_ERR_INVALID, "unknown zone counter option: " + k);
        AIC_REQUIRE(value >= 0 && value <= (1 << 20), AIC_ERR_INVALID, "frames_per_launch: 0 = a call's frames in one launch, or 1..2^20");
        z->z.frames_per_launch = value;
    });
}

}  // extern "C"
