// zones.hpp -- zone entries, dwell and line crossings per camera, on the device (zones.cpp, C ABI aic_zones_*; kernels_zones.hip;
// DESIGN.md section 27).  A tracker-agnostic stage over the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32): per stream up
// to 32 polygon zones and 32 directed lines in integer pixels, a table of max_tracks slots, and exact integer arithmetic on doubled
// coordinates in int64 -- tests/zones_oracle.py is the specification, bit for bit.
//
// An update costs one staging upload, one classify launch over every frame of the call, one walk launch (one block per stream, its
// frames in order) and one read-back, whatever the stream count.  The device is first touched by the first update: create, set and
// reset only record what the next update stages.
#pragma once
#include "common.hpp"

namespace aic {

constexpr int ZONES_MAX = 32;              // zones per stream = bits of the inside mask
constexpr int ZONES_LINES_MAX = 32;
constexpr int ZONES_VERTS_MAX = 32;
constexpr int ZONES_ROWS_MAX = 512;        // rows per frame = threads of the walk block
constexpr int ZONES_TRACKS_MAX = 512;      // slots per stream
constexpr int ZONES_STREAMS_MAX = 256;
constexpr int ZONES_COORD_MAX = 1 << 20;
constexpr int ZONES_CAP_EVENTS_MAX = 1 << 16;   // a frame emits at most 512 * 32 LOST + 512 * (32 + 32) row events = 49152

// geometry of one stream, ints, coordinates doubled: n_zones, n_lines, 6 unused | n_vert[32] | zone xy [32][32][2] | line [32][4]
constexpr int ZONES_GEO_NVERT = 8;
constexpr int ZONES_GEO_XY = ZONES_GEO_NVERT + ZONES_MAX;
constexpr int ZONES_GEO_LINES = ZONES_GEO_XY + ZONES_MAX * ZONES_VERTS_MAX * 2;
constexpr int ZONES_GEO_INTS = ZONES_GEO_LINES + ZONES_LINES_MAX * 4;
// state of one stream, ints: frame, status, 6 unused | id, last_seen (-1 = free), ax, ay, mask, cls [512] each | enter frame [512][32]
constexpr int ZONES_ST_SLOTS = 8;
constexpr int ZONES_ST_ENTER = ZONES_ST_SLOTS + 6 * ZONES_TRACKS_MAX;
constexpr int ZONES_ST_INTS = ZONES_ST_ENTER + ZONES_TRACKS_MAX * ZONES_MAX;
// counters of one stream, int64: zone_in[32] | zone_out[32] | line_pos[32] | line_neg[32]
constexpr int ZONES_CNT = 4 * ZONES_MAX;

// kernels_zones.hip
// rows6 [rows, 6] -> cls4 [rows] = (ax, ay, inside mask, valid); grid = the call's frames
void launch_zones_classify(const int* frame_off, const int* frame_stream, int n_frames, const int* rows6, const int* geo, int anchor_centre, int* cls4,
                           hipStream_t s);
// one block per stream walks frames [f_lo, f_hi) of the stream's frames of this call; first != 0: the launch applies pending resets
void launch_zones_walk(const int* fps, const int* fstart, const int* reset, const int* frame_off, const int* rows6, const int* cls4, const int* geo,
                       int* state, long long* counters, int streams, int max_tracks, int forget_after, int first, int f_lo, int f_hi, int cap_events,
                       int* n_events, int* events, int* occupancy, int* status, hipStream_t s);

// the checks of aic_zones_create / aic_zones_set: nothing is touched before they pass
void zones_check_params(int streams, int max_tracks, int forget_after, int anchor);

struct Zones {
    int device_id;
    Device* dev = nullptr;                       // resolved by the first update
    int n_streams, max_tracks, forget_after, anchor;
    int frames_per_launch = 0;                   // 0: a call's frames in one walk launch; k: at most k frames of a stream per launch
    std::vector<int> h_geo;                      // [streams][ZONES_GEO_INTS]
    std::vector<char> geo_dirty, reset_pending;  // what the next update stages
    std::vector<int> stop;                       // 0 or the code a stream stopped with
    DevBuf<int> d_geo, d_state, d_stage, d_cls4, d_out;
    DevBuf<long long> d_cnt;
    PinBuf<int> h_stage, h_out;
    PinBuf<long long> h_cnt;

    Zones(int device, int streams, int max_tracks_, int forget_after_, int anchor_);
    void set(int stream, int n_zones, const int32_t* zone_nvert, const int32_t* zone_xy, int n_lines, const int32_t* line_xy);
    void reset(int stream);
    void update(const int32_t* fps, const int32_t* counts, const int32_t* rows6, int mem, int cap_events, int32_t* n_events, int32_t* events,
                int32_t* occupancy, int32_t* status);
    void counters(int stream, int64_t* zone_in, int64_t* zone_out, int64_t* line_pos, int64_t* line_neg);
};

}  // namespace aic

struct aic_zones {
    aic::Zones z;
    aic_zones(int device, int streams, int max_tracks, int forget_after, int anchor) : z(device, streams, max_tracks, forget_after, anchor) {}
};
