// prox.hpp -- proximity: ground plane, speed, pairs and parties per camera, on the device (prox.cpp, C ABI aic_prox_*; kernels_prox.hip;
// prox_math.hpp).  A tracker-agnostic stage over the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32),
// for a bank of 1..256 cameras per call; no frames.  Every camera holds a table of max_tracks slots (slot_walk.hpp) that remembers where
// each track stood last, how fast it is and whom it has been with, and a resident table with one 8-byte entry per unordered PAIR of slots
// (linked, on, off, since).  A track that ends hands over a 16-int summary.  Integer arithmetic only -- tests/prox_oracle.py is the
// specification, bit for bit.
//
// Memory.  Resident: the slot tables, streams * PX_ST_INTS ints (32.8 KB a camera), and the pair tables, 8 bytes per slot pair:
// max_tracks (max_tracks - 1) / 2 entries a camera -- 65 KB a camera and 16.6 MB for 256 cameras at max_tracks 128; 1.05 MB a camera and
// 268 MB for 256 cameras at max_tracks 512.  Per launch: 32 bytes a row (tags) and 64 + 4 + cap_pairs * 32 bytes a frame (record, count,
// pair events).  All are allocated by the first call that reaches the device and grown on demand; an allocation that does not fit fails
// that call with AIC_ERR_CAPACITY.  create, option, reset and set_ground never touch the device.
//
// A pair entry is all zero whenever either slot is taken by a new track: the walk clears a new slot's max_tracks - 1 entries before the
// tick's pairs are judged, so the table needs no generation and a reset needs no pass over it (every slot is taken anew behind a reset).
#pragma once
#include "bank_stage.hpp"
#include "prox_math.hpp"

namespace aic {

constexpr int PX_STREAMS_MAX = 256;
constexpr int PX_ROWS_MAX = 512;           // rows per frame = threads of the walk block
constexpr int PX_TRACKS_MAX = SLOT_TRACKS;
constexpr int PX_COORD_MAX = 1 << 20;
constexpr int PX_DIM_MAX = 16384;
constexpr int PX_CAP_MAX = 4096;
constexpr int PX_CAP_PAIRS_MAX = 4096;
constexpr int PX_TICKS_MAX = 1 << 16;
constexpr int PX_EVENT_INTS = 16, PX_RECORD_INTS = 16, PX_TAG_INTS = 8, PX_PAIR_EVENT_INTS = 8;

// state of one stream, ints: frame, status, 6 unused | 16 arrays of 512: the six of every slot table, then these
enum { PX_A_GX = SLOT_A_SHARED, PX_A_GY, PX_A_PLACED, PX_A_VQ8, PX_A_GAIT, PX_A_DIST, PX_A_MAXV, PX_A_PTICKS, PX_A_MAXP, PX_A_LINKS, PX_ARRAYS };
constexpr int PX_ST_INTS = SLOT_ST_SLOTS + PX_ARRAYS * PX_TRACKS_MAX;

struct ProxGeom {                          // what sizes buffers, and the frame
    int streams, h, w, max_tracks;
    size_t pairs() const { return (size_t)max_tracks * (max_tracks - 1) / 2; }      // entries of one stream
};

// where a launch writes: records [frames of the launch, 16], n_pair_events [frames], pair_events [frames, cap_pairs, 8] (zeroed by the host),
// row_tags [rows of the launch, 8]; row0 = the call's row index of the launch's first row
struct ProxOut {
    int *records, *n_pair_events, *pair_events, *row_tags;
    int cap_pairs, row0;
};

// kernels_prox.hip
// One block per stream walks the launch's n_ticks ticks in order; n_ticks == 0: mode[stream] (drain / flush).  first != 0: the launch
// applies pending resets and starts the call's output lists.  grounds [streams]; pairs [streams, g.pairs()] int2.
void launch_prox_walk(const int* frame_off, int n_ticks, const int* rows6, const int* reset, const int* mode, int first, const ProxGeom& g,
                      int forget_after, const ProxRules& r, const ProxGround* grounds, int* state, int* pairs, int cap, int* n_final, int* pending,
                      int* status, int* events, const ProxOut& o, hipStream_t s);

void prox_check_params(int device, const aic_prox_config* p);

struct ProxOptions {                       // what option may change between calls
    int forget_after, metric, near, height_ratio_q8, link_ticks, unlink_ticks, speed_shift, still_speed, run_speed;
};

struct Prox : SlotBank {
    ProxGeom g;
    ProxOptions o;
    std::vector<ProxGround> grounds;       // per stream; uploaded with every call that walks
    DevBuf<int> d_state, d_pairs, d_rec, d_pe, d_tags, d_ground;
    std::vector<int> h_state, h_pairs;

    Prox(int device, const aic_prox_config& p);
    void option(const std::string& k, int value);
    void reset(int stream);
    void set_ground(int stream, const int32_t* H, int shift);
    void update(int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int cap_pairs, int32_t* n_final, int32_t* events,
                int32_t* pending, int32_t* status, int32_t* records, int32_t* row_tags, int32_t* n_pair_events, int32_t* pair_events);
    void flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status);
    void export_stream(int stream, int32_t* n, int32_t* events);
    void export_pairs(int stream, int32_t* n, int32_t* out6);

private:
    void touch_device();
    bool fetch_state(int stream);
    void walk(const int* d_off, int n_ticks, const int* d_rows, const BankStage& bs, int first, int cap, const SlotOut& so, const ProxOut& po);
};

}  // namespace aic

struct aic_prox {
    aic::Prox c;
    aic_prox(int device, const aic_prox_config& p) : c(device, p) {}
};
