// bestshot.hpp -- the best crop of every track, kept on the device, per camera (bestshot.cpp, C ABI aic_bestshot_*;
// kernels_bestshot.hip).  A tracker-agnostic stage over the frames and the rows every tracker here delivers
// (x1 y1 x2 y2 id cls, int32), for a bank of 1..256 cameras per call: every box of every frame is resampled to a TH x TW thumbnail by
// an integer area average and scored (sharpness x fill x visibility, halved when the frame clipped it); a table of max_tracks slots per
// stream keeps the best thumbnail per track id and hands it over when the track ends.  Integer arithmetic only --
// tests/bestshot_oracle.py is the specification, bit for bit.
//
// Memory.  The slot thumbnails are resident: streams * max_tracks * TH * TW * 3 bytes (805 MB at 256 x 128 x 64 x 128).  They, the
// per-row candidate buffer of a launch (rows of the launch * TH * TW * 3 bytes) and the staged frames of a launch (host frames only)
// are allocated by the first call that reaches the device and grown on demand; an allocation that does not fit fails that call with
// AIC_ERR_CAPACITY.  A call's ticks are cut into launches so that the candidate buffer and the staged frames each stay below
// launch_budget_mb (option, default 1024), one tick per launch at the least.  create, option and reset never touch the device.
#pragma once
#include "bank_stage.hpp"

namespace aic {

constexpr int BS_STREAMS_MAX = 256;
constexpr int BS_ROWS_MAX = 512;           // rows per frame = threads of the walk block
constexpr int BS_TRACKS_MAX = SLOT_TRACKS; // slots per stream
constexpr int BS_COORD_MAX = 1 << 20;
constexpr int BS_DIM_MAX = 16384;
constexpr int BS_CAP_MAX = 4096;           // finals per stream per call
constexpr int BS_TICKS_MAX = 1 << 16;
constexpr int BS_EVENT_INTS = 16;

enum { BS_LIVE = SLOT_LIVE, BS_EXPIRED = SLOT_EXPIRED, BS_FLUSHED = SLOT_FLUSHED };
enum { BS_REGION_BOX = 0, BS_REGION_HEAD = 1 };
// flags of a scored row
enum { BS_F_VALID = SLOT_F_VALID, BS_F_FIRST = SLOT_F_FIRST, BS_F_NONEMPTY = SLOT_F_NONEMPTY, BS_F_CAND = 8, BS_F_TRUNC = 16, BS_F_STORED = 32 };
// state of one stream, ints: frame, status, 6 unused | 13 arrays of 512: the six of every slot table (bank_call.hpp: id, state,
// last_seen, cls, first_frame, sightings), has_shot, best_frame, score, C.x0, C.y0, C.x1, C.y1
constexpr int BS_ST_SLOTS = SLOT_ST_SLOTS;
enum { BS_A_ID = SLOT_A_ID, BS_A_STATE = SLOT_A_STATE, BS_A_LAST = SLOT_A_LAST, BS_A_CLS = SLOT_A_CLS, BS_A_FIRST = SLOT_A_FIRST,
       BS_A_SIGHT = SLOT_A_SIGHT, BS_A_HAS = SLOT_A_SHARED, BS_A_BFRAME, BS_A_SCORE, BS_A_C0, BS_A_C1, BS_A_C2, BS_A_C3, BS_ARRAYS };
constexpr int BS_ST_INTS = BS_ST_SLOTS + BS_ARRAYS * BS_TRACKS_MAX;

struct BsGeom {                            // what the kernels need of aic_bestshot_config
    int streams, h, w, tw, th, max_tracks, forget_after, region, head_q8, pad, min_w, min_h;
};

// kernels_bestshot.hip
// One block per row of the launch (grid = frames of the launch x the most rows of one of them): info [rows, 8] = flags, score, C.x0,
// C.y0, C.x1, C.y1, 0, 0, and the thumbnail into cand [row - cand_base] when the row could still win.  frames: the launch's first
// frame; frame_off: the launch's first of n_frames + 1 row offsets (tick-major, frame x = tick x / S of stream x % S).
void launch_bestshot_score(const uint8_t* frames, const int* frame_off, int n_frames, int max_rows, const int* rows6, const int* state, const int* reset,
                           int first, const BsGeom& g, int cand_base, int* info, uint8_t* cand, hipStream_t s);
// One block per stream walks the launch's n_ticks ticks in order; n_ticks == 0: mode[stream] (drain / flush).  first != 0: the launch
// applies pending resets and starts the call's output lists.
void launch_bestshot_walk(const int* frame_off, int n_ticks, const int* rows6, const int* info, const uint8_t* cand, int cand_base, const int* reset,
                          const int* mode, int first, const BsGeom& g, int* state, uint8_t* slot_thumbs, int cap, int* n_final, int* pending,
                          int* status, int* events, uint8_t* out_thumbs, hipStream_t s);

// the checks of aic_bestshot_create: nothing is touched before they pass
void bestshot_check_params(int device, const aic_bestshot_config* p);

struct BestShot : SlotBank {
    BsGeom g;
    int stats = 0;                               // option "stats": 1 = every update reads its scored rows back and counts them
    int64_t n_rows = 0, n_candidates = 0, n_stored = 0;   // rows handed in, candidates scored, thumbnails the filter let through
    DevBuf<int> d_state, d_info;
    DevBuf<uint8_t> d_slot_thumbs, d_cand, d_out_thumbs;
    std::vector<int> h_state, h_info;

    BestShot(int device, const aic_bestshot_config& p);
    size_t thumb_bytes() const { return (size_t)g.tw * g.th * 3; }
    void reset(int stream) { reset_stream(stream, "stream outside the best-shot bank"); }
    void update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int32_t* n_final,
                int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status);
    void flush(int stream, int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status);
    void export_stream(int stream, int32_t* n, int32_t* events, uint8_t* thumbs);

private:
    void touch_device();
    SlotOut outputs(int cap);
    void walk(const int* d_off, int n_ticks, const int* d_rows, int cand_base, const BankStage& bs, int first, int cap, const SlotOut& so);
    void finish(int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status);
};

}  // namespace aic

struct aic_bestshot {
    aic::BestShot b;
    aic_bestshot(int device, const aic_bestshot_config& p) : b(device, p) {}
};
