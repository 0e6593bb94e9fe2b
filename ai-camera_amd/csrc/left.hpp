// left.hpp -- left objects: abandoned and removed items per camera (left.cpp, C ABI aic_left_*; kernels_left.hip; DESIGN.md
// section 44).  A tracker-agnostic stage over the frames and the rows every tracker here delivers, for a bank of 1..256 cameras per
// call: the gray grid of the scene watch (launch_scene_gray, unchanged), a two-speed background per cell that knows which cells
// people cover, the 8-connected blobs of the cells that stayed changed, and per stream a small table of objects that are matched
// from tick to tick, alarmed as LEFT or REMOVED and ended.  Integer arithmetic only -- tests/left_oracle.py is the specification,
// bit for bit.
//
// Memory.  Resident: 14 bytes per cell and stream (fast, slow, still as u16; last_id, last_tick as i32), 4 ints per stream and 12 ints
// per slot.  Per launch: 16 bytes per cell and frame of the launch (gray, occupied, occ_id, cand, slow >> 8, the owner's tick and id;
// 20 with labels asked for), the blob tables, the objects and the events of its frames, and for host frames the staged frames.  All
// of it is allocated by the first call that reaches the device and grown on demand; an allocation that does not fit fails that call
// with AIC_ERR_CAPACITY.  A call's ticks are cut into launches so that the per-cell buffers and the staged frames each stay below
// launch_budget_mb (option, default 1024), one tick per launch at the least.  create, option and reset never touch the device.
#pragma once
#include "scene.hpp"

namespace aic {

constexpr int LF_CELLS_MAX = 32768;              // the labels of a frame are u16 in LDS: cell index + 1
constexpr int LF_BLOBS_MAX = 64;
constexpr int LF_OBJECTS_MAX = 64;
constexpr int LF_RECORD_INTS = 8;
constexpr int LF_OBJECT_INTS = 12;
constexpr int LF_EVENT_INTS = 12;
constexpr int LF_NONE = 0x7fffffff;
enum { LF_APPEARED = 1, LF_RAISED = 2, LF_ENDED = 3 };
enum { LF_KIND_LEFT = 1, LF_KIND_REMOVED = 2 };
// a slot, ints: the box in cells, x1 y1 inclusive
enum { LF_O_UID = 0, LF_O_KIND, LF_O_ALARMED, LF_O_X0, LF_O_Y0, LF_O_X1, LF_O_Y1, LF_O_OWNER, LF_O_BORN, LF_O_AREA, LF_O_SEEN, LF_O_MISSING };
// a blob of a frame's table, ints: the box in cells, x1 y1 inclusive
enum { LF_B_AREA = 0, LF_B_X0, LF_B_Y0, LF_B_X1, LF_B_Y1, LF_B_CNOW, LF_B_CBG, LF_B_OWNER, LF_BLOB_INTS };
// the head of a frame's table, ints: candidate cells, blobs of a kept size (not capped at 64)
enum { LF_H_CAND = 0, LF_H_KEPT, LF_HEAD_INTS = 4 };
// scalars of one stream, ints: age, uids issued, 2 unused
enum { LF_S_AGE = 0, LF_S_UIDS, LF_S_INTS = 4 };

struct LfOpts {
    int fast_shift = 3, slow_shift = 8, thresh = 10, warmup = 16, decay = 2, min_ticks = 50, absorb_ticks = 9000, pad_cells = 1, owner_window = 150,
        min_cells = 2, max_cells = 4096, alarm_hold = 25, gone_ticks = 15;
};

// the resident cell state of all streams, [S, hc, wc] each
struct LfCells {
    uint16_t *fast, *slow, *still;
    int *last_id, *last_tick;
};
// what a launch's frames carry between the kernels, [n_frames, hc, wc] each
struct LfFrames {
    uint8_t *gray, *occ, *cand, *slow8;
    int *occ_id, *own_tick, *own_id;
};

// kernels_left.hip
// one wave per row: occ = 1 and occ_id = min(id) over the cells a valid row's padded box covers (occ zeroed, occ_id preset to LF_NONE by
// the caller); frame_off: the launch's first of n_frames + 1 row offsets
void launch_left_occupancy(const int* frame_off, int n_frames, int max_rows, const int* rows6, const ScGeom& g, int pad_cells, uint8_t* occ,
                           int* occ_id, hipStream_t s);
// a thread owns a cell of a stream and walks the launch's ticks in order
void launch_left_model(const LfFrames& fr, int n_ticks, const ScGeom& g, const LfOpts& o, const int* scalars, const int* reset, int first,
                       const LfCells& cells, hipStream_t s);
// one block per frame: the 8-connected components of cand in LDS, then head [n_frames, 4] and blobs [n_frames, 64, 8]; labels (may be
// NULL) [n_frames, hc, wc], -1 = none
void launch_left_blobs(const LfFrames& fr, int n_frames, const ScGeom& g, const LfOpts& o, int* head, int* blobs, int* labels, hipStream_t s);
// one thread per stream walks the launch's ticks: slots [S, M, 12], records [n_ticks, S, 8], objects [n_ticks, S, M, 12],
// ev_count [n_ticks * S] and ev [n_ticks * S, 2 M, 12]; tick0: the launch's first tick of the call
void launch_left_walk(const int* head, const int* blobs, int n_ticks, int tick0, const ScGeom& g, const LfOpts& o, int max_objects, const int* reset,
                      int first, int* scalars, int* slots, int* records, int* objects, int* ev_count, int* ev, hipStream_t s);
// packs the launch's events behind those of the call's earlier launches: out [cap, 12], *total counts on past cap
void launch_left_events(const int* ev_count, const int* ev, int n_frames, int max_objects, int cap, int* out, int* total, hipStream_t s);

void left_check_config(int device, const aic_left_config* p);

struct Left : FrameBank {
    ScGeom g;
    int max_objects;
    LfOpts o;
    DevBuf<uint16_t> d_fast, d_slow, d_still;
    DevBuf<uint8_t> d_gray, d_occ, d_cand, d_slow8;
    DevBuf<int> d_last_id, d_last_tick, d_occ_id, d_own_tick, d_own_id, d_labels, d_scalars, d_slots, d_head, d_blobs, d_rec, d_obj, d_evc, d_ev,
        d_events, d_total;

    Left(int device, const aic_left_config& p);
    size_t cells() const { return (size_t)g.hc * g.wc; }
    void option(const std::string& key, int value);
    void reset(int stream) { reset_streams(stream, "stream outside the bank (-1 = every stream)"); }
    void update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap_events,
                int32_t* records, int32_t* objects, int32_t* events, int32_t* n_events, int32_t* status, uint8_t* cand, int32_t* labels);
    void export_stream(int stream, int32_t* fast, int32_t* slow, int32_t* still, int32_t* last_id, int32_t* last_tick, int32_t* slots,
                       int32_t* scalars);

private:
    void touch_device();
};

}  // namespace aic

struct aic_left {
    aic::Left s;
    aic_left(int device, const aic_left_config& p) : s(device, p) {}
};
