// heat.hpp -- heat maps: footfall, dwell, flow and paths per camera, on the device (heat.cpp, C ABI aic_heat_*; kernels_heat.hip;
// heat_math.hpp).  A tracker-agnostic stage over the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32),
// for a bank of 1..256 cameras per call; only render touches frames.  Every camera holds twelve int32 layers over a grid of cell x cell
// pixels (VISITS, DWELL, STARTS, ENDS, DIR0..DIR7) and a table of max_tracks slots (slot_walk.hpp) that remembers where each track stood
// last, so that "entered a new cell" and "moved this way" are defined; a track that ends hands over a 16-int path summary.  Integer
// arithmetic only -- tests/heat_oracle.py is the specification, bit for bit.
//
// ENDS[the slot's cell] is counted when the track's event LEAVES THE TABLE (the variant's event hook), not when the slot expires: a
// track waiting in `pending` is not yet in ENDS, and after a drain the sums are what expiry would have given.  This keeps slot_walk.hpp
// untouched.
//
// Memory.  Resident: 48 bytes per cell and camera (12 layers; at most 32768 cells, 1.5 MB a camera) and the slot tables,
// streams * HT_ST_INTS ints (32.8 KB a camera).  They, the row tags of a call (16 bytes a row), the u16 levels of a render call (2 bytes
// per cell and camera) and the staged frames of a render chunk (host frames only) are allocated by the first call that reaches the device
// and grown on demand; an allocation that does not fit fails that call with AIC_ERR_CAPACITY.  create, option, reset, set_lut and the
// range check of import_layers never touch the device.
#pragma once
#include "bank_stage.hpp"
#include "heat_math.hpp"

namespace aic {

constexpr int HT_STREAMS_MAX = 256;
constexpr int HT_ROWS_MAX = 512;           // rows per frame = threads of the walk block
constexpr int HT_TRACKS_MAX = SLOT_TRACKS;
constexpr int HT_COORD_MAX = 1 << 20;
constexpr int HT_DIM_MAX = 16384;
constexpr int HT_CELLS_MAX = 32768;
constexpr int HT_CAP_MAX = 4096;
constexpr int HT_TICKS_MAX = 1 << 16;
constexpr int HT_EVENT_INTS = 16;
constexpr int HT_FRAMES_MAX = 1 << 16;     // frames of a render call
constexpr int HT_BAND = 8;                 // pixel rows of a render block

// state of one stream, ints: frame, status, 6 unused | 16 arrays of 512: the six of every slot table, then these
enum { HT_A_CELL = SLOT_A_SHARED, HT_A_FX, HT_A_FY, HT_A_SFX, HT_A_SFY, HT_A_PATH, HT_A_INCELL, HT_A_MAXSTEP, HT_A_CELLS, HT_A_MOVING, HT_ARRAYS };
constexpr int HT_ST_INTS = SLOT_ST_SLOTS + HT_ARRAYS * HT_TRACKS_MAX;

struct HeatGeom {                          // what the kernels need of aic_heat_config
    int streams, h, w, lc, gw, gh, max_tracks, forget_after, anchor, min_move;
    int cells() const { return gw * gh; }
};

struct HeatOptions {
    int scale = HEAT_LOG, alpha_q8 = 160, floor = 8, chunk_frames = 0;
};

// kernels_heat.hip
// One block per stream walks the launch's n_ticks ticks in order; n_ticks == 0: mode[stream] (drain / flush).  first != 0: the launch
// applies pending resets of the TABLE (the layers of a reset stream are zeroed by the host, in stream order) and starts the call's
// output lists.  layers [streams, 12, cells]; row_tags (may be NULL) [rows of the call, 4].
void launch_heat_walk(const int* frame_off, int n_ticks, const int* rows6, const int* reset, const int* mode, int first, const HeatGeom& g, int* state,
                      int* layers, int cap, int* n_final, int* pending, int* status, int* events, int* row_tags, hipStream_t s);
// v >>= shift on the masked layers of one stream (or of all, stream = -1)
void launch_heat_decay(int* layers, const HeatGeom& g, int stream, int layer_mask, int shift, hipStream_t s);
// the maximum and the u16 levels of one layer of the n_used cameras used[]: maxima [streams], levels [streams, cells]
void launch_heat_levels(const int* layers, const HeatGeom& g, int layer, int scale, const int* used, int n_used, int* maxima, uint16_t* levels,
                        hipStream_t s);
// the per-pixel pass over n_frames BGR24 frames, in place; frame f shows camera frame_cam[f]; lut: 256 dwords B | G << 8 | R << 16
void launch_heat_render(uint8_t* frames, int n_frames, const int* frame_cam, const HeatGeom& g, const int* maxima, const uint16_t* levels,
                        const unsigned* lut, int alpha_q8, int floor, hipStream_t s);

// the checks of aic_heat_create: nothing is touched before they pass
void heat_check_params(int device, const aic_heat_config* p);
HeatGeom heat_geom(const aic_heat_config& p);
void heat_default_lut(uint8_t* bgr);       // 256 x 3

struct Heat : SlotBank {
    HeatGeom g;
    HeatOptions o;
    DevBuf<int> d_state, d_layers, d_tags, d_max;
    DevBuf<uint16_t> d_levels;
    DevBuf<unsigned> d_lut;
    std::vector<char> layer_reset;         // the stream's layers are zeroed by the next call that reaches the device
    std::vector<int> h_state;
    unsigned lut[256];
    bool lut_dirty = true;

    Heat(int device, const aic_heat_config& p);
    void option(const std::string& k, int value);
    void reset(int stream);
    void update(int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int32_t* n_final, int32_t* events, int32_t* row_tags,
                int32_t* pending, int32_t* status);
    void flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status);
    void export_stream(int stream, int32_t* n, int32_t* events);
    void decay(int stream, int layer_mask, int shift);
    void export_layers(int stream, int layer_mask, int32_t* out);
    void import_layers(int stream, int layer_mask, const int32_t* in);
    void set_lut(const uint8_t* bgr);
    void render(void* frames, int n_frames, int mem, const int32_t* cameras, int layer);

private:
    void touch_device();
    void walk(const int* d_off, int n_ticks, const int* d_rows, const BankStage& bs, int first, int cap, const SlotOut& so, int* d_rt);
};

}  // namespace aic

struct aic_heat {
    aic::Heat c;
    aic_heat(int device, const aic_heat_config& p) : c(device, p) {}
};
