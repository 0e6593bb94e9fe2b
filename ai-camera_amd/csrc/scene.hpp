// scene.hpp -- scene watch: motion masks, an activity gate and tamper alarms per camera (scene.cpp, C ABI aic_scene_*;
// kernels_scene.hip).  A tracker-agnostic stage over the frames (and, optionally, the rows every tracker here
// delivers) for a bank of 1..256 cameras per call: every frame is reduced to a coarse gray grid (cells of c x c pixels), a running
// background model per cell marks what moved, a 3 x 3 vote cleans the mask, and per-stream counters turn the tick's statistics into
// the activity gate and the five alarms (dark, bright, defocus, scene change, frozen).  Integer arithmetic only --
// tests/scene_oracle.py is the specification, bit for bit.
//
// Memory.  Resident: 5 bytes per cell and stream (bg and dev as u16 Q8, prev as u8) and 16 ints per stream.  Per launch: three bytes
// per cell and frame of the launch (gray, model bits, mask), 12 ints per frame, and for host frames the staged frames.  All of it is
// allocated by the first call that reaches the device and grown on demand; an allocation that does not fit fails that call with
// AIC_ERR_CAPACITY.  A call's ticks are cut into launches so that the gray buffer and the staged frames each stay below
// launch_budget_mb (option, default 1024), one tick per launch at the least.  create, option and reset never touch the device.
#pragma once
#include "bank_stage.hpp"

namespace aic {

constexpr int SC_STREAMS_MAX = 256;
constexpr int SC_ROWS_MAX = 512;
constexpr int SC_COORD_MAX = 1 << 20;
constexpr int SC_DIM_MAX = 16384;
constexpr int SC_TICKS_MAX = 1 << 16;
constexpr int SC_SAT = 1 << 30;
constexpr int SC_RECORD_INTS = 16;
constexpr int SC_KINDS = 5;
enum { SC_DARK = 1, SC_BRIGHT = 2, SC_DEFOCUS = 4, SC_SCENE = 8, SC_FROZEN = 16 };
// model bits of a cell and tick; mask bits
enum { SC_B_RAW = 1, SC_B_CHANGED = 2, SC_B_DIFF = 4 };
enum { SC_M_CLEAN = 1, SC_M_RAW = 2 };
// scalars of one stream, ints: age, quiet, ref_q8, alarms, on[5], off[5], 2 unused
enum { SC_S_AGE = 0, SC_S_QUIET, SC_S_REF, SC_S_ALARM, SC_S_ON, SC_S_OFF = SC_S_ON + SC_KINDS, SC_S_INTS = 16 };
// accumulators of one frame of a launch, ints: counts, the box (encoded so that 0 = none), two 64-bit sums
enum { SC_A_RAW = 0, SC_A_MOVING, SC_A_CHANGED, SC_A_DIFF, SC_A_X0, SC_A_Y0, SC_A_X1, SC_A_Y1, SC_A_SUM_G, SC_A_SUM_SHARP = 10, SC_A_INTS = 12 };

struct ScGeom {
    int streams, h, w, c, hc, wc;
};
struct ScOpts {
    int thresh = 6, noise_k_q4 = 64, warmup = 16, big_thresh = 24, learn_shift = 4, slow_extra = 3, dev_init_q8 = 512, min_neighbours = 3,
        dark_luma = 16, bright_luma = 240, min_ref_q8 = 512, defocus_q8 = 96, scene_q16 = 39322, ref_shift = 6, hold = 25, gate_cells = 4,
        gate_hold = 30;
};

// kernels_scene.hip
// gray [n_frames, hc, wc] of n_frames frames [h, w, 3]; 16-byte loads when the base and the pitch 3 w are multiples of 16
void launch_scene_gray(const uint8_t* frames, int n_frames, const ScGeom& g, uint8_t* gray, hipStream_t s);
// a thread owns a cell of a stream and walks the launch's ticks in order: bits [n_ticks, S, hc, wc]
void launch_scene_model(const uint8_t* gray, int n_ticks, const ScGeom& g, const ScOpts& o, const int* scalars, const int* reset, int first,
                        uint16_t* bg, uint16_t* dev, uint8_t* prev, uint8_t* bits, hipStream_t s);
// stateless per frame: mask [n_frames, hc, wc] and acc [n_frames, 12] (zeroed by the caller)
void launch_scene_stats(const uint8_t* gray, const uint8_t* bits, int n_frames, const ScGeom& g, const ScOpts& o, uint8_t* mask, int* acc,
                        hipStream_t s);
// one wave per row: row_motion [rows]; frame_off: the launch's first of n_frames + 1 row offsets
void launch_scene_rows(const uint8_t* mask, const int* frame_off, int n_frames, int max_rows, const int* rows6, const ScGeom& g, int* row_motion,
                       hipStream_t s);
// one thread per stream walks the launch's ticks: records [n_ticks, S, 16]
void launch_scene_walk(const int* acc, int n_ticks, const ScGeom& g, const ScOpts& o, const int* reset, int first, int* scalars, int* records,
                       hipStream_t s);

void scene_check_config(int device, const aic_scene_config* p);

struct Scene : FrameBank {
    ScGeom g;
    ScOpts o;
    DevBuf<uint16_t> d_bg, d_dev;
    DevBuf<uint8_t> d_prev, d_gray, d_bits, d_mask;
    DevBuf<int> d_scalars, d_acc, d_rec, d_rm;

    Scene(int device, const aic_scene_config& p);
    size_t cells() const { return (size_t)g.hc * g.wc; }
    void option(const std::string& key, int value);
    void reset(int stream) { reset_streams(stream, "stream outside the scene bank (-1 = every stream)"); }
    void update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int32_t* records,
                uint8_t* masks, int32_t* row_motion);
    void export_stream(int stream, int32_t* bg, int32_t* dv, int32_t* prev, int32_t* scalars);

private:
    void touch_device();
};

}  // namespace aic

struct aic_scene {
    aic::Scene s;
    aic_scene(int device, const aic_scene_config& p) : s(device, p) {}
};
