// colours.hpp -- what each track wears, per camera, on the device (colours.cpp, C ABI aic_colours_*; kernels_colours.hip; DESIGN.md
// section 45).  A tracker-agnostic stage over the frames and the rows every tracker here delivers (x1 y1 x2 y2 id cls, int32), for a
// bank of 1..256 cameras per call: the pixels of a torso part and a legs part of every counted box are named (12 colours) and
// histogrammed; a table of max_tracks slots per stream accumulates each track's normalised histograms while it lives and hands over a
// 48-int descriptor when the track ends.  Integer arithmetic only -- tests/colours_oracle.py is the specification, bit for bit.
//
// Memory.  The slot tables are resident: streams * CL_ST_INTS ints (16.8 MB at 256 streams), the accumulators among them; they stay
// in HBM during a launch (kernels_colours.hip says why).  They, the per-row samples of a launch (128 bytes a row) and the staged frames
// of a launch (host frames only) are allocated by the first call that reaches the device and grown on demand; an allocation that does
// not fit fails that call with AIC_ERR_CAPACITY.  A call's ticks are cut into launches so that the samples and the staged frames each
// stay below launch_budget_mb (option, default 1024), one tick per launch at the least.  create, option and reset never touch the device.
#pragma once
#include "bank_stage.hpp"

namespace aic {

constexpr int CL_STREAMS_MAX = 256;
constexpr int CL_ROWS_MAX = 512;           // rows per frame = threads of the walk block
constexpr int CL_TRACKS_MAX = SLOT_TRACKS; // slots per stream
constexpr int CL_COORD_MAX = 1 << 20;
constexpr int CL_DIM_MAX = 16384;
constexpr int CL_CAP_MAX = 4096;           // finals per stream per call
constexpr int CL_TICKS_MAX = 1 << 16;
constexpr int CL_EVENT_INTS = 48;
constexpr int CL_INFO_INTS = 32;           // a sampled row: flags, n_upper, n_lower, 0, s[2][12], 4 zeros
constexpr int CL_BINS = 12;
constexpr int CL_SAMPLES_MAX = 1 << 20;    // samples per part and slot: acc <= 256 * 2^20 = 2^28 stays inside int32

enum { CL_LIVE = SLOT_LIVE, CL_EXPIRED = SLOT_EXPIRED, CL_FLUSHED = SLOT_FLUSHED };
enum { CL_BLACK = 0, CL_GRAY, CL_WHITE, CL_RED, CL_ORANGE, CL_YELLOW, CL_GREEN, CL_CYAN, CL_BLUE, CL_PURPLE, CL_PINK, CL_BROWN };
// flags of a sampled row
enum { CL_F_VALID = SLOT_F_VALID, CL_F_FIRST = SLOT_F_FIRST, CL_F_NONEMPTY = SLOT_F_NONEMPTY, CL_F_UPPER = 8, CL_F_LOWER = 16 };
// state of one stream, ints: frame, status, 6 unused | 8 arrays of 512: the six of every slot table (bank_call.hpp: id, state, last_seen,
// cls, first_frame, sightings), samples_upper, samples_lower | acc [512 slots][2 parts][12 bins]
constexpr int CL_ST_SLOTS = SLOT_ST_SLOTS;
enum { CL_A_ID = SLOT_A_ID, CL_A_STATE = SLOT_A_STATE, CL_A_LAST = SLOT_A_LAST, CL_A_CLS = SLOT_A_CLS, CL_A_FIRST = SLOT_A_FIRST,
       CL_A_SIGHT = SLOT_A_SIGHT, CL_A_NU = SLOT_A_SHARED, CL_A_NL, CL_ARRAYS };
constexpr int CL_ST_ACC = CL_ST_SLOTS + CL_ARRAYS * CL_TRACKS_MAX;
constexpr int CL_ST_INTS = CL_ST_ACC + CL_TRACKS_MAX * 2 * CL_BINS;

struct ColGeom {                           // what the kernels need of aic_colours_config
    int streams, h, w, max_tracks, forget_after, t0, t1, l0, l1, inset_q8, min_w, min_h, max_cover_q8;
};

// ---- the pixel rule, shared by the sample kernel and aic_colours_classify -----------------------------------------------------------
// floor(n / d) for 0 <= n < 2^17 and 1 <= d <= 255 as a multiply by m = ceil(2^31 / d): with e = m d - 2^31 < d the product n m / 2^31
// exceeds n / d by n e / (d 2^31) < 2^17 / 2^31, less than the 1 / d that separates n / d from the next integer: exact.
// tests/test_colours_oracle.py enumerates every (numerator, d) the rule can produce.
__host__ __device__ inline unsigned cl_recip(unsigned d) { return d ? (0x80000000u + d - 1u) / d : 0u; }
__host__ __device__ inline int cl_div(unsigned n, unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)__umulhi(2u * n, m);
#else
    return (int)(((unsigned long long)(2u * n) * m) >> 32);
#endif
}
// recip[d] = cl_recip(d) for d in 0..255
__host__ __device__ inline int cl_classify(int b, int g, int r, const unsigned* recip) {
    const int mx = b > g ? (b > r ? b : r) : (g > r ? g : r);
    const int mn = b < g ? (b < r ? b : r) : (g < r ? g : r);
    const int d = mx - mn;
    if (mx < 40) return CL_BLACK;
    const int sat = cl_div((unsigned)d << 8, recip[mx]);
    if (sat < 40) return mx < 72 ? CL_BLACK : mx < 200 ? CL_GRAY : CL_WHITE;
    int diff, base;                                                          // ties on the maximum: r, then g, then b
    if (mx == r) diff = g - b, base = 0;
    else if (mx == g) diff = b - r, base = 512;
    else diff = r - g, base = 1024;
    const unsigned m = recip[d];
    int hq = base + (diff >= 0 ? cl_div((unsigned)diff << 8, m) : -cl_div(((unsigned)(-diff) << 8) + d - 1, m));      // floor division
    if (hq < 0) hq += 1536;                                                  // (the r case alone can be negative)
    int c = (hq >= 1472 || hq < 64) ? CL_RED : hq < 192 ? CL_ORANGE : hq < 299 ? CL_YELLOW : hq < 704 ? CL_GREEN : hq < 853 ? CL_CYAN
            : hq < 1109 ? CL_BLUE : hq < 1300 ? CL_PURPLE : CL_PINK;
    if (c == CL_ORANGE && mx < 176) c = CL_BROWN;
    if (c == CL_YELLOW && mx < 136) c = CL_BROWN;
    if (c == CL_RED && sat < 128 && mx >= 176) c = CL_PINK;
    return c;
}

// top / second / hist of one part from its 12 accumulators (the event's and the row tag's arithmetic); hist may be NULL
__host__ __device__ inline void cl_describe(const int* acc, int samples, int* top, int* second, int* hist) {
    int t = -1, s2 = -1;
    if (samples > 0) {
        t = 0;
        for (int k = 1; k < CL_BINS; ++k)
            if (acc[k] > acc[t]) t = k;
        int best = 0;
        for (int k = 0; k < CL_BINS; ++k)
            if (k != t && acc[k] > best) best = acc[k], s2 = k;
        if (s2 >= 0 && (long long)best * 4 < acc[t]) s2 = -1;
    }
    *top = t, *second = s2;
    if (hist)
        for (int k = 0; k < CL_BINS; ++k) hist[k] = samples > 0 ? acc[k] / samples : 0;
}

// kernels_colours.hip
// One block per row of the launch (grid = frames of the launch x the most rows of one of them): info [row - info_base, 32].  frames: the
// launch's first frame; frame_off: the launch's first of n_frames + 1 row offsets (tick-major, frame x = tick x / S of stream x % S).
void launch_colours_sample(const uint8_t* frames, const int* frame_off, int n_frames, int max_rows, const int* rows6, const int* state, const int* reset,
                           int first, const ColGeom& g, int info_base, int* info, hipStream_t s);
// One block per stream walks the launch's n_ticks ticks in order; n_ticks == 0: mode[stream] (drain / flush).  first != 0: the launch
// applies pending resets and starts the call's output lists.  row_tags (may be NULL) [rows of the call, 4].
void launch_colours_walk(const int* frame_off, int n_ticks, const int* rows6, const int* info, int info_base, const int* reset, const int* mode,
                         int first, const ColGeom& g, int* state, int cap, int* n_final, int* pending, int* status, int* events, int* row_tags,
                         hipStream_t s);

// the checks of aic_colours_create: nothing is touched before they pass
void colours_check_params(int device, const aic_colours_config* p);

struct Colours : SlotBank {
    ColGeom g;
    DevBuf<int> d_state, d_info, d_tags;
    std::vector<int> h_state;

    Colours(int device, const aic_colours_config& p);
    void reset(int stream) { reset_stream(stream, "stream outside the colour bank"); }
    void update(const void* frames, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int32_t* n_final,
                int32_t* events, int32_t* row_tags, int32_t* pending, int32_t* status);
    void flush(int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status);
    void export_stream(int stream, int32_t* n, int32_t* events);

private:
    void touch_device();
    void walk(const int* d_off, int n_ticks, const int* d_rows, int info_base, const BankStage& bs, int first, int cap, const SlotOut& so, int* d_rt);
};

}  // namespace aic

struct aic_colours {
    aic::Colours c;
    aic_colours(int device, const aic_colours_config& p) : c(device, p) {}
};
