// epoch_stage.hpp -- the one staging layout of every tracker call that runs the epoch kernels: where a call's detections
// and output rows lie in its pinned buffer and in the device mirror, how they are filled, and how the rows are delivered.  Host arithmetic on raw
// base pointers: no HIP call, nothing but trk_dev.hpp and the standard library (tests/epoch_stage_check.cpp builds it with the system compiler).
// Growing the buffers, the copies and the syncs are the callers'.
//   [the caller's prefix] | frame_n[F] | frame_d0[F] | tlwh[n*4] | conf[n] | cls[n] | (valid[n]) | [the caller's input suffix]
//   || n_tracks[F] | rows[F*cap*6] | conf[F*cap] | [the caller's output suffix]
// frame_n, tlwh (read with 16-byte vector loads) and || (the output half: what comes back) start on 16-byte boundaries.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "trk_dev.hpp"

namespace aic {

inline size_t up16(size_t x) { return (x + 15) / 16 * 16; }

struct StageCursor {                // hands out the fields of a layout in the order they lie
    size_t at = 0;
    size_t take(size_t bytes, bool align16 = false) { const size_t o = align16 ? up16(at) : at; at = o + bytes; return o; }
};

// frame_n[F] | frame_d0[F] | tlwh[n*4] | conf[n] | cls[n] | valid[n] (when asked)
struct DetBlock {
    size_t F, n, o_n, o_d0, o_tlwh, o_conf, o_cls, o_valid;
    bool has_valid;
    DetBlock(StageCursor& c, size_t frames, size_t rows, bool valid) : F(frames), n(rows), has_valid(valid) {
        o_n = c.take(F * 4, true), o_d0 = c.take(F * 4), o_tlwh = c.take(n * 16, true), o_conf = c.take(n * 4), o_cls = c.take(n * 4);
        o_valid = valid ? c.take(n * 4) : 0;
    }
    // counts and their prefix sums; boxes as tlwh, or as xyxy -> tlwh in fp32 (the detection format of every tracker here)
    void fill(char* h, const int32_t* counts, const float* boxes, bool xyxy, const float* conf, const int32_t* cls) const {
        int32_t* hn = reinterpret_cast<int32_t*>(h + o_n);
        int32_t* hd = reinterpret_cast<int32_t*>(h + o_d0);
        int32_t d0 = 0;
        for (size_t f = 0; f < F; ++f) { hn[f] = counts[f]; hd[f] = d0; d0 += counts[f]; }
        if (!n) return;
        float* ht = reinterpret_cast<float*>(h + o_tlwh);
        if (!xyxy) std::memcpy(ht, boxes, n * 16);
        else
            for (size_t j = 0; j < n; ++j) {
                const float* b = boxes + j * 4;
                ht[j * 4 + 0] = b[0], ht[j * 4 + 1] = b[1], ht[j * 4 + 2] = b[2] - b[0], ht[j * 4 + 3] = b[3] - b[1];
            }
        std::memcpy(h + o_conf, conf, n * 4);
        std::memcpy(h + o_cls, cls, n * 4);
    }
    // the DeepSORT entries' rule: a row is valid when the call has features and the row is not marked as without one (has NULL = none is)
    template <class T>
    void fill_valid(char* h, bool any_feat, const T* has) const {
        int32_t* hv = reinterpret_cast<int32_t*>(h + o_valid);
        for (size_t j = 0; j < n; ++j) hv[j] = (any_feat && (!has || has[j])) ? 1 : 0;
    }
    const int32_t* host_n(const char* h) const { return reinterpret_cast<const int32_t*>(h + o_n); }
    const int32_t* host_d0(const char* h) const { return reinterpret_cast<const int32_t*>(h + o_d0); }
    EpochDets dets(const char* d, const float* feat = nullptr, const float* feat_n = nullptr) const {
        return EpochDets{reinterpret_cast<const int32_t*>(d + o_n), reinterpret_cast<const int32_t*>(d + o_d0),
                         reinterpret_cast<const float*>(d + o_tlwh), reinterpret_cast<const float*>(d + o_conf),
                         reinterpret_cast<const int32_t*>(d + o_cls), has_valid ? reinterpret_cast<const int32_t*>(d + o_valid) : nullptr,
                         feat, feat_n};
    }
};

struct OutViews { const int32_t* n; const int32_t* rows; const float* conf; };   // the output block on the host, behind the read-back

// n_tracks[F] | rows[F*cap*6] | conf[F*cap], 16-byte aligned, rows at up16(F*4) behind the start
struct OutBlock {
    size_t o_out, o_rows, o_conf, end;
    int cap;
    OutBlock(StageCursor& c, size_t F, int cap_rows) : cap(cap_rows) {
        o_out = c.take(up16(F * 4), true), o_rows = c.take(F * cap * 24), o_conf = c.take(F * cap * 4), end = c.at;
    }
    EpochOut out(char* d, int32_t* dbg_match = nullptr, int32_t* dbg_tn = nullptr, int dbg_stride = 0) const {
        return EpochOut{reinterpret_cast<int32_t*>(d + o_out), reinterpret_cast<int32_t*>(d + o_rows), reinterpret_cast<float*>(d + o_conf),
                        cap, dbg_match, dbg_tn, dbg_stride};
    }
    OutViews host(const char* h) const {
        return OutViews{reinterpret_cast<const int32_t*>(h + o_out), reinterpret_cast<const int32_t*>(h + o_rows),
                        reinterpret_cast<const float*>(h + o_conf)};
    }
};

// Frame f of the output block -> frame o of the caller's arrays (any may be NULL): the true count, or 0 for a frame that is not good;
// the first min(count, cap) rows and confidences; what lies behind them in the caller's arrays is not touched.  Returns the count.
inline int deliver_frame(const OutViews& v, int cap, size_t f, bool good, size_t o, int32_t* n_out, int32_t* out6, float* out_conf) {
    const int m = good ? v.n[f] : 0, kk = std::min(m, cap);
    if (n_out) n_out[o] = m;                                  // the true count: rows beyond cap are not stored
    if (out6) std::copy(v.rows + f * cap * 6, v.rows + (f * cap + kk) * 6, out6 + o * cap * 6);
    if (out_conf) std::copy(v.conf + f * cap, v.conf + f * cap + kk, out_conf + o * cap);
    return m;
}

// A stream-major call: fps[S] frames per stream in the order they lie, good(stream, local frame) says which are delivered.
template <class Good>
inline void deliver(const OutViews& v, int cap, int S, const int32_t* fps, Good good, int32_t* n_out, int32_t* out6, float* out_conf) {
    size_t f = 0;
    for (int q = 0; q < S; ++q)
        for (int i = 0; i < fps[q]; ++i, ++f) deliver_frame(v, cap, f, good(q, i), f, n_out, out6, out_conf);
}

// What a bank call's frames_per_stream[S] and counts[F] come to, or the first reason to refuse them (err non-empty; capacity says
// which error code it is).  `name` is the tracker's, max_total (0 = none) a bound of the call's detections, checked before the arrays.
struct CallShape {
    long F = 0, total = 0;
    int kmax_s = 0, nmax = 0;       // most frames of one stream; most detections of one frame
    bool capacity = false;
    std::string err;
};
inline CallShape check_call(const char* name, int S, const int32_t* frames_per_stream, const int32_t* counts, bool have_arrays, long max_total = 0) {
    CallShape c;
    auto fail = [&](bool capacity, const std::string& m) { c.capacity = capacity, c.err = m; return c; };
    for (int q = 0; q < S; ++q) {
        if (frames_per_stream[q] < 0) return fail(false, "negative frame count / row capacity");
        c.F += frames_per_stream[q], c.kmax_s = std::max(c.kmax_s, (int)frames_per_stream[q]);
    }
    if (c.F > (1 << 24)) return fail(false, "too many frames in one call");
    for (long f = 0; f < c.F; ++f) {
        if (counts[f] < 0) return fail(false, "negative detection count");
        if (counts[f] > TRK_DEV_NMAX) return fail(true, std::string(name) + ": more than 512 detections in one frame");
        c.total += counts[f], c.nmax = std::max(c.nmax, (int)counts[f]);
    }
    if (max_total && c.total >= max_total) return fail(false, "too many detections in one call");
    if (c.total && !have_arrays) return fail(false, "NULL detection arrays");
    return c;
}

// ---- a call's whole layout behind the caller's prefix (c): detections | warps[F*6] | feat || outputs | tail, the three optional fields
// 16-byte aligned, and, device only, feat_n (as large as feat) at o_featn behind the mirrored bytes
struct CallStage {
    DetBlock det;
    bool has_warps, has_feat;
    size_t feat_bytes, o_warp, o_feat;
    OutBlock out;
    size_t o_tail, bytes, o_featn;
    CallStage(StageCursor c, size_t F, size_t n, int cap_rows, bool valid, bool warps, bool feat, size_t feat_bytes_, bool tail, size_t tail_bytes)
        : det(c, F, n, valid), has_warps(warps), has_feat(feat), feat_bytes(feat_bytes_), o_warp(warps ? c.take(F * 24, true) : 0),
          o_feat(feat ? c.take(feat_bytes, true) : 0), out(c, F, cap_rows), o_tail(tail ? c.take(tail_bytes, true) : 0), bytes(c.at),
          o_featn(up16(bytes)) {}
};
// Tracker::update_device / update_batch: no prefix; dbg_stride ints of debug pairs per frame as the tail (update_batch only)
inline CallStage tracker_stage(size_t k, size_t n, int cap_rows, int dbg_stride) {
    return CallStage(StageCursor{}, k, n, cap_rows, true, false, false, 0, dbg_stride > 0, k * dbg_stride * 4);
}
// EpochBank::update: stream_f0[S] | stream_k[S] in front; valid, warps and feat (rows of dim floats) when a BankExtra gives them
inline CallStage bank_stage(int S, size_t F, size_t n, int cap_rows, bool valid, bool warps, bool feat, int dim) {
    return CallStage(StageCursor{(size_t)S * 8}, F, n, cap_rows, valid, warps, feat && n, feat && n ? n * (size_t)dim * 4 : 0, false, 0);
}
// DeepSortBank: plan[E*S] | row_map[n] | frame_e0[F] | stream_f0[S] | stream_k[S], alone in run_group()'s buffer and update()'s prefix
struct DeepSortPlanBlock {
    size_t o_map, o_e0, o_f0, o_k;
    DeepSortPlanBlock(StageCursor& c, size_t E, int S, size_t F, size_t n) {
        c.take(E * S * sizeof(EpochStreamPlan));                  // the plans, at the buffer's start
        o_map = c.take(n * 4), o_e0 = c.take(F * 4), o_f0 = c.take((size_t)S * 4, true), o_k = c.take((size_t)S * 4);
    }
};
// DeepSortBank::update: behind its plan block (c); valid and feat always placed; the S table headers as the tail
inline CallStage deepsort_stage(StageCursor c, int S, size_t F, size_t n, int cap_rows, bool feats, int dim) {
    return CallStage(c, F, n, cap_rows, true, false, true, feats ? n * (size_t)dim * 4 : 0, true, (size_t)S * sizeof(DevTrkHdr));
}

}  // namespace aic
