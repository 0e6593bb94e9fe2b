// bytetrack_host.hpp -- the ByteTrack tracker object (bytetrack.cpp): a bank of streams (epoch_bank.hpp) over the device tables of
// bytetrack.hpp.  Used by the C ABI (aic_bytetrack_*: a bank of one; aic_bytetrack_bank_*) and by the pipeline (aic_pipeline_create_bytetrack).
#pragma once
#include "bytetrack.hpp"
#include "common.hpp"
#include "epoch_bank.hpp"

namespace aic {

BtParams bytetrack_params(const aic_bytetrack_params& p, int* first_id);

// ---- what the two trackers of the BYTE life cycle (ByteTracker here, BotSortTracker in botsort_host.hpp) report alike
std::string byte_err_text(int err);                               // the error codes of byte_epoch.hpp

struct ByteExport {                 // the columns of aic_bytetrack_export, caller's memory, any may be NULL
    int32_t *id, *state, *act, *start, *end, *cls;
    float *score, *mean, *cov;
};
// The live tracks of a table fetched to the host, tracked list then lost list, into at most cap_rows rows of e; extra(row, slot) adds the
// caller's own columns.  Returns their number.
template <class Table, class F>
int byte_export(const Table& t, int cap_rows, const ByteExport& e, int32_t* n_tracked, F extra) {
    const int ntl = t.hdr->n_tracked, nll = t.hdr->n_lost, n = ntl + nll;
    if (n_tracked) *n_tracked = ntl;
    for (int i = 0; i < n && i < cap_rows; ++i) {
        const int sl = i < ntl ? t.tl[i] : t.ll[i - ntl];
        const BtTrack& r = t.trk[sl];
        if (e.id) e.id[i] = r.id;
        if (e.state) e.state[i] = r.state;
        if (e.act) e.act[i] = r.act;
        if (e.start) e.start[i] = r.start;
        if (e.end) e.end[i] = r.end;
        if (e.cls) e.cls[i] = r.cls;
        if (e.score) e.score[i] = r.score;
        if (e.mean) std::copy(t.mean + (size_t)sl * 8, t.mean + (size_t)sl * 8 + 8, e.mean + (size_t)i * 8);
        if (e.cov) std::copy(t.cov + (size_t)sl * 64, t.cov + (size_t)sl * 64 + 64, e.cov + (size_t)i * 64);
        extra(i, sl);
    }
    return n;
}

struct ByteTracker : EpochBank<BtHdr, BtParams> {
    ByteTracker(Device& d, const BtParams& p, int first_id, int streams = 1);
    const char* name() const override { return "ByteTrack"; }
    void launch(const BtParams& p, const EpochCall& c, hipStream_t s) override;
    std::string err_text(int err) const override { return byte_err_text(err); }
    // the single tracker's call: k consecutive frames of stream 0 of a bank of one
    void update_batch(int k, const int32_t* counts, const float* xyxy, const float* conf, const int32_t* cls, int cap_rows,
                      int32_t* n_out, int32_t* out6, float* out_conf);
    void counters(int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side);
    int export_state(int stream, int cap_rows, const ByteExport& e, int32_t* n_tracked);
};

}  // namespace aic

struct aic_bytetrack {
    aic::ByteTracker t;
    aic_bytetrack(aic::Device& d, const aic::BtParams& p, int first_id) : t(d, p, first_id) {}
};
struct aic_bytetrack_bank {
    aic::ByteTracker t;
    aic_bytetrack_bank(aic::Device& d, const aic::BtParams& p, int first_id, int streams) : t(d, p, first_id, streams) {}
};
