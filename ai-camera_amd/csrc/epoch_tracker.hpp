// epoch_tracker.hpp -- an epoch tracker as the pipeline's stage B sees it (pipeline.cpp): the group's frames go through its epoch
// launches on the tracker stream, the error check follows the caller's sync.  ByteTracker (bytetrack_host.hpp), OcSortTracker
// (ocsort_host.hpp) and BotSortTracker (botsort_host.hpp) are banks of streams (epoch_bank.hpp: one kernel block per stream); a
// BoT-SORT pipeline fixes its stream count at creation (aic_pipeline_create_botsort_bank), the other two take the option "streams".
#pragma once
#include <string>

#include "common.hpp"
#include "trk_dev.hpp"

namespace aic {

struct EpochTracker {
    bool failed = false;            // a capacity error stops the tracker: its table is no longer a frame boundary
    std::string fail_msg;
    virtual ~EpochTracker() = default;
    virtual const char* name() const = 0;
    // frames [0, frames) of `dets` as epochs on stream s; the header copy lands behind them (check_epochs() after the caller's sync)
    virtual void run_epochs(const EpochDets& dets, int frames, const EpochOut& out, hipStream_t s) = 0;
    virtual void check_epochs() = 0;
    // banks only: `streams` camera streams, the group's frames tick-major (frame t * streams + s = tick t of stream s)
    virtual int streams() const { return 1; }
    virtual void set_streams(int) { AIC_REQUIRE(false, AIC_ERR_INVALID, std::string(name()) + " tracks one stream per pipeline"); }
    virtual void reset_stream(int) { AIC_REQUIRE(false, AIC_ERR_INVALID, std::string(name()) + " tracks one stream per pipeline"); }
};

}  // namespace aic
