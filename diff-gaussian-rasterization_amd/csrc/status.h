// status.h -- what the orchestration (api.hip) needs of the status machinery (status.hip): where a forward reports its status
// word, and what the reports of earlier forwards say about the next one.  The slot pool, the tag protocol and the quarantine rule
// stay inside status.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "dgr_common.h"

namespace dgr {

// dgr_early_status_arm: copies the (final) status word to the host behind the binning kernels; a no-op unless armed.
int early_status_post(const int* device_status, hipStream_t st);

// dgr_backward_scratch_clean_arm: whether this thread armed it since its last backward.  Consumed by the call.
bool take_scratch_clean_arm();

// The tile schedule by the frame (option "tile_schedule" = 2) and the longest tile list of this shape's last reported frame
// (-1 without one), from the reports of armed status slots.
bool want_schedule(int W, int H, int P);
int hinted_longest_list(int W, int H, int P);

// The armed slot of this thread (dgr_status_arm), taken by a presized forward.  If the call leaves before its binning kernel is
// enqueued (an error, P == 0) the word is completed from the host -- all zero -- so that a poll never waits for a write that will
// not come.  id < 0: nothing was armed.
struct ArmedReport {
    long id = -1;
    StatusReport rep{nullptr, 0u, nullptr};
    bool handed_over = false;  // the forward's blend kernel -- which delivers the word -- has been enqueued
    ArmedReport(int W, int H, int P, hipStream_t st = nullptr);
    ~ArmedReport();
    ArmedReport(const ArmedReport&) = delete;
    ArmedReport& operator=(const ArmedReport&) = delete;
};

}  // namespace dgr
