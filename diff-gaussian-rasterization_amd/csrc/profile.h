// profile.h -- optional per-stage timing with HIP events on the launching stream (dgr_profile_* in dgr_hip.h; profile.hip).
// Disabled by default; when a stage is selected, two events bracket that stage's launch only.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "kernels.h"

namespace dgr {

// The stages, in the order dgr_profile_stage_name() lists them: id (ST_id) and name.
#define DGR_STAGES(X)                                                                                                          \
    X(ZERO_FWD, "zero_counters") X(PRE_FWD, "preprocess_fwd") X(SCAN_BLOCKS, "scan_blocks") X(BIN_SEGMENTS, "bin_segments")    \
    X(BIN_TILES, "bin_tiles") X(COUNT_RANK, "count_rank") X(SCAN, "scan_tiles") X(EMIT, "emit_instances") X(SORT, "sort_tiles") \
    X(TILE_SCHED, "tile_schedule") X(RENDER_FWD, "render_fwd") X(ZERO, "zero_scratch") X(RENDER_BWD, "render_bwd")             \
    X(PRE_BWD, "preprocess_bwd")
#define DGR_STAGE_ID(id, name) ST_##id,
enum Stage { DGR_STAGES(DGR_STAGE_ID) ST_COUNT };
#undef DGR_STAGE_ID

struct StageProf {
    const char* name;
    bool on = false;
    unsigned seen = 0;  // launches of this stage since it was selected
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
};
extern StageProf g_prof[ST_COUNT];

// A kernel stage hands its two events to the stage's first kernel launch (dgr::launch, kernels.h): they then hold
// that kernel's start and end.  A stage without a kernel (the scratch memset) is bracketed with hipEventRecord.
struct ScopedStage {
    StageProf* p = nullptr;
    hipStream_t st;
    LaunchEvents le{};
    bool kernel_stage;
    ScopedStage(int id, hipStream_t s, bool is_kernel = true) : st(s), kernel_stage(is_kernel) {
        if (g_prof[id].on) begin(id);
    }
    ~ScopedStage() {
        if (p) end();
    }
    ScopedStage(const ScopedStage&) = delete;
    ScopedStage& operator=(const ScopedStage&) = delete;

private:
    void begin(int id);
    void end();
};

}  // namespace dgr
