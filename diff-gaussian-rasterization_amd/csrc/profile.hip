// profile.hip -- the stage profiler behind dgr_profile_* (profile.h).
#include "profile.h"

#include <algorithm>
#include <mutex>
#include <string>

#include "options.h"

namespace dgr {

thread_local LaunchEvents* g_launch_events = nullptr;

#define DGR_STAGE_PROF(id, name) {name},
StageProf g_prof[ST_COUNT] = {DGR_STAGES(DGR_STAGE_PROF)};
#undef DGR_STAGE_PROF
namespace {
std::mutex g_prof_mu;
}

void ScopedStage::begin(int id) {
    // option "profile_every" = n: bracket every n-th launch only (the events ride in the dispatch packet
    // and cost a little overlap between streams; a sample keeps the timed region undisturbed)
    if (g_prof[id].seen++ % (unsigned)std::max(1, option(OPT_PROFILE_EVERY)) != 0) return;
    p = &g_prof[id];
    if (hipEventCreate(&le.start) != hipSuccess || hipEventCreate(&le.stop) != hipSuccess) { p = nullptr; return; }
    le.used = false;
    if (kernel_stage) g_launch_events = &le;
    else (void)hipEventRecord(le.start, st);
}
void ScopedStage::end() {
    if (kernel_stage) {
        g_launch_events = nullptr;
        if (!le.used) {  // nothing was launched (empty input)
            (void)hipEventDestroy(le.start);
            (void)hipEventDestroy(le.stop);
            return;
        }
    } else {
        (void)hipEventRecord(le.stop, st);
    }
    std::lock_guard<std::mutex> lk(g_prof_mu);
    p->ev.emplace_back(le.start, le.stop);
}

}  // namespace dgr

using namespace dgr;

extern "C" {

int dgr_profile_select(const char* stage) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    const std::string n(stage ? stage : "");
    bool found = n.empty() || n == "all";
    for (auto& p : g_prof) {
        p.seen = 0;
        p.on = (n == "all") || (n == p.name);
        found = found || p.on;
    }
    return found ? DGR_OK : DGR_ERR_BAD_ARGUMENT;
}
int dgr_profile_stage_count(void) { return ST_COUNT; }
const char* dgr_profile_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? g_prof[i].name : ""; }
int dgr_profile_read(const char* stage, double* total_ms, int* launches) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (auto& p : g_prof) {
        if (std::string(stage) != p.name) continue;
        double tot = 0;
        int n = 0;
        for (auto& e : p.ev) {
            float ms = 0;
            if (hipEventSynchronize(e.second) == hipSuccess && hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) {
                tot += ms;
                n++;
            }
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        p.ev.clear();
        *total_ms = tot;
        *launches = n;
        return DGR_OK;
    }
    return DGR_ERR_BAD_ARGUMENT;
}

}  // extern "C"
