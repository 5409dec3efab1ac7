// host_util.h -- what every host unit of the library needs: the thread's last error, HIP_TRY, aligned16.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/dgr_hip.h"

namespace dgr {

// The text behind dgr_last_error(), one per thread (defined in api.hip).
void set_last_error(const std::string& text);

inline int hip_fail(hipError_t e, const char* what) {
    set_last_error(std::string(what) + ": " + hipGetErrorString(e));
    return DGR_ERR_HIP;
}
#define HIP_TRY(expr)                                        \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return dgr::hip_fail(_e, #expr); \
    } while (0)

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace dgr
