// cooperative_groups::this_grid() / this_thread_block()
#pragma once
#include <hip/hip_cooperative_groups.h>
