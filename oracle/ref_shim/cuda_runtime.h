// Forwarding header: lets a CUDA translation unit that uses only the names below compile under hipcc.
// Part of the recipe that builds the reference rasterizer for gfx950 (oracle/build_ref.py); our own text.
#pragma once
#include <hip/hip_runtime.h>

#define cudaError_t hipError_t
#define cudaSuccess hipSuccess
#define cudaGetErrorString hipGetErrorString
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaMemcpy hipMemcpy
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemset hipMemset

// The only caller (in_frustum, `prefiltered` set and a point culled) is never reached: the wrapper refuses prefiltered = true.
// A no-op, so that no wave can trap on a shared machine.
#define __trap() ((void)0)
