// threadIdx / blockIdx / blockDim / gridDim come with <hip/hip_runtime.h>
#pragma once
#include "cuda_runtime.h"
