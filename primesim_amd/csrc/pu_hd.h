// pu_hd.h — PU_HD marks what the host and the kernels share (stream_step.h,
// delay_sum_step.h): __host__ __device__ under hipcc's HIP mode, nothing in plain C++.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PU_HD __host__ __device__
#else
#define PU_HD
#endif
