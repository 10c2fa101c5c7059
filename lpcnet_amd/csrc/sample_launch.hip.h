// Launch of one sample-kernel instantiation K (sample_variants.hip, sample_x2.hip, sample_x3.hip) with THREADS lanes per workgroup: raise its dynamic-LDS limit, then launch.
#pragma once
#include <hip/hip_runtime.h>
#include "sample_kernel.hip.h"          // LpcnSampleArgs, LPCN_WG_THREADS
#include <mutex>

// returns a hipError_t value (0 = launched)
template <void (*K)(const LpcnSampleArgs *), int THREADS = LPCN_WG_THREADS>
static int lpcn_launch_sample_kernel(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    // the dynamic-LDS limit of a variant is raised once per (device, size), not at every launch
    static std::mutex mu;
    static int limit[64];                                    // per HIP device: the size already granted
    int dev = 0;
    (void)hipGetDevice(&dev);
    {
        std::lock_guard<std::mutex> g(mu);
        if (dev < 0 || dev >= 64 || limit[dev] < lds) {
            hipError_t e = hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) return (int)e;
            if (dev >= 0 && dev < 64) limit[dev] = lds;
        }
    }
    // (the arguments stay a device-resident block read through scalar loads: passing the struct by value was measured --
    // 23 more spilled SGPRs, 105.6 vs 107.3 M samples/s on the float kernel, +1.7 % on the int8 one)
    hipLaunchKernelGGL(K, dim3(grid), dim3(THREADS), lds, st, d_args);
    return (int)hipGetLastError();
}
