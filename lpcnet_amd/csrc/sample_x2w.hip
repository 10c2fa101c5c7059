// Instantiations of the two-group sample kernel (sample_kernel_x2.hip.h) for models of more than 32 items per lane: the variants that keep 24
// items of a lane in registers and stream the others from L2.  A translation unit of its own: it builds beside sample_x2.hip, whose kernels
// it leaves as they are.
#include "sample_kernel_x2.hip.h"
#include "sample_launch.hip.h"
#include "sample_variants.h"

template <int NW>
static int launch_x2w(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    return lpcn_launch_sample_kernel<lpcn::sample_kernel_x2<NW>>(grid, lds, st, d_args);
}

// returns a hipError_t value (0 = launched) or LPCN_NO_SUCH_VARIANT, which fails the caller's launch like any HIP error (engine_synth.hip: launch_sample)
extern "C" int lpcn_launch_sample_x2w(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    switch (nw) {
#define LPCN_CASE_X2W(n) case n: return launch_x2w<n>(grid, lds, st, d_args);
#ifndef LPCN_ONLY_BENCH_VARIANT          // (tools' quick builds: the benchmark model needs none of these)
    LPCN_VARIANTS_X2W(LPCN_CASE_X2W)
#endif
#undef LPCN_CASE_X2W
    default: return LPCN_NO_SUCH_VARIANT;
    }
}
