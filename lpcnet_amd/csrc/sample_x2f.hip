// Instantiations of the two-group sample kernel (sample_kernel_x2.hip.h) with FAST fp32 arithmetic (a batch's opt-in, lpcnet_batch_set_fast_two_group):
// one per register-resident items-per-lane variant; the streamed variants and the twelve-wave form have none.  A translation unit of its own so
// that it builds beside the others.
#include "sample_kernel_x2.hip.h"
#include "sample_launch.hip.h"
#include "sample_variants.h"

template <int NW>
static int launch_x2f(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    return lpcn_launch_sample_kernel<lpcn::sample_kernel_x2<NW, true>>(grid, lds, st, d_args);
}

// returns a hipError_t value (0 = launched) or LPCN_NO_SUCH_VARIANT, which fails the caller's launch like any HIP error (engine_synth.hip: launch_sample)
extern "C" int lpcn_launch_sample_x2f(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    switch (nw) {
#define LPCN_CASE_X2F(n) case n: return launch_x2f<n>(grid, lds, st, d_args);
#ifdef LPCN_ONLY_BENCH_VARIANT
    LPCN_CASE_X2F(30)
#else
    LPCN_VARIANTS_X2(LPCN_CASE_X2F)
#endif
#undef LPCN_CASE_X2F
    default: return LPCN_NO_SUCH_VARIANT;
    }
}
