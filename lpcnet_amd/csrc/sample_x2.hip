// Instantiations of the two-group sample kernel (sample_kernel_x2.hip.h): eight float streams per workgroup, PARITY arithmetic,
// one per register-resident items-per-lane variant.  A translation unit of its own so that it builds beside the others.
#include "sample_kernel_x2.hip.h"
#include "sample_launch.hip.h"
#include "sample_variants.h"

template <int NW>
static int launch_x2(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    return lpcn_launch_sample_kernel<lpcn::sample_kernel_x2<NW>>(grid, lds, st, d_args);
}

// returns a hipError_t value (0 = launched) or LPCN_NO_SUCH_VARIANT, which fails the caller's launch like any HIP error (engine_synth.hip: launch_sample)
extern "C" int lpcn_launch_sample_x2(int nw, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    switch (nw) {
#define LPCN_CASE_X2(n) case n: return launch_x2<n>(grid, lds, st, d_args);
#ifdef LPCN_ONLY_BENCH_VARIANT
    LPCN_CASE_X2(30)
#else
    LPCN_VARIANTS_X2(LPCN_CASE_X2)
#endif
#undef LPCN_CASE_X2
    default: return LPCN_NO_SUCH_VARIANT;
    }
}
extern "C" int lpcn_x2_lds_bytes(int nb_b) { return lpcn::LdsX2::total(nb_b); }
