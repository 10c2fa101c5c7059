// The twelve-wave form of the two-group sample kernel (sample_kernel_x3.hip.h): eight float streams per workgroup on three waves per SIMD, PARITY
// arithmetic, 16 register-resident items per lane.  A translation unit of its own so that it builds beside the others.
#include "sample_kernel_x3.hip.h"
#include "sample_launch.hip.h"

// dynamic LDS of a launch: the two-group layout plus this form's own cells (LdsX3: the streams' sequence words, 32 B)
extern "C" int lpcn_x3_lds_bytes(int nb_b) { return lpcn::LdsX3::total(nb_b); }

// returns a hipError_t value (0 = launched)
extern "C" int lpcn_launch_sample_x3(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    return lpcn_launch_sample_kernel<lpcn::sample_kernel_x3, LPCN_X3_THREADS>(grid, lds, st, d_args);
}
