// Instantiations of the persistent sample kernel for ONE streams-per-workgroup value (compile with -DLPCN_S=1|2|4):
// items per lane (register-resident GRU-A variants) x blob flavour (fp32 / int8) x arithmetic (PARITY / FAST).
// Units of their own beside the engine's so that the three values build in parallel.
#include "sample_kernel.hip.h"
#include "sample_launch.hip.h"
#include "sample_variants.h"

#ifndef LPCN_S
#error "compile with -DLPCN_S=1, 2 or 4"
#endif
#define LPCN_CAT2(a, b) a##b
#define LPCN_CAT(a, b) LPCN_CAT2(a, b)

template <int NW, bool I8, bool FAST, bool PACK2 = false>
static int launch(int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    return lpcn_launch_sample_kernel<lpcn::sample_kernel<LPCN_S, NW, I8, FAST, PACK2>>(grid, lds, st, d_args);
}

template <bool FAST>
static int pick(int nw, int is_int8, int pack2, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
#ifdef LPCN_ONLY_BENCH_VARIANT       // tools: compile only the benchmark model's PARITY float kernel (quick assembly listings)
    if constexpr (FAST) return LPCN_NO_SUCH_VARIANT;
#if LPCN_ONLY_BENCH_VARIANT == 2     // ... the int8 one (32 items per lane, two workgroups per CU; build with -DLPCN_S=2)
    else return (is_int8 && nw == 32 && pack2) ? launch<32, true, false, (LPCN_S <= 2)>(grid, lds, st, d_args) : LPCN_NO_SUCH_VARIANT;
#else
    else return (!is_int8 && nw == 30) ? launch<30, false, false>(grid, lds, st, d_args) : LPCN_NO_SUCH_VARIANT;
#endif
#else
    // one case per compiled items-per-lane variant (sample_variants.h); int8 at 32 items and S <= 2 also has the two-workgroups-per-CU form
#define LPCN_CASE_I8(n) case n: return (pack2 && n == 32 && LPCN_S <= 2) ? launch<n, true, FAST, (n == 32 && LPCN_S <= 2)>(grid, lds, st, d_args) : launch<n, true, FAST>(grid, lds, st, d_args);
#define LPCN_CASE_F32(n) case n: return launch<n, false, FAST>(grid, lds, st, d_args);
    if (is_int8) {
        switch (nw) {
        LPCN_VARIANTS_I8(LPCN_CASE_I8)
        default: return LPCN_NO_SUCH_VARIANT;
        }
    }
    switch (nw) {
    LPCN_VARIANTS_F32(LPCN_CASE_F32)
    default: return LPCN_NO_SUCH_VARIANT;
    }
#undef LPCN_CASE_I8
#undef LPCN_CASE_F32
#endif
}

// returns a hipError_t value (0 = launched) or LPCN_NO_SUCH_VARIANT
// flags: bit 0 = FAST arithmetic, bit 1 = PACK2 (two workgroups per CU; int8, 32 items per lane only)
extern "C" int LPCN_CAT(lpcn_launch_sample_s, LPCN_S)(int nw, int is_int8, int flags, int grid, int lds, hipStream_t st, const LpcnSampleArgs *d_args)
{
    const int pack2 = (flags >> 1) & 1;
    return (flags & 1) ? pick<true>(nw, is_int8, pack2, grid, lds, st, d_args) : pick<false>(nw, is_int8, pack2, grid, lds, st, d_args);
}
