// Device-side stream copies (engine_roster.hip: lpcn_batch_dev_copy_streams): everything a batch keeps per stream moves from stream src[i] to
// stream dst[i] in ONE launch.  Every per-stream array of the batch is `bytes` bytes per stream at base + stream * bytes; the host lists the
// arrays that are allocated now in a small table passed by value -- at most ROSTER_MAX_ROWS entries -- with the widest vector each row may move
// in: 16 bytes where the row size allows (the bases come from hipMalloc), 8 for the 3 592-byte state record and the 72-byte VQ memories (as
// group_gather_kernel moves states), 4 for the 3 924-byte analysis record and the PLC's `delta`.  Plain copies: no LDS, no scratch.
// The pair list is validated on the host (api_roster.h: roster_check): every index lies inside the batch, the destinations are distinct and no
// stream is both a source and a destination, so the workgroups of a launch never touch each other's rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace lpcn {

constexpr int ROSTER_THREADS = 256;
constexpr int ROSTER_MAX_ROWS = 24;
struct RosterRow {
    char *base;            // the array
    unsigned bytes;        // per stream
    unsigned vec;          // 16, 8 or 4: bytes per element moved (divides `bytes`)
};
struct RosterTable {
    int rows, pairs;
    RosterRow row[ROSTER_MAX_ROWS];
};

template <typename V>
__device__ inline void roster_copy(char *base, unsigned bytes, size_t s, size_t d, int t)
{
    const V *src = (const V *)(base + s * bytes);
    V *dst = (V *)(base + d * bytes);
    const int count = (int)(bytes / sizeof(V));
    for (int k = t; k < count; k += ROSTER_THREADS) dst[k] = src[k];
}

// One workgroup per pair; pairs [m][2] = {src, dst}.
__global__ __launch_bounds__(ROSTER_THREADS) void stream_copy_kernel(RosterTable T, const int *pairs)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= T.pairs) return;
    const size_t s = (size_t)pairs[2 * i], d = (size_t)pairs[2 * i + 1];
    for (int r = 0; r < T.rows; ++r) {
        const RosterRow R = T.row[r];      // (the table lives in the kernel's argument segment: indexed scalar loads, nothing copied to scratch)
        if (R.vec == 16) roster_copy<int4>(R.base, R.bytes, s, d, t);
        else if (R.vec == 8) roster_copy<int2>(R.base, R.bytes, s, d, t);
        else roster_copy<int>(R.base, R.bytes, s, d, t);
    }
}

}  // namespace lpcn
