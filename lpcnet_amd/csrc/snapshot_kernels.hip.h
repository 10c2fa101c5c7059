// Stream snapshots on the device (engine_snapshot.hip: lpcn_batch_dev_snapshot / _restore): the records of m listed streams to or from one
// contiguous buffer in ONE launch.  The table walk is stream_copy_kernel's (roster_kernels.hip.h) with an outside end: row r of the by-value table
// is one section of the record (snapshot_plan.h) -- the array `bytes` per stream at base + stream * bytes on the batch's side, `off` bytes into
// record i at records + i * record_bytes on the other.  Sections start on 16-byte boundaries of a 16-byte aligned buffer, so the record side never
// narrows a row: `vec` is the widest vector the ARRAY side allows, chosen on the host as for the stream copies (16 where base and size allow, 8 for
// the 3 592-byte state record and the 72-byte VQ memories, 4 for the 3 924-byte analysis record and the PLC's `delta`).
// The two host halves (the PLC's control ints, the kept products' flag) are rows without an array: the gather copies them from the meta ints that
// were uploaded behind the list, the scatter skips them (the host consumes them when the call is made).  A row whose section the snapshot lacks
// (off == SNAP_FRESH) gives the stream a fresh record: zeros.  The gather also zeroes the bytes between a section's end and the next boundary, so
// equal states give equal records.  Plain copies: no LDS, no scratch.
// The list is validated on the host: every index inside the batch and all distinct, so the workgroups of a launch never touch each other's rows.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "snapshot_plan.h"

namespace lpcn {

constexpr int SNAP_THREADS = 256;
constexpr int SNAP_MAX_ROWS = LPCN_SNAP_MAX_SECTIONS;      // (the stream copies' ROSTER_MAX_ROWS arrays and the two host halves)
constexpr unsigned SNAP_FRESH = 0xffffffffu;
struct SnapRow {
    char *base;            // the array; nullptr: a host half
    unsigned bytes;        // per stream
    unsigned off;          // of the section in the record (SNAP_FRESH: the snapshot has no such section)
    unsigned vec;          // 16, 8 or 4: bytes per element moved (divides `bytes`); a host half: its first int in the stream's meta row
};
struct SnapTable {
    int rows, m;
    unsigned record_bytes;
    unsigned meta_ints;    // ints of a stream's meta row, at list + m
    SnapRow row[SNAP_MAX_ROWS];
};

template <typename V>
__device__ inline void snap_copy(V *dst, const V *src, unsigned bytes, int t)
{
    const int count = (int)(bytes / sizeof(V));
    for (int k = t; k < count; k += SNAP_THREADS) dst[k] = src[k];
}
template <typename V>
__device__ inline void snap_zero(V *dst, unsigned bytes, int t)
{
    const int count = (int)(bytes / sizeof(V));
    for (int k = t; k < count; k += SNAP_THREADS) dst[k] = V{};
}

// One workgroup per listed stream: list[i] is the stream of record i; the meta rows [m][meta_ints] follow the list.
__global__ __launch_bounds__(SNAP_THREADS) void stream_gather_kernel(SnapTable T, const int *list, char *records)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= T.m) return;
    const size_t s = (size_t)list[i];
    char *rec = records + (size_t)i * T.record_bytes;
    for (int r = 0; r < T.rows; ++r) {
        const SnapRow R = T.row[r];        // (the table lives in the kernel's argument segment: indexed scalar loads, nothing copied to scratch)
        char *dst = rec + R.off;
        if (!R.base) snap_copy<int>((int *)dst, list + T.m + (size_t)i * T.meta_ints + R.vec, R.bytes, t);
        else if (R.vec == 16) snap_copy<int4>((int4 *)dst, (const int4 *)(R.base + s * R.bytes), R.bytes, t);
        else if (R.vec == 8) snap_copy<int2>((int2 *)dst, (const int2 *)(R.base + s * R.bytes), R.bytes, t);
        else snap_copy<int>((int *)dst, (const int *)(R.base + s * R.bytes), R.bytes, t);
        const int pad = (int)((16u - R.bytes % 16u) % 16u) / 4;      // (every size is a whole number of ints)
        if (t < pad) ((int *)(dst + R.bytes))[t] = 0;
    }
}

// record i -> stream list[i]
__global__ __launch_bounds__(SNAP_THREADS) void stream_scatter_kernel(SnapTable T, const int *list, const char *records)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (i >= T.m) return;
    const size_t d = (size_t)list[i];
    const char *rec = records + (size_t)i * T.record_bytes;
    for (int r = 0; r < T.rows; ++r) {
        const SnapRow R = T.row[r];
        if (!R.base) continue;
        char *dst = R.base + d * R.bytes;
        if (R.off == SNAP_FRESH) {
            if (R.vec == 16) snap_zero<int4>((int4 *)dst, R.bytes, t);
            else if (R.vec == 8) snap_zero<int2>((int2 *)dst, R.bytes, t);
            else snap_zero<int>((int *)dst, R.bytes, t);
        } else if (R.vec == 16) snap_copy<int4>((int4 *)dst, (const int4 *)(rec + R.off), R.bytes, t);
        else if (R.vec == 8) snap_copy<int2>((int2 *)dst, (const int2 *)(rec + R.off), R.bytes, t);
        else snap_copy<int>((int *)dst, (const int *)(rec + R.off), R.bytes, t);
    }
}

}  // namespace lpcn
