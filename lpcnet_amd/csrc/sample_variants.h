// The compiled items-per-lane variants of the sample kernels, in rising order: the one place where they are listed.
// engine.hip rounds a model's item count up to the next value of a list; sample_variants.hip, sample_x2.hip and sample_x2w.hip
// instantiate one kernel per value.  (No HIP in here: plain preprocessor lists, X(n) applied to every value.)
#pragma once

// float blobs: an item is 4 VGPRs; more than 32 items per lane: the items past the 28th are streamed from L2 (sample_kernel.hip.h);
// 96 = a full row, every one of its 96 input blocks
#define LPCN_VARIANTS_F32(X) X(24) X(28) X(30) X(32) X(36) X(40) X(48) X(64) X(80) X(96)
// int8 blobs: an item is 1 VGPR; 96 = a row group may list every one of its 96 input blocks (trained, heavy-tailed sparsity)
#define LPCN_VARIANTS_I8(X) X(32) X(48) X(64) X(96)
// the two-group kernel (eight float streams per workgroup): register-resident items only
#define LPCN_VARIANTS_X2(X) X(24) X(28) X(30) X(32)
// ... its streamed variants (sample_x2w.hip; a batch's opt-in): 24 items resident, the others from L2; a wave runs to its own item count, so the
// padding of a model's count to the next value costs nothing at run time
#define LPCN_VARIANTS_X2W(X) X(48) X(64) X(80) X(96)
// what a launcher returns, in place of a hipError_t value, for an items-per-lane value it has no kernel for (no HIP call returns it)
#define LPCN_NO_SUCH_VARIANT (-1)
