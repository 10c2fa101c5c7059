/* How a call of the feature analysis or of the encoder is cut into launches: the chunk of a call and the (stream, packet) items a wavefront of
 * the VQ kernels takes.  Plain C, no device code: engine_codec.hip and encode_kernels.hip.h launch by these rules, and api_tools.c reports them
 * (lpcnet_hip_encode_plan) so that a test can tell which form of a kernel a shape runs. */
#pragma once
#include <stddef.h>

/* (stream, frame) items per launch of the analysis kernels: bounds their scratch (2.7 KB per item) at 176 MB */
#define LPCN_AN_ITEMS_MAX 65536
#define LPCN_ENC_VQ_WAVES 8      /* wavefronts of a VQ workgroup, one (stream, packet) item each per slot */
#define LPCN_ENC_END_IPW 4       /* items per wavefront, at most: encode_vq_end_kernel (77 KB of LDS: two workgroups per CU) */
#define LPCN_ENC_MID_IPW 2       /*   ... encode_vq_mid_kernel (78 KB) */

/* frames per launch of a call of n_frames frames on a batch of capacity n (at least one frame, whatever the batch size) */
static inline int lpcn_analysis_chunk(int n, int n_frames)
{
    int cap = LPCN_AN_ITEMS_MAX / n;
    if (cap < 1) cap = 1;
    return n_frames < cap ? n_frames : cap;
}

/* packets per launch: a whole number of packets (four frames each) within the same bound, at least one */
static inline int lpcn_encode_chunk(int n, int n_packets)
{
    int cap = LPCN_AN_ITEMS_MAX / n / 4;
    if (cap < 1) cap = 1;
    return n_packets < cap ? n_packets : cap;
}

/* items per wavefront of a VQ kernel: enough workgroups for two per CU before a workgroup takes more items per staged codebook */
static inline int lpcn_encode_ipw(size_t items, int ipw_max)
{
    const size_t want = items / ((size_t)LPCN_ENC_VQ_WAVES * 512);
    return want < 1 ? 1 : (want > (size_t)ipw_max ? ipw_max : (int)want);
}
