// TEST INFRASTRUCTURE: host build of the two leader-lane functions of lpcnet_amd/csrc/lpcnet_math.h that the loud census
// (tests/tools/loud_census.py) can put in place of the oracle's: the float-to-mu-law conversion and the PCM rounding.
//   g++ -O2 -ffp-contract=off -shared -fPIC -I lpcnet_amd/csrc tests/tools/loud_math_host.cpp -o <tmp>/libloud_math_host.so
#include "lpcnet_math.h"

extern "C" {
int loud_lin2ulaw(float x) { return lpcn_lin2ulaw(x); }
// the kernels store (short)lpcn_round_pcm(pcm) (sample_common.hip.h, finish_sample): the census applies the same narrowing
int loud_round_pcm(float pcm) { return lpcn_round_pcm(pcm); }
}
