// What the PLC planner (plc_plan.cpp, host) writes and the PLC kernels (plc_kernels.hip.h) read: record sizes, flags and operation codes of a
// step's control lists.  Plain C++, no device code.
#pragma once

namespace lpcn {

constexpr int PLC_PRED_REC = 6;      // ints per record of plc_pred_kernel: stream, flags, FEC row, two float offsets, unused
constexpr int PLC_MIX_REC = 3;       // ints per record of plc_mix_kernel: stream, a, b
constexpr int PLC_FEED_REC = 8;      // ints per record of plc_fec_feed_kernel: stream, first source row, rows a, their ring row, move-from row, rows moved, rows b, their ring row

enum { PLC_F_ROT = 1, PLC_F_RESTORE_SHIFT = 1, PLC_F_INPUT_SHIFT = 3, PLC_F_COMPUTE = 32, PLC_F_KEEP = 64, PLC_F_ATT = 128, PLC_F_RAW = 256 };
enum { PLC_IN_ZEROS = 0, PLC_IN_FEC = 1, PLC_IN_BURG = 2, PLC_IN_BURG_FEAT = 3 };
// The dynamic LDS of the predictor's forms with S > 1 streams per workgroup (plc_pred_s_kernel<S>), in dwords per STREAM: every array lies [j][S].
// The 57 inputs (rounded up to 60), dense1's output, both GRU states, the GRUs' two scratch arrays over the wider GRU, the 20 outputs; an int8 blob's
// GRUs add their quantised input and old state, four int8 per dword; then the stream's control record and its live flag.  The S = 1 kernels have
// static LDS only.
constexpr int PLC_PRED_IN_PAD = 60;
constexpr int PLC_PRED_FORM_LDS_LIMIT = 160 * 1024;
constexpr int plc_pred_max(int a, int b) { return a > b ? a : b; }
constexpr int plc_pred_lds_floats(int d1, int g1, int g2) { return PLC_PRED_IN_PAD + d1 + g1 + g2 + 6 * plc_pred_max(g1, g2) + 20; }
constexpr int plc_pred_lds_quants(int d1, int g1, int g2, int int8) { return int8 ? (plc_pred_max(d1, g1) + plc_pred_max(g1, g2)) / 4 : 0; }
constexpr int plc_pred_lds_bytes(int S, int d1, int g1, int g2, int int8)
{
    return S > 1 ? S * 4 * (plc_pred_lds_floats(d1, g1, g2) + plc_pred_lds_quants(d1, g1, g2, int8) + PLC_PRED_REC + 1) : 0;
}

enum { PLC_MIX_QTAIL, PLC_MIX_QAPPEND, PLC_MIX_QPUSH, PLC_MIX_QSHIFT, PLC_MIX_FAPPEND, PLC_MIX_RESETSIG, PLC_MIX_DCRECV, PLC_MIX_DCLOST, PLC_MIX_XFADE };

}  // namespace lpcn
