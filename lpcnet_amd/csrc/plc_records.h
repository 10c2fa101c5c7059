// What the PLC planner (plc_plan.cpp, host) writes and the PLC kernels (plc_kernels.hip.h) read: record sizes, flags and operation codes of a
// step's control lists.  Plain C++, no device code.
#pragma once

namespace lpcn {

constexpr int PLC_PRED_REC = 6;      // ints per record of plc_pred_kernel: stream, flags, FEC row, two float offsets, unused
constexpr int PLC_MIX_REC = 3;       // ints per record of plc_mix_kernel: stream, a, b
constexpr int PLC_FEED_REC = 8;      // ints per record of plc_fec_feed_kernel: stream, first source row, rows a, their ring row, move-from row, rows moved, rows b, their ring row

enum { PLC_F_ROT = 1, PLC_F_RESTORE_SHIFT = 1, PLC_F_INPUT_SHIFT = 3, PLC_F_COMPUTE = 32, PLC_F_KEEP = 64, PLC_F_ATT = 128, PLC_F_RAW = 256 };
enum { PLC_IN_ZEROS = 0, PLC_IN_FEC = 1, PLC_IN_BURG = 2, PLC_IN_BURG_FEAT = 3 };
enum { PLC_MIX_QTAIL, PLC_MIX_QAPPEND, PLC_MIX_QPUSH, PLC_MIX_QSHIFT, PLC_MIX_FAPPEND, PLC_MIX_RESETSIG, PLC_MIX_DCRECV, PLC_MIX_DCLOST, PLC_MIX_XFADE };

}  // namespace lpcn
