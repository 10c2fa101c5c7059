"""TEST TOOLING shared by the end-to-end PLC tests (tests/test_gpu_plc.py, test_gpu_plc_i8.py, test_gpu_plc_forms.py): the frame loop that drives
a batch with the fixture's PCM, loss flags and FEC schedule."""
import numpy as np


def run(b, pcm, lost, t0=0, t1=None, ops=None, vec=None, streams=None):
    """steps frames [t0, t1) of the given streams' inputs (default: stream i of the batch = stream i of the fixture) -> [n][t1 - t0][160]"""
    streams = list(range(b.n)) if streams is None else streams
    t1 = pcm.shape[1] if t1 is None else t1
    out = np.zeros((b.n, t1 - t0, 160), np.int16)
    for t in range(t0, t1):
        if ops is not None:
            for i, s in enumerate(streams):
                op = int(ops[t, s])
                if op in (1, 4):
                    for k in range(2 if op == 4 else 1):
                        b.plc_fec_add(i, vec[t, s, k])
                elif op == 2:
                    b.plc_fec_add(i, None)
                elif op == 3:
                    b.plc_fec_clear(i)
        lo = np.ascontiguousarray(lost[streams, t])
        frame = np.ascontiguousarray(pcm[streams, t])
        frame[lo != 0] = 0
        out[:, t - t0] = b.plc_step(frame, lo)
    return out
