"""TEST TOOLING shared by tests/tools/make_golden_plc_state.py, tests/test_plc_state_host.py and tests/test_gpu_plc_state.py: the replays the PLC
state fixture (tests/golden/golden_plc_state_v1.npz) is recorded over.  No new inputs: the seeded scripts of plc_model.py (loss_patterns at the
four option sets, fec_schedule with fec_loss_patterns) and of plc_fec_script.py, brought to one form of events per (frame, stream) -- clear, then
`skip` NULL adds, then the vectors, then the step with its loss flag -- and one function each that plays a frame's events to the reference
(oracle.ref.RefPlc) and to a stream of an engine batch."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plc_model as pm  # noqa: E402
import plc_fec_script as fs  # noqa: E402

# name -> (flavour of the blob and of the reference build, options, streams, frames, checkpoints: frames processed when the state is recorded)
CHECKPOINTS = (33, 85, 120)
REPLAYS = {
    "causal":    ("float", 0, pm.N_STREAMS, pm.T, CHECKPOINTS),
    "codec":     ("float", 2, pm.N_STREAMS, pm.T, CHECKPOINTS),
    "causal_dc": ("float", 4, pm.N_STREAMS, pm.T, CHECKPOINTS),
    "codec_dc":  ("float", 6, pm.N_STREAMS, pm.T, CHECKPOINTS),
    "fec":       ("float", 0, pm.FEC_STREAMS, pm.T, CHECKPOINTS),          # (the streams with schedules; the others repeat "causal")
    "script":    ("float", 2, fs.N, fs.T, (10, 33, 60)),
    "i8":        ("int8", 4, 16, 140, CHECKPOINTS),
}
CONT = 20          # frames of the reference's output a snapshot carries


class Events:
    """one replay's inputs: pcm [n][T][160], lost [n][T], clear / skip / count [T][n] and vectors(t, s) -> [count][20]"""

    def __init__(self, name):
        self.name = name
        self.flavour, self.options, self.n, self.T, self.checkpoints = REPLAYS[name]
        n, T = self.n, self.T
        self.clear = np.zeros((T, n), np.uint8)
        self.skip = np.zeros((T, n), np.int32)
        self.count = np.zeros((T, n), np.int32)
        self.op = None          # the plc_model form of the same traffic, where the replay has one (what lpcnet_hip_plc_plan takes as fec_op)
        if name == "script":
            sc = fs.script()
            self.pcm, self.lost = sc["pcm"], np.ascontiguousarray(sc["lost"].T)
            self.clear, self.skip, self.count = sc["clear"], sc["skip"], sc["count"]
            self._vec = sc["vec"]
            self._first = np.concatenate([[0], np.cumsum(self.count.reshape(-1))])          # (step 0's vectors first, within a step stream 0's first)
        else:
            self.pcm = np.stack([pm.stream_pcm(s) for s in range(n)])[:, :T]
            if name == "fec":
                self.lost = pm.fec_loss_patterns()[:n, :T]
                self.op, self._vec = (x[:, :n] for x in pm.fec_schedule())
                self.clear[:] = self.op == 3
                self.skip[:] = self.op == 2
                self.count[:] = np.where(self.op == 1, 1, np.where(self.op == 4, 2, 0))
            else:
                self.lost = pm.loss_patterns()[:n, :T]

    def vectors(self, t, s):
        k = int(self.count[t, s])
        if self.name == "script":
            first = int(self._first[t * self.n + s])
            return self._vec[first:first + k]
        return self._vec[t, s, :k] if k else np.zeros((0, 20), np.float32)

    def feed_ref(self, st, t, s):
        """the FEC calls of stream s in front of frame t, on an oracle.ref.RefPlc"""
        if self.clear[t, s]:
            st.fec_clear()
        for _ in range(int(self.skip[t, s])):
            st.fec_add(None)
        for v in self.vectors(t, s):
            st.fec_add(v)

    def feed_engine(self, b, slot, t, s):
        """the same calls on stream `slot` of an engine batch"""
        if self.clear[t, s]:
            b.plc_fec_clear(slot)
        for _ in range(int(self.skip[t, s])):
            b.plc_fec_add(slot, None)
        for v in self.vectors(t, s):
            b.plc_fec_add(slot, v)

    def has_fec(self):
        return bool(self.clear.any() or self.skip.any() or self.count.any())

    def frame(self, t, s):
        f = self.pcm[s, t].copy()
        if self.lost[s, t]:
            f[:] = 0
        return f


@functools.lru_cache(maxsize=None)
def events(name):
    """the replay's Events, built once per process (the tests only read them)"""
    return Events(name)


def run_engine(b, ev, t0, t1):
    """frames [t0, t1) of the whole replay on a batch of ev.n streams (stream i = stream i of the replay) -> [n][t1 - t0][160]; every frame's FEC
    traffic goes through one plc_fec_feed"""
    out = np.zeros((ev.n, t1 - t0, 160), np.int16)
    fec = ev.has_fec()
    for t in range(t0, t1):
        if fec:
            b.plc_fec_feed([ev.vectors(t, s) for s in range(ev.n)], ev.count[t], ev.skip[t], ev.clear[t])
        out[:, t - t0] = b.plc_step(np.stack([ev.frame(t, s) for s in range(ev.n)]), ev.lost[:, t])
    return out
