"""TEST INFRASTRUCTURE: seeded LOUD inputs for the sample loop, and the runners that drive the plain-C oracle and the compiled
reference over them.

Every other synthesis test feeds the loop signals below 6 % of full scale, so the +-32767 clip of the PCM, both clamps of the
float-to-mu-law conversion, the outer rows of the three embedding tables and an LPC history of several 10^4 are never reached
there.  The families here reach them (tests/test_loud_census.py counts what each one reaches, tests/tools/README.md holds the
table); tests/test_gpu_loud.py runs them through every form of the sample kernel.

A family is one stream: conditioning features from synth.make_features (the frame network stays what the other tests cover),
the samples imposed on the loop (teacher forcing, src/lpcnet.c:256-259), how many samples of each frame are imposed, and --
for the families that go through the tail entry point -- LPC coefficients supplied by the caller instead of the frame
network's.  Families of one GROUP share the per-frame preload counts, so they can sit in one batch call.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass

import numpy as np

from lpcnet_amd import synth

T = 20                     # frames per stream (the first two only fill the feature pipeline: 18 live frames = 2880 samples)
FRAME = 160
LIVE0 = 2 * FRAME          # first sample of the first live frame


@dataclass(frozen=True)
class Family:
    name: str
    group: str             # families of one group have the same `preload`
    feat_seed: int
    forced: np.ndarray     # [T*160] int16: the imposed samples (read only where sample-in-frame < preload[frame])
    preload: tuple         # [T] imposed samples per frame
    lpc: np.ndarray | None = None      # [16] caller-supplied LPC -> the stream runs through the tail entry point
    what: str = ""

    @property
    def features(self) -> np.ndarray:
        return synth.make_features(self.feat_seed, T)

    @property
    def tail(self) -> bool:
        return self.lpc is not None

    def segments(self):
        """[(first frame, end frame, preload)]: maximal runs of frames with one preload count = the calls of a batch run"""
        out, a = [], 0
        for t in range(1, T + 1):
            if t == T or self.preload[t] != self.preload[a]:
                out.append((a, t, self.preload[a]))
                a = t
        return out

    def digest(self) -> int:
        """CRC of everything the stream is driven with (the fixture stores it: a generator that drifts is told from a wrong result)"""
        c = zlib.crc32(self.features.tobytes())
        c = zlib.crc32(self.forced.tobytes(), c)
        c = zlib.crc32(np.asarray(self.preload, np.int32).tobytes(), c)
        if self.lpc is not None:
            c = zlib.crc32(self.lpc.tobytes(), c)
        return c


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def _resonator(r):
    """1 / (1 + a1 z^-1 + a2 z^-2) with poles r exp(+-0.3 i): at r = 1 the loop integrates its own excitation without decay"""
    lpc = np.zeros(16, np.float32)
    lpc[0], lpc[1] = np.float32(-2.0 * r * np.cos(0.3)), np.float32(r * r)
    return lpc


def families() -> list:
    n = T * FRAME
    k = np.arange(n)
    out = []

    def add(name, group, seed, forced, preload, lpc=None, what=""):
        pre = tuple([int(preload)] * T) if np.isscalar(preload) else tuple(int(p) for p in preload)
        assert len(pre) == T and forced.shape == (n,) and forced.dtype == np.int16
        out.append(Family(name, group, seed, forced, pre, lpc, what))

    # ---- half of every frame imposed, the other half free-running out of that history
    add("alt80", "p80", 31, np.where(k % 2 == 0, 32767, -32768).astype(np.int16), 80,
        what="full-scale alternation +32767 / -32768, sample by sample")
    rng = np.random.default_rng([31, 1])
    runs = np.repeat(np.arange(n), rng.integers(1, 8, n))[:n]                    # runs of 1..7 equal samples
    add("altrun80", "p80", 32, np.where(runs % 2 == 0, -32768, 32767).astype(np.int16), 80,
        what="full-scale alternation in runs of 1..7 samples")
    add("quiet80", "p80", 33, _i16(3000 * np.sin(k * 0.05) + 800 * np.sin(k * 0.31 + 1.0)), 80,
        what="3000-amplitude sine: the quiet neighbour of the loud streams of its group")
    # ---- whole frames imposed
    rail = np.array([-32768, 32767, -32768, -32768, 32767, 32767], np.int64)
    add("rails160", "p160", 34, rail[(k // FRAME) % 6].astype(np.int16), 160,
        what="frames made entirely of -32768 or entirely of +32767")
    rng = np.random.default_rng([31, 2])
    loud = rng.integers(-32768, 32768, n)
    add("loudsilent160", "p160", 35, np.where((k // FRAME) % 2 == 0, loud, 0).astype(np.int16), 160,
        what="full-range noise frames alternating with frames of digital silence")
    # ---- full-range uniform noise, a quarter frame and a single sample imposed
    for j, (pre, grp) in enumerate(((40, "p40"), (40, "p40"), (1, "p1"), (1, "p1"))):
        rng = np.random.default_rng([31, 3, j])
        add(f"noise{pre}{'ab'[j % 2]}", grp, 36 + j, rng.integers(-32768, 32768, n).astype(np.int16), pre,
            what=f"uniform int16 noise, {pre} imposed sample{'s' if pre > 1 else ''} per frame")
    # ---- loud AM sine imposed on the first frames only: the stream then free-runs out of a loud history
    sched = [160] * 8 + [0] * (T - 8)
    add("am160_0a", "p160_0", 40, _i16(30000 * np.sin(k * 0.3) * (0.55 + 0.45 * np.sin(k * 0.004))), sched,
        what="30000-amplitude AM sine for 8 frames, then free-running")
    add("am160_0b", "p160_0", 41, _i16(32767 * np.sin(k * 1.1 + 0.5) * (0.6 + 0.4 * np.sin(k * 0.011))), sched,
        what="32767-amplitude AM sine near a quarter of the sample rate for 8 frames, then free-running")
    # ---- caller-supplied resonator LPC through the tail entry point: the loop's own excitation drives it to full scale
    rng = np.random.default_rng([31, 4])
    kick = rng.integers(-32768, 32768, n).astype(np.int16)
    for j, r in enumerate((1.0, 0.998)):
        add(f"res{j}_free", "tail0", 42 + j, np.zeros(n, np.int16), 0, _resonator(r),
            what=f"resonator LPC (a1 = -2 r cos 0.3, a2 = r^2), r = {r}, free-running")
    for j, r in enumerate((1.0, 0.998)):
        add(f"res{j}_p16", "tail16", 44 + j, kick if j == 0 else kick[::-1].copy(), 16, _resonator(r),
            what=f"resonator LPC, r = {r}, 16 imposed noise samples per frame")
    assert len(out) < 16 and len({f.name for f in out}) == len(out)
    return out


def by_name() -> dict:
    return {f.name: f for f in families()}


def groups() -> dict:
    g = {}
    for f in families():
        g.setdefault(f.group, []).append(f)
    return g


def arrangements(group, n):
    """two orders of a group's families over n stream slots of a batch: the second shifted by one family, so that (with 2 or 3 families
    per group) every slot holds each of two different families once"""
    fams = groups()[group]
    return [[fams[(s + shift) % len(fams)] for s in range(n)] for shift in (0, 1)]


# ---- runners: one stream, alone, frame by frame -------------------------------------------------------------------------------
STATE_KEYS = ("gru_a", "gru_b", "last_sig", "last_exc", "deemph_mem", "rng")


def _pack_state(nnet, sig):
    ls, le, dm, fc, rng = sig
    return dict(gru_a=nnet[2].copy(), gru_b=nnet[3].copy(), last_sig=ls.copy(), last_exc=np.int32(le), deemph_mem=np.float32(dm),
                rng=rng.copy(), frame_count=int(fc))


def run_oracle(om, fam, frames=T):
    """-> (pcm [frames*160] int16, final state dict, the oracle state).  `om`: oracle.orc.OracleModel"""
    st = om.new_state()
    L = st.L
    feats = fam.features
    pcm = fam.forced[:frames * FRAME].copy()
    if fam.tail:
        ca, cb, _ = tail_products(om, fam)
        L.orc_force_frame_count(st.p, T)
        for t in range(frames):
            L.orc_synthesize_tail(st.p, ca[t], cb[t], fam.lpc, pcm[t * FRAME:(t + 1) * FRAME], FRAME, fam.preload[t])
    else:
        for t in range(frames):
            L.orc_synthesize(st.p, np.ascontiguousarray(feats[t, :20]), pcm[t * FRAME:(t + 1) * FRAME], FRAME, fam.preload[t])
    return pcm, _pack_state(st.nnet_state(), st.signal_state()), st


def tail_products(om, fam):
    """conditioning of a tail family: the frame network over the family's features on a fresh state (its own LPC is replaced)"""
    st = om.new_state()
    ca, cb, lp = np.zeros((T, 1152), np.float32), np.zeros((T, 48), np.float32), np.zeros((T, 16), np.float32)
    feats = fam.features
    for t in range(T):
        lp[t], ca[t], cb[t] = st.frame_network(feats[t])
    return ca, cb, lp


def run_reference(reflib, blob, fam):
    """the same through the compiled reference (oracle/ref.py RefLib): lpcnet_synthesize_impl per frame, or -- tail families --
    run_frame_network for every frame, then lpcnet_synthesize_tail_impl with the caller's LPC (ref_harness.c: ref_synthesize_tail)"""
    st = reflib.new_state(blob)
    lib = reflib.lib
    feats = fam.features
    pcm = fam.forced.copy()
    if fam.tail:
        ca, cb, lp = np.zeros((T, 1152), np.float32), np.zeros((T, 48), np.float32), np.zeros(16, np.float32)
        for t in range(T):
            lib.ref_run_frame_network(st.p, np.ascontiguousarray(feats[t, :20]), ca[t], cb[t], lp)
        for t in range(T):
            lib.ref_synthesize_tail(st.p, ca[t], cb[t], fam.lpc, pcm[t * FRAME:(t + 1) * FRAME], FRAME, fam.preload[t])
    else:
        for t in range(T):
            lib.ref_synthesize_impl(st.p, np.ascontiguousarray(feats[t, :20]), pcm[t * FRAME:(t + 1) * FRAME], FRAME, fam.preload[t])
    return pcm, _pack_state(st.nnet_state(), st.signal_state())
