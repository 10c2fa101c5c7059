"""TEST INFRASTRUCTURE: a census of what the loud input families (loud_inputs.py) reach inside the sample loop.

The loop of src/lpcnet.c:235-271 restated in NumPy float32, sample by sample: the network (GRU-A, GRU-B, sampling tree, RNG)
and the two tables are the oracle's (orc_sample_network, orc_lin2ulaw, orc_ulaw2lin); the LPC history, the de-emphasis memory
and the last excitation are kept HERE, so that every intermediate can be recorded: the three embedding indices of each
sample, whether the mu-law conversion clamped at each of its three call sites, whether the PCM clipped, the largest state.

    python tests/tools/loud_census.py        prints the table of tests/tools/README.md

`math="engine"` takes the mu-law conversion and the PCM rounding from a host build of lpcnet_amd/csrc/lpcnet_math.h (the
functions the kernels' leader lanes call) instead: a third implementation next to the oracle and the reference.
`mutate` plants one of four mistakes of the kind a kernel rework can make, to show that the inputs notice them: the low PCM
clip dropped, the excitation byte of the index word cut to 7 bits (the quiet suite sees that one too: the excitation's reset value
is 128), the excitation gather right only for rows 32..223, and the clipped value kept as de-emphasis memory.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loud_inputs  # noqa: E402

f32 = np.float32
FRAME = loud_inputs.FRAME
MUTATIONS = ("no_low_clip", "exc7", "exc_inner", "deemph_clipped")
SITES = ("newest", "pred", "forced_exc")          # the three call sites of lin2ulaw (src/lpcnet.c:253, 254, 257)
ROLES = ("sig", "pred", "exc")                    # the three embedding gathers (src/lpcnet.c:154)


def engine_math(csrc=None, tmpdir=None):
    """host build of lpcnet_math.h: (lin2ulaw, round_pcm) as Python callables"""
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "loud_math_host.cpp")
    out = os.path.join(tmpdir or tempfile.mkdtemp(prefix="loudmath"), "libloud_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc or os.path.join(ROOT, "lpcnet_amd", "csrc"), src, "-o", out])
    L = C.CDLL(out)
    L.loud_lin2ulaw.argtypes = [C.c_float]
    L.loud_round_pcm.argtypes = [C.c_float]
    return L.loud_lin2ulaw, L.loud_round_pcm


def _log2_approx(x):
    """src/common.h:18-33 in float32"""
    i = int(np.array(x, f32).view(np.int32))
    integer = (i >> 23) - 127
    m = np.array(i - (integer << 23), np.int32).view(f32)[()]
    frac = m - f32(1.5)
    frac = f32(-0.41445418) + frac * (f32(0.95909232) + frac * (f32(-0.33951290) + frac * f32(0.16541097)))
    return f32(1 + integer) + frac


def lin2ulaw_np(x):
    """src/common.h:47-58 in float32 -> (code, clamped low, clamped high)"""
    x = f32(x)
    s = f32(1) if x >= 0 else f32(-1)
    scale = f32(255.0) / f32(32768.0)
    u = s * (f32(128) * (f32(0.69315) * _log2_approx(f32(1) + scale * abs(x))) / f32(5.5451774445))
    u = f32(128) + u
    lo, hi = bool(u < 0), bool(u > 255)
    if lo:
        u = f32(0)
    if hi:
        u = f32(255)
    return int(np.floor(0.5 + float(u))), lo, hi


class Census:
    """per-sample records of one stream (live frames only; arrays of length n)"""

    def __init__(self, fam, n):
        self.fam = fam
        self.pcm = fam.forced.copy()
        self.idx = np.zeros((3, n), np.int16)            # [role][sample]
        self.clamp_lo = np.zeros((3, n), bool)           # [site][sample]
        self.clamp_hi = np.zeros((3, n), bool)
        self.free = np.zeros(n, bool)                    # sample is free-running (not imposed)
        self.clip_lo = np.zeros(n, bool)
        self.clip_hi = np.zeros(n, bool)
        self.needs_unclipped_mem = np.zeros(n, bool)     # unclipped free sample right after a clipped one whose value would differ had the memory been clipped
        self.live = np.zeros(n, bool)
        self.max_state = 0.0
        self.max_pred = 0.0
        self.finite = True
        self.diverged_at = None                          # (mutations, with `stop_at_diff`) first sample that differs from `expect`


def run(om, fam, math="oracle", mutate=None, engine=None, expect=None):
    """one stream through the restated loop.  om: oracle.orc.OracleModel.  expect: PCM to compare with as the run goes; the run stops
    at the first difference (used with `mutate`)."""
    assert mutate in (None,) + MUTATIONS
    st = om.new_state()
    L = st.L
    T = loud_inputs.T
    n = T * FRAME
    c = Census(fam, n)
    feats = fam.features
    if math == "engine":
        e_lin2ulaw, e_round = engine or engine_math()
    if fam.tail:
        tca, tcb, _ = loud_inputs.tail_products(om, fam)
        L.orc_force_frame_count(st.p, T)
    last_sig = np.zeros(16, f32)
    deemph = f32(0)
    last_exc = L.orc_lin2ulaw(0.0)
    ca, cb, lpc = np.zeros(1152, f32), np.zeros(48, f32), np.zeros(16, f32)
    k85 = f32(0.85)
    for t in range(T):
        out = c.pcm[t * FRAME:(t + 1) * FRAME]
        if fam.tail:
            ca, cb, lpc = tca[t], tcb[t], fam.lpc
        else:                                             # the LPC as orc_synthesize takes it: the frame network's third product
            L.orc_frame_network(st.p, np.ascontiguousarray(feats[t, :20]), ca, cb, lpc)
        if st.signal_state()[3] <= 2:                     # src/lpcnet.c:239-243
            out[:] = 0
            continue
        preload = fam.preload[t]
        for i in range(FRAME):
            g = t * FRAME + i
            c.live[g] = True
            prods = last_sig * lpc                        # one rounded product per tap, subtracted in tap order
            pred = f32(0)
            for j in range(16):
                pred = pred - prods[j]
            sig_u, lo0, hi0 = lin2ulaw_np(last_sig[0])
            pred_u, lo1, hi1 = lin2ulaw_np(pred)
            if math == "engine":
                assert (sig_u, pred_u) == (e_lin2ulaw(float(last_sig[0])), e_lin2ulaw(float(pred))), (fam.name, g)
            else:
                assert (sig_u, pred_u) == (L.orc_lin2ulaw(float(last_sig[0])), L.orc_lin2ulaw(float(pred))), (fam.name, g)
            c.idx[:, g] = (sig_u, pred_u, last_exc)
            c.clamp_lo[0, g], c.clamp_hi[0, g], c.clamp_lo[1, g], c.clamp_hi[1, g] = lo0, hi0, lo1, hi1
            fed = last_exc                                # the excitation index as the gather sees it
            if mutate == "exc7":
                fed = last_exc & 0x7F
            elif mutate == "exc_inner":                   # a gather that is right only on the rows the quiet suite fetches
                fed = min(max(last_exc, 32), 223)
            exc = L.orc_sample_network(st.p, ca, cb, fed, sig_u, pred_u)
            if i < preload:
                x = f32(out[i])
                v = x - k85 * deemph - pred
                exc, lo2, hi2 = lin2ulaw_np(v)
                assert exc == (e_lin2ulaw(float(v)) if math == "engine" else L.orc_lin2ulaw(float(v))), (fam.name, g)
                c.clamp_lo[2, g], c.clamp_hi[2, g] = lo2, hi2
                pcm = x - k85 * deemph
            else:
                pcm = pred + f32(L.orc_ulaw2lin(exc))
                c.free[g] = True
            last_sig[1:] = last_sig[:-1].copy()
            last_sig[0] = pcm
            last_exc = exc
            prev_clipped = g > 0 and (c.clip_lo[g - 1] or c.clip_hi[g - 1])
            pre = pcm
            pcm = pcm + k85 * deemph
            unclipped = pcm
            lo, hi = bool(pcm < -32767), bool(pcm > 32767)
            clipped = f32(-32767) if lo else (f32(32767) if hi else pcm)
            if i >= preload:
                c.clip_lo[g], c.clip_hi[g] = lo, hi
                if math == "engine":
                    val = e_round(float(unclipped))
                elif mutate == "no_low_clip":
                    val = int(np.floor(0.5 + float(f32(32767) if hi else unclipped)))
                else:
                    val = int(np.floor(0.5 + float(clipped)))
                out[i] = np.array(val, np.int64).astype(np.int16)          # (short) of the C: wraps
                if prev_clipped and not (lo or hi):
                    alt = pre + k85 * np.clip(deemph, f32(-32767), f32(32767))
                    c.needs_unclipped_mem[g] = int(np.floor(0.5 + float(np.clip(alt, f32(-32767), f32(32767))))) != val
            deemph = clipped if mutate == "deemph_clipped" else unclipped
            m = max(float(np.max(np.abs(last_sig))), abs(float(deemph)))
            c.max_state = max(c.max_state, m)
            c.max_pred = max(c.max_pred, abs(float(pred)))
            if not (np.isfinite(m) and np.isfinite(pred)):
                c.finite = False
            if expect is not None and out[i] != expect[g]:
                c.diverged_at = g
                return c
    c.final = dict(last_sig=last_sig.copy(), last_exc=np.int32(last_exc), deemph_mem=f32(deemph))
    return c


def table(rows):
    """rows: [(family, Census)] -> the markdown table of tests/tools/README.md"""
    head = ("| family | group | free samples | clipped low / high | codes sig | codes pred | codes exc | lin2ulaw clamps low / high: newest, pred, forced exc"
            " | max abs state | max abs pred |\n|---|---|---|---|---|---|---|---|---|---|\n")
    lines = []

    def codes(a):
        return f"{np.unique(a).size} ({a.min()}..{a.max()})" if a.size else "-"

    def line(name, group, cs):
        live = np.concatenate([c.live for c in cs])
        idx = np.concatenate([c.idx for c in cs], axis=1)[:, live]
        free = np.concatenate([c.free for c in cs])
        cl = np.concatenate([c.clip_lo for c in cs]).sum(), np.concatenate([c.clip_hi for c in cs]).sum()
        lo = np.concatenate([c.clamp_lo for c in cs], axis=1).sum(axis=1)
        hi = np.concatenate([c.clamp_hi for c in cs], axis=1).sum(axis=1)
        clamps = ", ".join(f"{lo[s]} / {hi[s]}" for s in range(3))
        return (f"| {name} | {group} | {free.sum()} | {cl[0]} / {cl[1]} | {codes(idx[0])} | {codes(idx[1])} | {codes(idx[2])} | {clamps} | "
                f"{max(c.max_state for c in cs):.0f} | {max(c.max_pred for c in cs):.0f} |")

    for fam, c in rows:
        lines.append(line(f"`{fam.name}`: {fam.what}", fam.group, [c]))
    lines.append(line("**whole set**", "", [c for _, c in rows]))
    return head + "\n".join(lines) + "\n"


def main():
    from lpcnet_amd import synth
    from oracle import orc
    om = orc.OracleModel(synth.blob_bytes(synth.make_model(flavour="float")))
    print(table([(fam, run(om, fam)) for fam in loud_inputs.families()]))


if __name__ == "__main__":
    main()
