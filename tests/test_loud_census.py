"""What the loud input families (tests/tools/loud_inputs.py) reach inside the sample loop, counted on the CPU.

tests/tools/loud_census.py restates the loop of the oracle's tail() (oracle/lpcnet_oracle.c, src/lpcnet.c:235-271) in NumPy
float32 around the oracle's network and tables, and records every sample's embedding indices, mu-law clamps, PCM clip and
state.  Two kinds of assertion:
  * the census is faithful: its PCM and final signal state equal the C oracle's on every family, bit for bit -- also with the
    mu-law conversion and the PCM rounding taken from a host build of the ENGINE's lpcnet_math.h (a third implementation);
  * the inputs reach the edges: conditions on the counts, so that tests/test_gpu_loud.py can say what it covers.
A third test plants four mistakes in the restated loop (no low clip, excitation index cut to 7 bits, excitation gather right only
on the inner rows, clipped value kept as de-emphasis memory): the loud families must notice each; the quiet inputs of the rest of
the suite notice only the 7-bit cut (codes >= 128 occur from the first sample on: the excitation's reset value is 128).
The oracle itself is tied to the compiled reference on the same families by tests/test_loud_golden.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import loud_census  # noqa: E402
import loud_inputs  # noqa: E402
from oracle import orc  # noqa: E402

FAMS = loud_inputs.families()
NAMES = [f.name for f in FAMS]


@pytest.fixture(scope="module")
def om(blob_f32):
    return orc.OracleModel(blob_f32)


@pytest.fixture(scope="module")
def censuses(om):
    return {f.name: loud_census.run(om, f) for f in FAMS}


@pytest.fixture(scope="module")
def oracle_runs(om):
    return {f.name: loud_inputs.run_oracle(om, f)[:2] for f in FAMS}


def _same_as_oracle(c, want):
    pcm, st = want
    assert np.array_equal(c.pcm, pcm)
    assert np.array_equal(c.final["last_sig"].view(np.uint32), st["last_sig"].view(np.uint32))
    assert c.final["last_exc"] == st["last_exc"] and np.float32(c.final["deemph_mem"]) == st["deemph_mem"]


@pytest.mark.parametrize("name", NAMES)
def test_census_is_faithful_to_the_c_oracle(name, censuses, oracle_runs):
    _same_as_oracle(censuses[name], oracle_runs[name])


def test_census_on_the_engines_host_math_is_faithful_too(om, oracle_runs, tmp_path):
    """lpcn_lin2ulaw and lpcn_round_pcm of lpcnet_amd/csrc/lpcnet_math.h, built for the host, in place of the oracle's: every call
    is compared with the NumPy restatement as the run goes, and the PCM with the C oracle's"""
    engine = loud_census.engine_math(tmpdir=str(tmp_path))
    for f in FAMS:
        _same_as_oracle(loud_census.run(om, f, math="engine", engine=engine), oracle_runs[f.name])


def test_the_inputs_reach_the_edges(censuses):
    cs = [censuses[n] for n in NAMES]
    table = loud_census.table([(f, censuses[f.name]) for f in FAMS])
    print("\n" + table)
    assert table in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "README.md")).read()      # the README shows what is measured here
    live = np.concatenate([c.live for c in cs])
    idx = np.concatenate([c.idx for c in cs], axis=1)[:, live]
    for r, role in enumerate(loud_census.ROLES):
        seen = np.unique(idx[r])
        assert 0 in seen and 255 in seen, role
        assert seen.size == 256, (role, sorted(set(range(256)) - set(seen.tolist())))       # no exemption needed: every code, every role
    lo = np.concatenate([c.clamp_lo for c in cs], axis=1).sum(axis=1)
    hi = np.concatenate([c.clamp_hi for c in cs], axis=1).sum(axis=1)
    for s, site in enumerate(loud_census.SITES):
        assert lo[s] > 0 and hi[s] > 0, (site, lo[s], hi[s])
    free = np.concatenate([c.free for c in cs])
    clip_lo, clip_hi = np.concatenate([c.clip_lo for c in cs]), np.concatenate([c.clip_hi for c in cs])
    assert not (clip_lo & ~free).any() and not (clip_hi & ~free).any()
    assert clip_lo.sum() >= 100 and clip_hi.sum() >= 100, (clip_lo.sum(), clip_hi.sum())
    assert sum(int(c.needs_unclipped_mem.sum()) for c in cs) >= 1
    assert all(c.finite for c in cs)
    # the history the LPC chain works on: several 10^4 with both signs (the quiet suite stays below 1700)
    assert max(c.max_state for c in cs) > 6e4 and max(c.max_pred for c in cs) > 6e4
    # what tests/test_gpu_loud.py relies on: the families it splits calls in do clip, the quiet neighbour does not
    assert censuses["alt80"].clip_lo.sum() + censuses["alt80"].clip_hi.sum() > 20
    assert not censuses["quiet80"].clip_lo.any() and not censuses["quiet80"].clip_hi.any()


def test_planted_mistakes_are_noticed_by_the_loud_families(om, censuses):
    """breaks a rework of the leader arithmetic can make; all but the 7-bit cut of the excitation index pass the quiet inputs"""
    plain = loud_inputs.Family("plain", "p0", 2600, np.zeros(loud_inputs.T * 160, np.int16), tuple([0] * loud_inputs.T),
                               what="free-running on the default features, as every other synthesis test")
    quiet = [(plain, loud_census.run(om, plain).pcm), (loud_inputs.by_name()["quiet80"], censuses["quiet80"].pcm)]
    assert np.abs(quiet[0][1].astype(np.int32)).max() < 3000
    for mut in loud_census.MUTATIONS:
        hit = [f.name for f in FAMS if f.name != "quiet80"
               and loud_census.run(om, f, mutate=mut, expect=censuses[f.name].pcm).diverged_at is not None]
        assert len(hit) >= 3, (mut, hit)
        for f, pcm in quiet:
            noticed = loud_census.run(om, f, mutate=mut, expect=pcm).diverged_at is not None
            assert noticed == (mut == "exc7"), (mut, f.name)
