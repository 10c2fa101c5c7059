"""The batched FEC feed's host planner (lpcnet_hip_plc_fec_feed_plan, no GPU needed) against lpcnet_plc_fec_add / lpcnet_plc_fec_clear restated
from the reference (src/lpcnet_plc.c:111-132) and applied vector by vector, and against the step planner's own fec_op path where that can
express the case."""
import os
import re

import numpy as np
import pytest

from lpcnet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, KEEP, READ, SKIP = 4, 5, 6, 7          # columns of ctl [n][9] (lpcn_plc_ctl)
MAX_FEC = 100


class Ring:
    """one LPCNetPLCState's FEC ring: the positions, and per row the id of the vector it holds (rows of the initial state: -1 - row)"""

    def __init__(self, fill, keep, read, skip):
        self.fill, self.keep, self.read, self.skip = fill, keep, read, skip
        self.rows = [-1 - r for r in range(MAX_FEC)]
        self.dropped = 0

    def add(self, v):          # src/lpcnet_plc.c:111-128
        if v is None:
            self.skip += 1
            return
        if self.fill == MAX_FEC:
            if self.keep == 0:
                self.dropped += 1
                return
            k = self.fill - self.keep
            self.rows[0:k] = self.rows[self.keep:self.keep + k]          # RNN_MOVE
            self.fill -= self.keep
            self.read -= self.keep
            self.keep = 0
        self.rows[self.fill] = v
        self.fill += 1

    def clear(self):           # :130-132
        self.keep = self.read = self.fill = self.skip = 0


def random_cases(rng, n):
    ctl = np.zeros((n, 9), np.int32)
    ctl[:, 0] = 400
    fill = rng.choice([0, 97, 98, 99, 100, 100, 100, -1], n)
    fill = np.where(fill < 0, rng.integers(0, 101, n), fill)
    keep = rng.choice([0, 0, 1, 50, 99, -1], n)
    keep = np.minimum(np.where(keep < 0, rng.integers(0, 101, n), keep), fill)
    read = keep + (rng.uniform(size=n) * (fill - keep + 1)).astype(np.int64)
    ctl[:, FILL], ctl[:, KEEP], ctl[:, READ] = fill, keep, np.minimum(read, fill)
    ctl[:, SKIP] = rng.choice([0, 0, 1, 3], n)
    count = rng.choice([0, 1, 3, 101, 150, 2, 5], n).astype(np.int32)
    skip = rng.choice([0, 0, 1, 2], n).astype(np.int32)
    clear = (rng.uniform(size=n) < 0.15).astype(np.uint8)
    return ctl, count, skip, clear


def apply_record(rows, rec, ids):
    """what plc_fec_feed_kernel does with one record, on row ids; ids = the packed source"""
    s, off, a, at_a, frm, moved, b, at_b = (int(x) for x in rec)
    assert 0 <= at_a and at_a + a <= MAX_FEC and 0 <= frm and frm + moved <= MAX_FEC and 0 <= at_b and at_b + b <= MAX_FEC and a + b > 0
    rows[at_a:at_a + a] = ids[off:off + a]
    if moved or b:                                        # a compaction: rows [frm, 100) to the front (none of them with keep == 100), b rows behind them
        assert frm > 0 and moved == MAX_FEC - frm and at_b == moved
    else:
        assert (frm, at_b) == (0, 0)
    rows[0:moved] = rows[frm:frm + moved]
    rows[at_b:at_b + b] = ids[off + a:off + a + b]
    return s


def test_symbols_are_exported_declared_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    for name in ("lpcnet_batch_plc_fec_feed", "lpcnet_batch_plc_fec_feed_device", "lpcnet_batch_plc_fec_feed_device_shard", "lpcnet_hip_plc_fec_feed_plan"):
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
    for m in ("plc_fec_feed", "plc_fec_feed_device"):
        assert callable(getattr(api.LPCNetBatch, m)), m


def test_planner_equals_the_reference_vector_by_vector():
    rng = np.random.default_rng(0xFEED1)
    n = 64
    seen = dict(mid=0, drop_keep0=0, a0_move=0, none=0, clear_then_vec=0, count0=0)
    for _ in range(60):                                   # 3840 cases
        ctl, count, skip, clear = random_cases(rng, n)
        rings = [Ring(*(int(x) for x in ctl[s, [FILL, KEEP, READ, SKIP]])) for s in range(n)]
        first = np.concatenate([[0], np.cumsum(count)])
        ids = list(range(int(first[-1])))
        for s, r in enumerate(rings):
            if clear[s]:
                r.clear()
            for _k in range(int(skip[s])):
                r.add(None)
            for v in ids[first[s]:first[s + 1]]:
                r.add(v)
        before = ctl.copy()
        rec, dropped = api.plc_fec_feed_plan(ctl, count, skip, clear)
        assert np.array_equal(ctl[:, [FILL, KEEP, READ, SKIP]], np.array([[r.fill, r.keep, r.read, r.skip] for r in rings]))
        assert np.array_equal(np.delete(ctl, [FILL, KEEP, READ, SKIP], 1), np.delete(before, [FILL, KEEP, READ, SKIP], 1))
        assert np.array_equal(dropped, [r.dropped for r in rings])
        got = {s: [-1 - r for r in range(MAX_FEC)] for s in range(n)}
        streams = [apply_record(got[int(r[0])], r, ids) for r in rec]
        assert streams == sorted(set(streams))            # one record per stream, in stream order
        for s in range(n):
            assert got[s] == rings[s].rows, (s, before[s], count[s], skip[s], clear[s])
            stored = count[s] - dropped[s]
            assert (s in streams) == (stored > 0)
        for r in rec:
            s = int(r[0])
            assert r[1] == first[s] and r[2] + r[6] == count[s] - dropped[s]
            seen["mid"] += int(r[2] > 0 and r[5] > 0 and r[6] > 0)
            seen["a0_move"] += int(r[2] == 0 and r[5] > 0)
            seen["clear_then_vec"] += int(clear[s])
        seen["drop_keep0"] += int(((dropped > 0) & (before[:, KEEP] == 0) & (clear == 0)).sum())
        seen["none"] += int(((count > 0) & (count == dropped)).sum())
        seen["count0"] += int((count == 0).sum())
    assert all(v > 20 for v in seen.values()), seen


@pytest.mark.parametrize("options", [api.PLC_CAUSAL, api.PLC_CODEC])
def test_planner_agrees_with_the_step_planners_fec_ops(options):
    """ops 1..4 of lpcnet_hip_plc_plan (a vector, a skip, a clear, two vectors before the step) are feeds of (count, skip, clear) =
    (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0): streams driven either way for 400 steps stay in the same state"""
    rng = np.random.default_rng(0xFEED2 + options)
    n, T = 48, 400
    a = np.zeros((n, 9), np.int32)
    a[:, 0] = 400
    b = a.copy()
    as_feed = {0: (0, 0, 0), 1: (1, 0, 0), 2: (0, 1, 0), 3: (0, 0, 1), 4: (2, 0, 0)}
    compactions = 0
    for t in range(T):
        op = rng.choice([0, 1, 1, 4, 4, 4, 2, 3], n, p=[.1, .2, .2, .15, .15, .1, .07, .03]).astype(np.uint8)
        lost = (rng.uniform(size=n) < 0.1).astype(np.uint8)
        sm_a = api.plc_plan(options, a, lost, op)
        f = np.array([as_feed[int(o)] for o in op])
        rec, _ = api.plc_fec_feed_plan(b, f[:, 0], f[:, 1], f[:, 2].astype(np.uint8))
        compactions += int((rec[:, 5] > 0).sum())
        sm_b = api.plc_plan(options, b, lost)
        assert np.array_equal(a, b) and np.array_equal(sm_a, sm_b), t
    assert compactions > 20                               # (each one found its ring full)


def test_planner_refuses_before_it_changes_anything():
    ctl = np.zeros((3, 9), np.int32)
    ctl[:, 0] = 400
    ctl[:, FILL] = 10
    before = ctl.copy()
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        api.plc_fec_feed_plan(ctl, [2, 1, -1], [1, 1, 1], [1, 0, 0])
    assert np.array_equal(ctl, before)
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        api.plc_fec_feed_plan(ctl, [2, 1, 1], [1, -2, 1])
    assert np.array_equal(ctl, before)
    bad = before.copy()
    bad[2, KEEP] = 11                                     # keep beyond read: ring positions out of order
    with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
        api.plc_fec_feed_plan(bad, [1, 1, 1])
    assert np.array_equal(bad[:2], before[:2])
    rec, dropped = api.plc_fec_feed_plan(ctl, [0, 0, 0])
    assert rec.shape == (0, 8) and not dropped.any() and np.array_equal(ctl, before)
