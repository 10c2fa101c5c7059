"""The group schedule's host half (no GPU): the PLC planner with lanes (plc_plan.cpp through lpcnet_hip_plc_plan_lanes).

The plan of lanes == 1 is the plan of a PLC step as every step runs it with the schedule off (`the serial plan`).  A plan of 2 .. 4 lanes must
be that plan re-dealt, never another computation:
  I1  the launches and records that name a stream are the serial plan's, in the serial plan's order, and before the join -- the frame analysis
      on the whole batch -- they all sit in one lane;
  I2  before the join, launches of different lanes never name the same stream;
  I3  a group works in rows [slot, slot + cnt) of the n rows of the group buffers, and the rows of groups in different lanes are disjoint.
The control state after the step and the step's summary do not depend on the lanes."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import plc_model as pm  # noqa: E402
from lpcnet_amd import api  # noqa: E402

N, T = 96, 400
T_BURG, T_PRED, T_MIX, T_GROUP, T_ANALYSIS = range(5)
SYMBOLS = ("lpcnet_batch_set_group_schedule", "lpcnet_batch_get_group_schedule", "lpcnet_batch_group_form", "lpcnet_batch_last_groups",
           "lpcnet_hip_plc_plan_lanes")


def test_symbols_are_exported_declared_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
    assert isinstance(api.LPCNetBatch.group_schedule, property)
    for m in ("group_form", "last_groups"):
        assert callable(getattr(api.LPCNetBatch, m)), m
    assert callable(api.plc_plan_lanes)


def sequences():
    """name -> (lost [N][T], fec_op [T][N]): seeded random loss at 5, 20 and 60 %, and the fixture's patterns; random FEC traffic"""
    out = {}
    for pct in (5, 20, 60):
        rng = np.random.default_rng([pct, 0x5C4ED])
        out["random %d %%" % pct] = (rng.uniform(size=(N, T)) < pct / 100).astype(np.uint8), rng.choice(5, size=(T, N), p=[.5, .3, .1, .02, .08]).astype(np.uint8)
    rng = np.random.default_rng(0xF1C)
    out["fixture"] = pm.loss_patterns(N, T), rng.choice(5, size=(T, N), p=[.5, .3, .1, .02, .08]).astype(np.uint8)
    return out


def named(launches, lists):
    """-> per launch (before the join?, lane, slot, cnt, key, records [cnt][ints per record]); key = what the launch does, apart from whom it names"""
    out, before = [], True
    for ty, op, lane, slot, cnt, off, rs, kind, n_s, preload in launches.tolist():
        if ty == T_ANALYSIS:
            before = False
            assert lane == 0 and cnt == 0
            out.append((False, 0, 0, 0, (ty,), np.zeros((0, 1), np.int32)))
            continue
        assert rs == {T_BURG: 1, T_PRED: 6, T_MIX: 3, T_GROUP: 1}[ty] and cnt > 0 and off >= 0 and off + cnt * rs <= lists.size
        key = (ty, op, kind, n_s, preload) if ty == T_GROUP else (ty, op)
        out.append((before, lane, slot, cnt, key, lists[off:off + cnt * rs].reshape(cnt, rs)))
    assert not before, "a plan has its analysis launch"
    return out


def per_stream(plan):
    """-> stream -> [(key, its record)] in launch order"""
    seq = {}
    for _, _, _, _, key, recs in plan:
        for r in recs.tolist():
            seq.setdefault(r[0], []).append((key, tuple(r)))
    return seq


def check_invariants(serial, plan, lanes, tag):
    assert per_stream(plan) == per_stream(serial), tag + ": I1, a stream's launches and records"
    lane_of = {}
    spans = []
    for before, lane, slot, cnt, key, recs in plan:
        assert 0 <= lane < lanes, tag
        if not before:
            assert lane == 0 and slot == 0, tag + ": from the analysis on everything is on lane 0"
            continue
        for s in recs[:, 0].tolist():
            assert lane_of.setdefault(s, lane) == lane, tag + ": I1 / I2, stream %d in lanes %d and %d" % (s, lane_of[s], lane)
        if key[0] == T_GROUP:
            assert slot >= 0 and slot + cnt <= N, tag + ": I3, rows [%d, %d) of %d" % (slot, slot + cnt, N)
            spans.append((lane, slot, slot + cnt))
    for la, a0, a1 in spans:
        for lb, b0, b1 in spans:
            assert la == lb or a1 <= b0 or b1 <= a0, tag + ": I3, lanes %d and %d share rows" % (la, lb)
    return {lane for before, lane, *_ in plan if before}


@pytest.mark.parametrize("options", [api.PLC_CAUSAL, api.PLC_CODEC | api.PLC_DC_FILTER])
def test_planner_invariants_at_every_lane_count(options):
    most = {lanes: 0 for lanes in (2, 3, 4)}
    for name, (lost, ops) in sequences().items():
        ctl = {lanes: np.zeros((N, 9), np.int32) for lanes in (0, 1, 2, 3, 4)}      # (0: lpcnet_hip_plc_plan)
        for c in ctl.values():
            c[:, 0] = 400
        for t in range(T):
            tag = "options %d, %s, step %d" % (options, name, t)
            summary = api.plc_plan(options, ctl[0], lost[:, t], ops[t])
            s1, launches, lists = api.plc_plan_lanes(options, ctl[1], lost[:, t], 1, ops[t])
            assert np.array_equal(s1, summary) and np.array_equal(ctl[1], ctl[0]), tag
            assert not launches[:, 2].any() and not launches[:, 3].any(), tag + ": one lane is lane 0, rows from 0"
            serial = named(launches, lists)
            check_invariants(serial, serial, 1, tag)
            for lanes in (2, 3, 4):
                sl, la, li = api.plc_plan_lanes(options, ctl[lanes], lost[:, t], lanes, ops[t])
                assert np.array_equal(sl, summary) and np.array_equal(ctl[lanes], ctl[0]), "%s, %d lanes" % (tag, lanes)
                assert li.size == lists.size and sorted(li.tolist()) == sorted(lists.tolist()), tag
                used = check_invariants(serial, named(la, li), lanes, "%s, %d lanes" % (tag, lanes))
                most[lanes] = max(most[lanes], len(used))
    assert most[2] == 2 and most[3] >= 3 and most[4] >= 3, most      # (else the run has shown nothing about lanes)


def test_one_lane_is_the_order_a_step_runs_today():
    """the serial plan, restated: lost streams' flushes, three rounds of prediction / 160 / 80 / shift, tail, prediction, concealed half; then the
    received streams' chain; the analysis; the rest"""
    lost, ops = sequences()["random 20 %"]
    ctl = np.zeros((N, 9), np.int32)
    ctl[:, 0] = 400
    for t in range(60):
        _, la, _ = api.plc_plan_lanes(api.PLC_CAUSAL, ctl, lost[:, t], 1, ops[t])
        types = la[:, 0].tolist()
        assert types.count(T_ANALYSIS) == 1
        j = types.index(T_ANALYSIS)
        if lost[:, t].any() and not lost[:, t].all():
            b = types.index(T_BURG)
            groups = [k for k in range(j) if types[k] == T_GROUP]
            tails = [k for k in groups if la[k, 7] == 2]
            assert len(tails) == 1 and tails[0] < b, "the lost streams' chain comes first"
            assert la[tails[0] + 1, 0] == T_PRED and la[tails[0] + 2, 0] == T_GROUP and la[tails[0] + 2, 4] == la[tails[0], 4] == lost[:, t].sum()
            assert la[b, 4] == N - lost[:, t].sum()


def expected_plan(spec):
    """spec: [(type, op, kind, N, preload, records)] -> (launches [k][10], lists), every launch on lane 0 in rows from 0, lists in launch order"""
    launches, lists = [], []
    for ty, op, kind, n_s, preload, recs in spec:
        rs = {T_BURG: 1, T_PRED: 6, T_MIX: 3, T_GROUP: 1, T_ANALYSIS: 0}[ty]
        recs = [[r] if rs == 1 else list(r) for r in recs]
        assert all(len(r) == rs for r in recs)
        launches.append([ty, op, 0, 0, len(recs), len(lists) if recs else 0, rs, kind, n_s, preload])
        lists += [x for r in recs for x in r]
    return np.array(launches, np.int32), np.array(lists, np.int32)


def test_one_lane_plan_of_two_hand_written_steps():
    """Four streams from a reset, LPCNET_PLC_CAUSAL; the expected launches and lists are written out from src/lpcnet_plc.c:188-340 and the order
    DESIGN.md 4.4 gives, not taken from the planner.  Step 1: streams 0 and 3 lost with a full PCM queue (400 samples: rounds of 160, 160 and 80,
    tail, concealed half), 1 and 2 received.  Step 2: stream 1 lost with one deferred feature vector to flush; 0 and 3 receive their first frame
    after a loss (prediction restored from copy 2, two deferred features, trial synthesis, cross-fade, teacher-forced half, queue tail); 2 receives."""
    QTAIL, QPUSH, QSHIFT, FAPPEND, XFADE = 0, 2, 3, 4, 8
    LOST, LAST, FIRST_BACK, KEPT = 1 | 32 | 64, 1 | 32 | 64 | 128, (2 << 1) | (2 << 3) | 32 | 64, (3 << 3) | 32 | 64      # prediction flags (plc_records.h)
    pred = lambda fl, ss: (T_PRED, 0, 0, 160, 0, [(s, fl, 0, 0, 0, 0) for s in ss])
    mix = lambda op, recs: (T_MIX, op, 0, 160, 0, recs)
    group = lambda kind, n_s, preload, ss: (T_GROUP, 0, kind, n_s, preload, ss)
    analysis = (T_ANALYSIS, 0, 0, 160, 0, [])

    def lost_chain(ss):
        out = []
        for n_s in (160, 160, 80):
            out += [pred(LOST, ss), group(1, n_s, n_s, ss), mix(QSHIFT, [(s, 0, 0) for s in ss])]
        return out + [group(2, 80, 0, ss), pred(LAST, ss), group(1, 80, 0, ss)]

    step1 = lost_chain([0, 3]) + [(T_BURG, 0, 0, 160, 0, [1, 2]), analysis, pred(KEPT, [1, 2]), mix(FAPPEND, [(1, 0, 1), (2, 0, 1)]), mix(QPUSH, [(1, 0, 0), (2, 0, 0)])]
    step2 = [group(0, 160, 0, [1])] + lost_chain([1]) + [
        (T_BURG, 0, 0, 160, 0, [0, 2, 3]), pred(FIRST_BACK, [0, 3]), mix(FAPPEND, [(0, 0, 0), (3, 0, 0)]), mix(FAPPEND, [(0, 1, 0), (3, 1, 0)]),
        group(1, 80, 0, [0, 3]), mix(XFADE, [(0, 0, 0), (3, 1, 0)]), group(1, 80, 80, [0, 3]), mix(QTAIL, [(0, 0, 0), (3, 0, 0)]),
        analysis, pred(KEPT, [2]), mix(FAPPEND, [(0, 2, 1), (2, 1, 1), (3, 2, 1)]), mix(QPUSH, [(2, 0, 0)])]
    ctl = np.zeros((4, 9), np.int32)
    ctl[:, 0] = 400
    for k, (lost, spec) in enumerate((([1, 0, 0, 1], step1), ([0, 1, 0, 0], step2))):
        _, launches, lists = api.plc_plan_lanes(api.PLC_CAUSAL, ctl, lost, 1)
        want_launches, want_lists = expected_plan(spec)
        assert np.array_equal(launches, want_launches), "step %d: launches\n%s\nexpected\n%s" % (k + 1, launches, want_launches)
        assert np.array_equal(lists, want_lists), "step %d: lists" % (k + 1)


def test_bad_arguments_leave_the_control_state_alone():
    ctl = np.zeros((4, 9), np.int32)
    ctl[:, 0] = 400
    before = ctl.copy()
    for lanes in (0, 5, -1):
        with pytest.raises(api.LPCNetError):
            api.plc_plan_lanes(api.PLC_CAUSAL, ctl, [1, 0, 0, 1], lanes, [1, 1, 0, 0])
        assert np.array_equal(ctl, before)
    with pytest.raises(api.LPCNetError):
        api.plc_plan_lanes(api.PLC_NONCAUSAL, ctl, [1, 0, 0, 1], 2)
    assert np.array_equal(ctl, before)
    L = api.load_library()
    launch, lists = np.zeros((2, 10), np.int32), np.zeros(64, np.int32)
    lost = np.array([1, 0, 0, 1], np.uint8)
    assert L.lpcnet_hip_plc_plan_lanes(0, 4, 2, ctl.ctypes.data, lost, None, None, launch.ctypes.data, 2, lists.ctypes.data, 64) == -4      # two launches do not hold a step
    assert np.array_equal(ctl, before) and "fit" in api.last_error()


SANITIZED_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "plc_plan.h"
int main()
{
    const int n = 96;
    unsigned x = 12345u;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (x >> 8) & 0xffff; };
    for (int lanes = 1; lanes <= 4; ++lanes)
        for (int options = 0; options <= 6; options += 6)
            for (unsigned pct = 5; pct <= 60; pct += pct < 20 ? 15 : 40) {
                std::vector<lpcn_plc_ctl> a(n), b(n);
                for (int s = 0; s < n; ++s) { lpcn_plc_ctl_reset(&a[s]); lpcn_plc_ctl_reset(&b[s]); }
                std::vector<unsigned char> lost(n);
                std::vector<int> sa(n * LPCN_PLC_SUMMARY), sb(n * LPCN_PLC_SUMMARY), launch(128 * PLC_LANES_REC), lists(64 * n + 64);
                char err[256];
                for (int t = 0; t < 400; ++t) {
                    for (int s = 0; s < n; ++s) {
                        lost[s] = rnd() % 100 < pct;
                        const unsigned op = rnd() % 10;
                        if (op < 3) { lpcn_plc_ctl_fec_add(&a[s], op == 2); lpcn_plc_ctl_fec_add(&b[s], op == 2); }
                    }
                    PlcPlan P;
                    if (plc_plan(options, n, a.data(), lost.data(), P, sa.data(), err, sizeof(err))) { printf("serial: %s\n", err); return 1; }
                    const int k = lpcn_plc_plan_lanes(options, n, lanes, b.data(), lost.data(), sb.data(), launch.data(), 128, lists.data(), (int)lists.size(), err, sizeof(err));
                    if (k < 0) { printf("lanes: %s\n", err); return 1; }
                    if (memcmp(a.data(), b.data(), sizeof(lpcn_plc_ctl) * n) || sa != sb) { printf("step %d: the lanes changed the control state\n", t); return 1; }
                    for (int i = 0; i < k; ++i) {
                        const int *r = &launch[(size_t)i * PLC_LANES_REC];
                        if (r[2] < 0 || r[2] >= lanes || r[3] < 0 || (r[0] == PLC_T_GROUP && r[3] + r[4] > n)) { printf("step %d launch %d: lane %d slot %d cnt %d\n", t, i, r[2], r[3], r[4]); return 1; }
                    }
                }
            }
    printf("ok\n");
    return 0;
}
"""


def test_planner_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, never loaded into python) links plc_plan.cpp with -fsanitize=address,undefined and plans the random sequences"""
    csrc = os.path.join(ROOT, "lpcnet_amd", "csrc")
    src, exe = tmp_path / "plan_main.cpp", tmp_path / "plan_main"
    src.write_text(SANITIZED_MAIN)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", csrc, "-I", os.path.join(ROOT, "include"),
           str(src), os.path.join(csrc, "plc_plan.cpp"), "-o", str(exe)]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and "runtime does not come first in initial library list" in r.stderr:
        pytest.skip("a preloaded library keeps the sanitizer's runtime from coming first here")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
