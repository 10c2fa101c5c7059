"""The slot plan of the two-group sample kernel (lpcnet_amd/csrc/slot_plan.h, round 10): which slot the start of P1 opens, which slots need
bias + diag*h formed, which slot the close stores.  Checked on the host, exhaustively, from the header the kernel includes: the start, the walk over
the slot boundaries and the close as the kernel runs them from the plan (tests/tools/slot_plan_host.cpp, on symbolic values) against a brute-force
restatement of the generic walk they replace -- open slot 0, form all three rows' start values, move through every slot at the boundaries and
through the empty ones at the close.  What is compared is what the rest of the kernel can observe: the value the first item is added to and the
final content of every cell that belongs to a row.  The packer is built on the host too: the four-stream map of the benchmark model is the one the
dealing of both images was measured with, and the two-group image of that model has the per-wave shapes the kernel's comments name."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

from lpcnet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY, UR, CAND, DUMMY = 0, 1, 2, 6
NW = 4                                                       # items per lane in these cases: all boundaries 0 <= b1 <= b2 <= b3 <= 4
BENCH_MAP = "c30:4 c22:7 c21:6 c19:5 c18:2 c15:3 12:1 8:0 7:5 6:6 5:7 5:0 5:3 4:5 3:7 3:6 3:1 2:2"


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("slot_plan") / "libslot_plan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tools", "slot_plan_host.cpp"), "-o", out])
    L = C.CDLL(out)
    L.sp_run.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    return L


def generic_walk(kind, parked, b1, b2, b3):
    """what the start, the items and the close did before the plan (sample_kernel_x2.hip.h up to round 9), on the same symbolic values"""
    cell = [(0, 0, 0), (1, 0, 0), (2, 0, 0)]
    read = lambda k: cell[k] if kind[k] != EMPTY else (DUMMY, 0, 0)
    acc = None
    for k in range(3):                                       # the start: every slot, needed or not
        bv = (3 + k, 0, 0)
        if k == 0:
            acc = bv if (kind[0] == CAND and not parked) else read(0)
        elif kind[k] == CAND:
            cell[k] = bv

    def swap(done, nxt):
        nonlocal acc
        if kind[done] != EMPTY:
            cell[done] = acc
        acc = read(nxt)

    first_item = (-1, 0, 0)
    for j in range(b3):
        if j == b1:
            swap(0, 1)
        if j == b2:
            swap(1, 2)
        if j == 0:
            first_item = acc
        acc = (acc[0], j if acc[1] == acc[2] else acc[1], j + 1)
    if b1 >= b3:                                             # the close: through every slot behind the open one
        swap(0, 1)
        swap(1, 2)
    elif b2 >= b3:
        swap(1, 2)
    if kind[2] != EMPTY:
        cell[2] = acc
    return first_item, cell


def all_cases():
    for kind in itertools.product((EMPTY, UR, CAND), repeat=3):
        for parked in (0, 1):
            for b1, b2, b3 in itertools.combinations_with_replacement(range(NW + 1), 3):
                yield kind, parked, b1, b2, b3


def test_start_walk_and_close_from_the_plan_equal_the_generic_walk(sp):
    """The plan is the WAVE's: a slot counts as live, or as holding candidate rows, if any lane says so.  The lane under test sits beside `other` lanes
    of every other slot triple -- a lane with an update / reset row or none where a neighbour holds a candidate, a lane that is on the start-forming
    path only because of its neighbours, a lane whose slot is skipped nowhere else: 27 x 27 lane pairs x parked x 35 boundary triples."""
    n = 0
    kinds = list(itertools.product((EMPTY, UR, CAND), repeat=3))
    out = (C.c_int * 12)()
    for kind, parked, b1, b2, b3 in all_cases():
        first_item, cell = generic_walk(kind, parked, b1, b2, b3)      # (per lane: what its neighbours hold never mattered to the generic walk)
        ck = (C.c_int * 3)(*kind)
        for other in kinds:
            sp.sp_run(ck, (C.c_int * 3)(*other), parked, b1, b2, b3, NW, out)
            case = (kind, other, parked, b1, b2, b3)
            if b3 > 0 and first_item[0] != DUMMY:            # (a lane without a row in the running slot: whatever it accumulates is never stored)
                assert tuple(out[0:3]) == first_item, case
            elif b3 == 0:
                assert out[0] == -1, case
            for k in range(3):
                if kind[k] != EMPTY:
                    assert tuple(out[3 + 3 * k:6 + 3 * k]) == cell[k], (case, k)
            n += 1
    assert n == 27 * 27 * 2 * 35


def test_plan_fields(sp):
    for kind, parked, b1, b2, b3 in all_cases():
        live = sum(1 << k for k in range(3) if kind[k] != EMPTY)
        cand = sum(1 << k for k in range(3) if kind[k] == CAND)
        plan = sp.sp_plan(live, cand, b1, b2, b3, 19 if parked else 0)
        bounds = (0, b1, b2, b3)
        with_items = [k for k in range(3) if bounds[k + 1] > bounds[k]]
        assert sp.sp_with_items(plan) == len(with_items)
        for k in range(3):
            assert bool(sp.sp_live(plan, k)) == (kind[k] != EMPTY)
            assert bool(sp.sp_parked(plan, k)) == (k == 0 and bool(parked))
            assert bool(sp.sp_forms_start(plan, k)) == (kind[k] == CAND and not (k == 0 and parked))
        plain = not any(sp.sp_forms_start(plan, k) for k in range(3))
        assert bool(sp.sp_plain_start(plan)) == plain
        assert sp.sp_last(plan) == (with_items[-1] if with_items else 0)
        assert sp.sp_first(plan) == (with_items[0] if with_items and plain else 0)
        assert sp.sp_first(plan) <= sp.sp_last(plan)


# ---------------------------------------------------------------------------------------------------------- the packer, on the host
@pytest.fixture(scope="module")
def deal_print(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import deal_print as dp
    run = dp.build(tmp_path_factory.mktemp("deal_print"))
    blob = synth.blob_bytes(synth.make_model())
    return lambda: run(blob)


def test_benchmark_model_keeps_its_measured_map(deal_print):
    have, nw, w, maps, err = deal_print()
    assert len(maps) == 2 and "two-group kernel" in err
    assert maps[0] == BENCH_MAP                              # the four-stream image
    assert maps[1] == BENCH_MAP                              # the two-group image is dealt the same way
    assert (have, nw) == (1, 30)
    assert [w[i]["bounds"] for i in range(8)] == [(8, 13, 13), (12, 15, 15), (18, 20, 20), (15, 20, 20), (6, 6, 6), (0, 7, 11), (0, 6, 9), (0, 5, 8)]
    assert [w[i]["head"] for i in range(8)] == [0, 0, 0, 0, 24, 19, 21, 22]
    assert [w[i]["cand"] for i in range(8)] == [0, 0, 1, 1, 1, 1, 1, 1]
    assert [w[i]["live"] for i in range(8)] == [3, 3, 3, 3, 1, 7, 7, 7]


def test_plans_of_the_benchmark_model(sp, deal_print):
    """chain waves 0 and 1: plain, close stores slot 1; chain waves 2 and 3: slot 0 alone forms start values; the leader: parked slot 0 opened and stored;
    row waves 5..7: slot 0 ran in the head -- the start opens slot 1 and nothing is moved in front of item 0"""
    w = deal_print()[2]
    plans = [sp.sp_plan(w[i]["live"], w[i]["cand"], *w[i]["bounds"], w[i]["head"]) for i in range(8)]
    assert [sp.sp_plain_start(p) for p in plans] == [1, 1, 0, 0, 1, 1, 1, 1]
    assert [sp.sp_first(p) for p in plans] == [0, 0, 0, 0, 0, 1, 1, 1]
    assert [sp.sp_last(p) for p in plans] == [1, 1, 1, 1, 0, 2, 2, 2]
    assert [[sp.sp_forms_start(p, k) for k in range(3)] for p in plans[2:4]] == [[1, 0, 0], [1, 0, 0]]
