"""Streams that come and go, the host half, without a GPU.

lpcnet_amd/csrc/api_roster.h -- which pair lists lpcnet_batch_copy_streams accepts, how a list splits over the shards, the swap-remove planner --
has no engine or HIP include, so tests/tools/roster_host.c, a program of its own built with the address and undefined-behaviour sanitizers,
drives it for 1..40 streams on 1..8 shards and every set of up to 4 leaving streams: after the planned copies each shard's survivors are exactly
its new prefix, no pair has a leaving stream as its source, destinations are distinct and disjoint from the sources, the copies are as many as
the leaving streams inside the new prefix, and malformed lists are refused.  lpcnet_amd/roster.py restates the rule in Python: StreamRoster is
checked against it and through random join / leave sequences.  The new names are declared in the header, exported by the library and wrapped."""
import itertools
import os
import random
import re
import subprocess

import pytest

from lpcnet_amd import api
from lpcnet_amd.roster import StreamRoster, plan_leave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["lpcnet_batch_set_active", "lpcnet_batch_get_active", "lpcnet_batch_active_streams", "lpcnet_batch_copy_streams",
             "lpcnet_batch_get_decoder_vq_mem", "lpcnet_batch_set_decoder_vq_mem"]


def test_roster_header_alone(tmp_path):
    exe = str(tmp_path / "roster_host")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "roster_host.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-3000:])
    assert int(r.stdout.split()[1]) > 1000000                # (the checks ran)


def partition(n, K):
    """lpcnet_amd/csrc/api_shards.h: shard_partition"""
    base, extra = divmod(n, K)
    spans = [(k * base + min(k, extra), base + (k < extra)) for k in range(K)]
    return [s for s in spans if s[1]]


def check_plan(spans, active, leaving, pairs, new_active):
    gone = set(leaving)
    content = {s: s for f, c in spans for s in range(f, f + c)}
    srcs, dsts = [p[0] for p in pairs], [p[1] for p in pairs]
    assert len(set(dsts)) == len(dsts) and not set(srcs) & set(dsts) and not set(srcs) & gone
    for s, d in pairs:
        content[d] = content[s]
    need = 0
    for (f, _), a, na in zip(spans, active, new_active):
        survivors = {s for s in range(f, f + a) if s not in gone}
        assert na == len(survivors) and sorted(content[s] for s in range(f, f + na)) == sorted(survivors)
        need += sum(1 for s in range(f, f + na) if s in gone)
    assert len(pairs) == need


def test_python_planner_follows_the_rule():
    rnd = random.Random(5)
    for n, K in itertools.product((1, 2, 5, 9, 16, 23), (1, 2, 3, 8)):
        spans = partition(n, K)
        for full in (True, False):
            active = [c if full else rnd.randint(0, c) for _, c in spans]
            act = [f + i for (f, _), a in zip(spans, active) for i in range(a)]
            for m in range(0, 4):
                for leaving in itertools.combinations(act, m):
                    pairs, new_active = plan_leave(spans, active, leaving)
                    check_plan(spans, active, leaving, pairs, new_active)
    with pytest.raises(ValueError):
        plan_leave([(0, 4)], [2], [2])                       # not active
    with pytest.raises(ValueError):
        plan_leave([(0, 4)], [3], [1, 1])                    # twice
    assert plan_leave([(0, 6)], [6], [1, 5]) == ([(4, 1)], [4])      # the stream in the tail costs nothing
    assert plan_leave([(0, 3), (3, 3)], [3, 2], [0, 4]) == ([(2, 0)], [2, 1])


@pytest.mark.parametrize("n,K,seed", [(7, 1, 0), (12, 2, 1), (40, 8, 2), (5, 8, 3)])
def test_roster_stays_a_bijection_onto_the_prefixes(n, K, seed):
    rnd = random.Random(seed)
    spans = partition(n, K)
    r = StreamRoster(spans)
    next_id, moved_total = 0, 0
    for _ in range(300):
        ids = list(r.slots())
        if ids and (len(ids) == n or rnd.random() < 0.45):
            leave = rnd.sample(ids, rnd.randint(1, min(4, len(ids))))
            before, active = r.slots(), list(r.active)
            pairs, new_active = r.leave(leave)
            check_plan(spans, active, [before[i] for i in leave], pairs, new_active)
            after = r.slots()
            inv = {v: k for k, v in before.items()}
            for s, d in pairs:
                assert after[inv[s]] == d                    # the moved stream's id names its new slot
            moved = {inv[s] for s, _ in pairs}
            assert all(after[i] == before[i] for i in after if i not in moved) and set(after) == set(before) - set(leave)
            moved_total += len(pairs)
        else:
            loads = list(r.active)
            slot = r.join(next_id)
            k = next(k for k, (f, c) in enumerate(spans) if f <= slot < f + c)
            free = [j for j, (_, c) in enumerate(spans) if loads[j] < c]
            assert loads[k] == min(loads[j] for j in free) and k == min(j for j in free if loads[j] == loads[k])      # least loaded, first on a tie
            assert slot == spans[k][0] + loads[k]
            next_id += 1
        slots = r.slots()
        assert len(set(slots.values())) == len(slots)
        assert sorted(slots.values()) == [f + i for (f, _), a in zip(spans, r.active) for i in range(a)]
    assert moved_total > 0 or K > 2                          # (few streams per shard and join() levelling the loads: the leaving ones may all sit in the tails)
    if not r.slots():
        r.join("first")
    with pytest.raises(ValueError):
        r.join(next(iter(r.slots())))                        # an id joins once
    while sum(r.active) < n:
        r.join(("fill", sum(r.active)))
    with pytest.raises(RuntimeError):
        r.join("one too many")


def test_new_names_are_declared_exported_and_wrapped(hip_lib):
    text = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True).splitlines() if ln.strip()}
    for name in NEW_NAMES:
        assert re.search(r"LPCNET_EXPORT\s+int\s+" + name + r"\s*\(", text), name
        assert name in exported, name
        assert getattr(hip_lib, name).argtypes, name         # (api.load_library declares its arguments)
    for attr in ("active", "active_streams", "copy_streams", "get_decoder_vq_mem", "set_decoder_vq_mem"):
        assert hasattr(api.LPCNetBatch, attr), attr
    assert isinstance(api.LPCNetBatch.active, property) and api.LPCNetBatch.active.fset is not None
