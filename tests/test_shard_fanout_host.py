"""The shard geometry and the fan-out runner of the batch API (lpcnet_amd/csrc/api_shards.h), on the host and alone: the header has no engine or
HIP include, so tests/tools/shard_fanout_host.c -- a program of its own -- drives it with a fake per-shard function.  Built twice with gcc, once with
the address and undefined-behaviour sanitizers and once with the thread sanitizer (the runner starts one thread per shard).  The program checks, for
1..40 streams on 1..16 devices: the partition against lpcnet_amd/shard.py's rule restated in C; every (first, count) of up to 12 streams clipped
against the shards; the owner lookup; and the runner in both modes -- every shard called once, the in-turn mode stopping at the first failure, the
threaded mode returning the first negative code in shard order, else the first positive one, each with the failing shard's own message."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_shard_geometry_and_runner(sanitize, tmp_path):
    exe = str(tmp_path / "shard_fanout_host")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-pthread",
                           "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"), os.path.join(ROOT, "tests", "tools", "shard_fanout_host.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout[-500:], r.stderr[-3000:])
    assert int(r.stdout.split()[1]) > 100000                 # (the checks ran)
