"""The JSON lines bench.py prints (GPU box): the plain run's line, the extra records of `--full` and the real-time mode (the code that produces the
real-time claim ran in no test, and the driver's line carried neither the measured sustained-stream figure nor BASELINE config 4's weights)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, timeout=1500):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=env, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2500:])
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_rt_mode_is_oracle_checked_and_carries_both_clocks():
    """`bench.py --rt`: frame-at-a-time steps at two small stream counts -- the one-frame kernels at real-time grid shapes -- every step's wall AND device
    time, the timed steps' output checked against the oracle"""
    d = run_bench(["--rt", "--rt-sweep", "64,256", "--steps", "20"])
    assert d["parity_checked"] > 0 and len(d["rt"]) == 2
    for r in d["rt"]:
        assert r["parity_checked"] > 0 and r["steps"] == 20
        assert 0 < r["device_ms_p50"] <= r["step_ms_p50"] * 1.02 and r["device_ms_max"] >= r["device_ms_p50"]
        assert r["step_ms_p99"] < 10.0 and r["meets_deadline_p99"] and r["meets_deadline_p999"] and r["over_deadline_steps"] == len(r["late_steps"]) == 0
    assert d["realtime_streams_sustained"] == 256


def test_plain_line_carries_the_headline_and_nothing_that_takes_a_run_of_its_own():
    """`python bench.py --gpus 1 --steps K --warmup W`: set up, warm up, time, print -- the headline fields of the full line, on the same kernel, and none of the
    records that `--full` measures after the timed steps"""
    d = run_bench(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert d["metric"].startswith("16 kHz samples/sec") and d["unit"] == "samples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["config"]["streams_per_gpu"] == 2048 and d["config"]["streams_per_workgroup"] == 8
    assert d["value"] > 0 and abs(d["value"] * d["ms_per_step"] * 1e-3 / (2048 * 25 * 160) - 1.0) < 1e-9      # one step = 2048 streams x 25 frames x 160 samples
    assert d["parity_checked"] == 0 and d["realtime_streams_sustained"] is None
    assert not {"roofline", "also", "rt", "cpu_baseline", "envelope"} & set(d)


def test_default_line_shape_with_its_also_and_rt_records(monkeypatch):
    """`python bench.py --full` (here with fewer steps and without the CPU baseline): headline on the two-group kernel, `also` (BASELINE config 2's
    1024 streams, config 4's int8 weights), `rt` (measured sustained stream count), each oracle-checked"""
    d = run_bench(["--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    assert d["n_gpus"] == 1 and d["parity_checked"] == 8 and d["config"]["streams_per_gpu"] == 2048
    assert d["config"]["streams_per_workgroup"] == 8 and d["roofline"]["kernel"] == "lpcn::sample_kernel_x2"
    assert d["roofline"]["frac"] > 0.2 and d["roofline"]["library_matches_sources"]
    a = d["also"]
    assert a["config2_1024_streams"]["parity_checked"] == 8 and a["config2_1024_streams"]["streams_per_workgroup"] == 4
    assert a["int8_parity"]["parity_checked"] == 8 and a["int8_parity"]["value"] > a["config2_1024_streams"]["value"]
    assert d["value"] > a["config2_1024_streams"]["value"]                                  # eight streams per CU beat four
    rt = d["rt"]
    assert len(rt["probe"]) == 2 and all(p["parity_checked"] > 0 for p in rt["probe"])
    assert d["realtime_streams_sustained"] == rt["sustained_streams"] and rt["sustained_streams"] in (0, 7168, 8192)
    assert rt["sustained_streams"] <= d["realtime_streams_by_division"]                     # a deadline cannot beat a division


def test_fast_line_carries_its_envelope_check():
    """a FAST (not bit-exact) line says what it WAS checked against: the teacher-forced deviation from the PARITY engine on streams of the
    batch, inside the reference's own AVX2-vs-generic-C envelope"""
    d = run_bench(["--fast", "--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-extras"])
    assert d["parity_checked"] == 0 and d["envelope_checked"] == 4 and d["config"]["arithmetic"] == "fast"
    assert 0 <= d["envelope"]["max_gru_a_deviation"] < 1e-4 and 0 <= d["envelope"]["max_gru_b_deviation"] < 1e-4


def test_shard_threads_enqueue_their_steps_concurrently():
    """VERDICT r5 item 8 (what one GPU can show of the 8-shard real-time shape): eight host threads, one per shard of 896 streams, enqueue a 10-ms step each on
    the shard's own HIP stream -- the calls overlap in wall time (no lock serialises the step path) and each costs well under a millisecond of host time"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "shard_rt.py"), "--steps", "80"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["shards"] == 8 and d["streams_per_shard"] == 896
    assert d["overlap_factor"]["p50"] > 1.3, d["overlap_factor"]                           # 1.0 = serialised
    assert d["enqueue_us_per_shard_thread"]["p50"] < 500, d["enqueue_us_per_shard_thread"]
    assert d["enqueue_span_us_p50"] < 2000                                                  # all eight steps are in flight within 2 ms of a 10-ms period
