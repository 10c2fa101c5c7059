#!/usr/bin/env python3
"""gpurun_out/prof (tools/profile_round.sh) -> profiles/r01_* (committed evidence)."""
import csv, glob, json, os, shutil, sys, collections
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gpurun_out", "prof")
DST = os.path.join(ROOT, "profiles")
RND = sys.argv[1] if len(sys.argv) > 1 else "r06"
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (kernel_source_hash: ties the PMC numbers to the kernel sources they were measured with)

def one(pattern):
    f = glob.glob(os.path.join(SRC, pattern), recursive=True)       # gpurun merges runs: take the newest
    return max(f, key=os.path.getmtime) if f else None

def counter_avg(dirname, counter):
    f = one(f"{dirname}/**/*counter_collection.csv")
    acc = collections.defaultdict(list)
    if f:
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == counter:
                acc[r["Kernel_Name"].split("(")[0].replace("void ", "")].append(float(r["Counter_Value"]))
    # the auto-tune's short launches (1 and 5 frames, every streams-per-workgroup value) are not the workload: per kernel, keep the
    # dispatches within 20 % of its largest value (= the full 25-frame launches)
    out = {}
    for k, v in acc.items():
        full = [x for x in v if x >= 0.8 * max(v)]
        out[k] = (sum(full) / len(full), len(full))
    return out

for fl, suffix in (("f32", ""), ("i8", "_int8"), ("f32_fast", "_fast"), ("i8_fast", "_int8_fast")):
    b = os.path.join(SRC, f"bench_{fl}.json")
    if os.path.exists(b) and os.path.getsize(b) and fl in ("f32", "i8"):
        shutil.copy(b, os.path.join(DST, f"{RND}_bench_n1{suffix}.json"))
    tr = one(f"stats_{fl}/**/*kernel_trace.csv")
    st = one(f"stats_{fl}/**/*kernel_stats.csv")
    if tr:
        # per kernel: the workload's launches only -- dispatches within 20 % of the kernel's longest one (a safeguard: the profiled runs set
        # LPCNET_HIP_NO_AUTOTUNE=1, so no trial launches should be there at all) -- in rocprofv3's own column layout
        dur = collections.defaultdict(list)
        for r in csv.DictReader(open(tr)):
            dur[r["Kernel_Name"]].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        rows = []
        for k, v in dur.items():
            full = [x for x in v if x >= 0.8 * max(v)]
            rows.append((k, len(full), sum(full), sum(full) / len(full), min(full), max(full), len(v) - len(full)))
        tot = sum(r[2] for r in rows) or 1
        with open(os.path.join(DST, f"{RND}_kernel_stats{suffix}.csv"), "w") as o:
            o.write("# rocprofv3 --kernel-trace --stats -- python bench.py --steps 3 --warmup 1" + (" --int8" if fl == "i8" else "")
                    + " (LPCNET_HIP_NO_AUTOTUNE=1); per kernel the workload's launches only (Dropped = shorter launches left out)\n")
            o.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","Dropped"\n')
            for k, n, t, avg, mn, mx, dropped in sorted(rows, key=lambda r: -r[2]):
                o.write(f'"{k}",{n},{t},{avg:.1f},{100.0 * t / tot:.2f},{mn},{mx},{dropped}\n')
    elif st:
        shutil.copy(st, os.path.join(DST, f"{RND}_kernel_stats{suffix}.csv"))
    fe, wr = counter_avg(f"fetch_{fl}", "FETCH_SIZE"), counter_avg(f"write_{fl}", "WRITE_SIZE")
    if fe and wr:
        with open(os.path.join(DST, f"{RND}_pmc_hbm_summary{suffix}.csv"), "w") as o:
            o.write("# rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes), python bench.py --steps 3 --warmup 1"
                    + {"f32": "", "i8": " --int8", "f32_fast": " --fast", "i8_fast": " --int8 --fast --spw 2"}[fl] + ", MI355X\n")
            o.write("# workload per launch: 2048 streams x 25 frames x 160 samples; values are per-dispatch averages in KB as reported\n")
            o.write("kernel,dispatches,FETCH_SIZE_KB_avg,WRITE_SIZE_KB_avg\n")
            for k in sorted(fe):
                o.write(f"{k},{fe[k][1]},{fe[k][0]:.1f},{wr.get(k, (0, 0))[0]:.1f}\n")
        sk = sorted((k for k in fe if "sample_kernel" in k), key=lambda k: -fe[k][0] * fe[k][1])      # the variant the bench ran, not the auto-tune's other candidates
        if sk:
            k = sk[0]
            json.dump({"kernel": k, "kernel_source_hash": bench.kernel_source_hash(), "fetch_size_kb": fe[k][0], "write_size_kb": wr[k][0],
                       "hbm_bytes_per_launch": (2 * fe[k][0] + wr[k][0]) * 1024,
                       "correction": "FETCH_SIZE doubled (gfx950 reports 1/2 of wide coalesced reads, MI355X_MICROARCH.md HBM section); WRITE_SIZE as reported",
                       "launch": "2048 streams x 25 frames x 160 samples = 8 192 000 output samples",
                       "command": "tools/profile_round.sh (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, --kernel-trace)"},
                      open(os.path.join(DST, f"{RND}_hbm_traffic{suffix}.json"), "w"), indent=1)
for src, dst in (("bench_single.json", "bench_single_stream.json"), ("bench_f32_fast.json", "bench_n1_fast.json"),
                 ("bench_i8_fast.json", "bench_n1_int8_fast.json"), ("rtf_demo.json", "demo_single_stream_rtf.json"),
                 ("bench_f32_fast_f16.json", "bench_n1_fast_fp16fc.json"), ("bench_i8_fast_f16.json", "bench_n1_int8_fast_fp16fc.json"),
                 ("bench_rehearsal_2ranks.json", "bench_rehearsal_2ranks_one_gpu.json"), ("bench_rehearsal_4ranks.json", "bench_rehearsal_4ranks_one_gpu.json"),
                 ("bench_rehearsal_4ranks_int8.json", "bench_rehearsal_4ranks_one_gpu_int8.json"),
                 ("bench_rt_f32.json", "bench_rt_f32.json"), ("bench_rt_int8.json", "bench_rt_int8.json"),
                 ("bench_skewed.json", "bench_n1_skewed.json"), ("bench_skewed_int8.json", "bench_n1_skewed_int8.json"),
                 ("bench_denseA_nw32.json", "bench_n1_denseA_nw32.json"), ("bench_denseA_nw36.json", "bench_n1_denseA_nw36.json"),
                 ("bench_denseA_nw40.json", "bench_n1_denseA_nw40.json"), ("bench_denseA_nw48.json", "bench_n1_denseA_nw48.json")):
    b = os.path.join(SRC, src)
    if os.path.exists(b) and os.path.getsize(b):
        txt = open(b).read()
        js = [ln for ln in txt.split("\n") if ln.startswith("{") and ln.rstrip().endswith("}")]      # (multi-rank runs: gloo prints its connection chatter to stdout too)
        open(os.path.join(DST, f"{RND}_{dst}"), "w").write(js[-1] + "\n" if js and not txt.lstrip().startswith("{\n") else txt)
# throughput at other batch sizes: one file, one bench line per (flavour, stream count)
sweep = []
for fl in ("f32", "i8"):
    for ns in (256, 512, 1024, 1536, 2048, 4096, 8192):
        b = os.path.join(SRC, f"bench_{fl}_n{ns}.json")
        if os.path.exists(b) and os.path.getsize(b):
            js = [ln for ln in open(b).read().split("\n") if ln.startswith("{") and ln.rstrip().endswith("}")]
            if js:
                sweep.append(js[-1])
if sweep:
    open(os.path.join(DST, f"{RND}_bench_stream_sweep.jsonl"), "w").write("\n".join(sweep) + "\n")
b1024 = os.path.join(ROOT, "gpurun_out", "sq", f"{RND}_n1024_sq_f32.csv")
if os.path.exists(b1024):
    shutil.copy(b1024, os.path.join(DST, f"{RND}_sq_counters_n1024.csv"))
px2 = os.path.join(SRC, "phase_x2.log")
if os.path.exists(px2):
    with open(os.path.join(DST, f"{RND}_phase_clocks_x2.txt"), "w") as o:
        o.write("# two-group sample kernel (sample_kernel_x2.hip.h): in-kernel s_memtime phase table of workgroup 0 (profiling build; LPCNET_HIP_LIB=.../liblpcnet_hip_prof.so\n"
                "# python tests/tools/x2_phase.py 12 2048), shader clocks per HALF-step; the instrumentation costs ~15 % here (11 clock reads per half-step)\n"
                "# columns: lead = top of the half-step (leader / thresholds / frame boundary); chain = GRU-B mat-vec; gatesB = its gates; heads = candidate heads of the other group;\n"
                "# start = start-value pass (waves 4..7: wait for the indices + 3 + 1.5 rounds of loads) + wait for its counter + the slots' start values; items; close;\n"
                "# tree = dual-FC prefetch wait + the tree of the other group (in front of the barrier); B1wait; P2 = gate stage; B2wait\n")
        o.write(open(px2).read())
for fl, suffix in (("f32", ""), ("i8", "_int8"), ("f32_fast", "_fast_f32")):
    b = os.path.join(ROOT, "gpurun_out", "sq", f"{RND}_sq_{fl}.csv")
    if os.path.exists(b):
        shutil.copy(b, os.path.join(DST, f"{RND}_sq_counters{suffix}.csv"))
ph = [os.path.join(SRC, f) for f in ("phase_f32.log", "phase_i8.log", "phase_f32_fast.log", "phase_i8_fast.log") if os.path.exists(os.path.join(SRC, f))]
if ph:
    with open(os.path.join(DST, f"{RND}_phase_clocks.txt"), "w") as o:
        o.write("# in-kernel s_memtime phase table (profiling build: LPCN_PROF_MASK=0xFFF python -m lpcnet_amd.build --prof; LPCNET_HIP_LIB=.../liblpcnet_hip_prof.so\n"
                "# python tests/tools/gpu_sweep.py 22 1024:4), shader clocks per sample step, workgroup 0; the instrumentation itself costs a few %\n"
                "# columns: B1wait = wait at the barrier behind GRU-A; P2 = GRU-A gates; P3tail = wait at the barrier behind GRU-B; P4 = tree; P5 = leader /\n"
                "# thresholds; gather, close = GRU-A begin / end work; fcpre = dual-FC prefetch (+ mirror arrival); gruB = GRU-B mat-vec (incl. recurrent part,\n"
                "# arrival wait, scalar-cache warm-up); items = GRU-A item chain; start = wait for the indices + gather + start values; P5a = GRU-B gates\n"
                "# (waves 0..3; int8 at two streams per workgroup: waves 2, 3) / early candidate heads (the other waves)\n")
        for f in ph:
            o.write("## " + os.path.basename(f) + "\n")
            o.write(open(f).read())
print(sorted(os.listdir(DST)))
