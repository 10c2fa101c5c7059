"""The packer on the host, for tests: builds tests/tools/deal_print_host.c (lpcnet_amd/csrc/model_pack.c compiled into a small program) and runs it on a
weight blob, optionally under a forced two-group map.  Returns what the two-group kernel derives its slot plan from, per wave, and the slot -> wave
maps the packer prints."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(workdir):
    """-> run(blob_bytes, force_x2=None) -> (have_x2, nw, {wave: dict(bounds=(b1, b2, b3), head=, live=, cand=)}, [map lines], stderr)"""
    exe = os.path.join(str(workdir), "deal_print_host")
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "deal_print_host.c"), "-o", exe, "-lm"])

    def run(blob_bytes, force_x2=None):
        blob = os.path.join(str(workdir), "model.blob")
        with open(blob, "wb") as f:
            f.write(blob_bytes)
        env = {k: v for k, v in os.environ.items() if not k.startswith("LPCN_DEAL")}
        env["LPCN_DEAL_PRINT"] = "1"
        if force_x2:
            env["LPCN_DEAL_FORCE_X2"] = force_x2
        r = subprocess.run([exe, blob], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
        lines = r.stdout.splitlines()
        head = lines[0].split()                                  # "x2 <have> nw <items per lane>"
        waves = {}
        for ln in lines[1:]:
            t = ln.split()
            if t and t[0] == "wave":
                waves[int(t[1])] = dict(bounds=tuple(int(x) for x in t[4:7]), head=int(t[8]), live=int(t[10]), cand=int(t[12]))
        maps = [ln.split("):", 1)[1].strip() for ln in r.stderr.splitlines() if ln.startswith("LPCN_DEAL slots")]
        return int(head[1]), int(head[3]), waves, maps, r.stderr
    return run
