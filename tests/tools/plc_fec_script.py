"""TEST TOOLING shared by tests/tools/make_golden_plc_fec.py and tests/test_gpu_plc_fec_feed.py: the 60-step script of loss flags and FEC
traffic that the batched FEC feed (lpcnet_batch_plc_fec_feed) is checked with, five streams, seeded.  Per step and stream: clear, then `skip`
NULL adds, then `count` vectors, then the step with its loss flag.

  stream 0   never lost.  40 vectors in each of steps 0..2: the ring is full in step 2 with nothing consumed beyond the rewind margin
             (keep == 0), so 20 vectors are dropped, and one more in step 3; from step 4 on every vector compacts the full ring first.
  stream 1   30 vectors in steps 0..2, then 3, 3, 2: fill 98 before step 6, whose 5 vectors take the last two rows, compact the ring and go on
             behind the moved rows.  Lost in steps 8..13 and 30..33: the concealment reads what was moved.
  stream 2   nothing for most steps, beside the others; three vectors at once every seventh step, skips, losses.
  stream 3   one vector per step as a receiver with redundancy sees them; every 13th step a clear followed by two vectors in the same call.
  stream 4   a seeded mix of everything.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plc_model as pm  # noqa: E402

f32 = np.float32
N, T = 5, 60


def script():
    """-> dict(lost [T][N] uint8, count [T][N] int32, skip [T][N] int32, clear [T][N] uint8, vec [sum(count)][20] float32: step 0's vectors first,
    within a step stream 0's first), and pcm [N][T][160] int16 the received frames"""
    rng = np.random.default_rng(0xFEED)
    lost = np.zeros((T, N), np.uint8)
    count = np.zeros((T, N), np.int32)
    skip = np.zeros((T, N), np.int32)
    clear = np.zeros((T, N), np.uint8)
    count[0:3, 0] = 40
    count[3:, 0] = 1
    count[0:3, 1] = 30
    count[3:7, 1] = (3, 3, 2, 5)
    count[7:, 1] = rng.integers(0, 3, T - 7)
    lost[8:14, 1] = 1
    lost[30:34, 1] = 1
    count[3::7, 2] = 3
    skip[5::11, 2] = 2
    lost[[4, 11, 12, 25, 26, 27, 45], 2] = 1
    count[:, 3] = 1
    clear[12::13, 3] = 1
    count[12::13, 3] = 2
    lost[[6, 20, 21, 22, 23, 40, 41, 52], 3] = 1
    count[:, 4] = rng.choice([0, 1, 1, 1, 2, 3], T)
    skip[:, 4] = rng.choice([0, 0, 0, 0, 1, 2], T)
    clear[:, 4] = rng.uniform(size=T) < 0.05
    lost[:, 4] = rng.uniform(size=T) < 0.2
    total = int(count.sum())
    vec = (rng.standard_normal((total, 20)) * 0.5).astype(f32)          # (shaped like plc_model.fec_schedule's)
    vec[:, 0] -= f32(3.0)
    vec[:, 18] = rng.uniform(-0.6, 0.6, total).astype(f32)
    vec[:, 19] = rng.uniform(-0.4, 0.4, total).astype(f32)
    pcm = np.stack([pm.stream_pcm(s, T) for s in range(N)])
    return dict(lost=lost, count=count, skip=skip, clear=clear, vec=vec, pcm=pcm)


def step_rows(sc, t):
    """rows of sc["vec"] that belong to step t: (first, end)"""
    first = int(sc["count"][:t].sum())
    return first, first + int(sc["count"][t].sum())
