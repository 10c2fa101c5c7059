"""The DRED decoder's FAST flavour, the parts that need no GPU: the switch's entry points (declared, exported, bound), the packer of the GRUs' sparse
input matrices (lpcnet_amd/csrc/dred_fast_pack.h, driven by tests/tools/dred_fast_pack_host.c) against the blob's own arrays, and the fixture
(tests/golden/golden_dred_fast_v1.npz, made by tests/tools/make_golden_dred_fast.py) against the seeded blobs and inputs."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_model as dm  # noqa: E402
import make_golden_dred_fast as mf  # noqa: E402
from lpcnet_amd import api, synth  # noqa: E402

C_NAMES = ("lpcnet_batch_dred_set_fast", "lpcnet_batch_dred_get_fast")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_fast_v1.npz"))


def test_the_switch_is_declared_exported_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name in C_NAMES:
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
        assert name in exported, name
    assert isinstance(api.LPCNetBatch.dred_fast, property) and api.LPCNetBatch.dred_fast.fset is not None
    assert "lpcnet_batch_set_fast does not change this kernel; its\n *   own switch is dred_set_fast" in header


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dred_fast_pack") / "dred_fast_pack_host")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "dred_fast_pack_host.c"), "-o", exe, "-lm"])
    return exe


def blob_with_a_full_row_group():
    """the small decoder with the first row group of dec_dense2's input matrix given every block (seeded weights): the seeded sets' block masks
    (block_density = 0.5) have row groups without blocks but none with all of them"""
    s = dm.SETS["small"]
    m = dm.add_dred(synth.make_model(), s["widths"], s["latent_dim"])
    (w, wt), (idx, it) = m.arrays["dec_dense2_weights"], m.arrays["dec_dense2_weights_idx"]
    w, idx = np.asarray(w, np.float32).reshape(-1, 32), np.asarray(idx, np.int32).reshape(-1)
    n_in, cnt0 = s["widths"][0], int(idx[0])
    full = (np.random.default_rng(0xF011).standard_normal((n_in // 4, 32)) * 0.08).astype(np.float32)
    m.add("dec_dense2_weights", np.concatenate([full, w[cnt0:]]).reshape(-1), wt)
    m.add("dec_dense2_weights_idx", np.concatenate([[n_in // 4], np.arange(0, n_in, 4), idx[1 + cnt0:]]).astype(np.int32), it)
    return synth.blob_bytes(m)


@pytest.mark.parametrize("name", ["small", "mixed", "full"])
def test_the_tile_image_holds_the_blobs_weights_and_zero_elsewhere(name, packer, tmp_path):
    blob = blob_with_a_full_row_group() if name == "full" else dm.set_blob(name)
    (tmp_path / "blob.bin").write_bytes(blob)
    out = subprocess.check_output([packer, str(tmp_path / "blob.bin"), str(tmp_path / "image.bin")], text=True)
    assert out.strip().splitlines()[-1] == "ok", out
    raw = np.fromfile(str(tmp_path / "image.bin"), np.int32)
    net = dm.DredDecNumpy(blob)
    at, empty, full = 0, 0, 0
    for k in dm.GRU_AT:
        G = net.layers[k]
        N, n_in = G["N"], (net.widths[k - 1])
        head = raw[at:at + 4]
        tiles = (N + 31) // 32
        assert head[:3].tolist() == [n_in, N, tiles]
        blocks = int(head[3])
        start = raw[at + 4:at + 4 + 3 * tiles + 1]
        pos = raw[at + 5 + 3 * tiles:at + 5 + 3 * tiles + blocks]
        at += 5 + 3 * tiles + blocks
        dense = raw[at:at + 3 * N * n_in].view(np.float32).reshape(3 * N, n_in)
        at += 3 * N * n_in
        # the matrix the blob's block lists stand for
        want = np.zeros((3 * N, n_in), np.float32)
        have = np.zeros((3 * N // 8, n_in), bool)
        first_col = [set() for _ in range(3 * N // 8)]
        idx, p, blk = G["idx"], 0, 0
        for grp in range(3 * N // 8):
            cnt = int(idx[p]); p += 1
            empty += cnt == 0
            full += cnt == n_in // 4
            for _ in range(cnt):
                c0 = int(idx[p]); p += 1
                want[grp * 8:grp * 8 + 8, c0:c0 + 4] = G["w"][blk].T          # [4 cols][8 rows] -> rows x cols
                have[grp, c0:c0 + 4] = True
                first_col[grp].add(c0)
                blk += 1
        assert np.array_equal(dense.view(np.uint32)[np.repeat(have, 8, 0)], want.view(np.uint32)[np.repeat(have, 8, 0)]), (name, k)
        assert not dense[~np.repeat(have, 8, 0)].any(), (name, k, "a weight where the row group has no block")
        assert want.any()
        # every tile's list: ascending, and the union of its row groups' blocks
        assert start[0] == 0 and start[-1] == blocks and (np.diff(start) >= 0).all()
        for t in range(tiles):
            for gate in range(3):
                mine = pos[start[3 * t + gate]:start[3 * t + gate + 1]]
                assert (np.diff(mine) > 0).all()
                g0 = (gate * N + 32 * t) // 8
                assert mine.tolist() == sorted(set().union(*first_col[g0:g0 + min(4, (N - 32 * t) // 8)])), (name, k, t, gate)
    assert at == raw.size
    assert empty > 0 and (full > 0) == (name == "full"), (empty, full)          # row groups without blocks in every set, one with all of them in `full`


def test_the_fixtures_crcs_match_the_seeded_blobs_and_inputs(golden):
    for name in dm.SETS:
        blob = dm.set_blob(name)
        state, latents = dm.set_inputs(name)
        assert np.uint32(zlib.crc32(blob)) == golden["blob_crc_" + name]
        assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == golden["in_crc_" + name]
        assert golden["env_" + name].shape == (dm.N_LATENTS,) and (golden["env_" + name] > 0).all()
    state, latents = mf.tile_inputs()
    count = mf.tile_counts()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes() + count.tobytes())) == golden["tile_in_crc"]
    assert golden["tile_gf"].shape == (mf.TILE_STREAMS, 4 * dm.N_LATENTS, 20) and golden["tile_env"].shape == (dm.N_LATENTS,)
    assert {0, 1, dm.N_LATENTS} <= set(count.tolist())
    for T in (16, 32, 64):
        for t0 in range(0, mf.TILE_STREAMS, T):
            assert len(set(count[t0:t0 + T].tolist())) > 1, (T, t0)
    state, latents = dm.long_inputs()
    assert np.uint32(zlib.crc32(state.tobytes() + latents.tobytes())) == golden["long_in_crc"]
    assert golden["long_gf"].shape == (dm.LONG_STREAMS, 4 * dm.LONG_LATENTS, 20) and golden["long_env"].shape == (dm.LONG_LATENTS,)
    # the envelope is neither zero nor loose: the AVX2 build's reciprocal approximation, far above the table tanh's 5e-6, far below the features
    assert 1e-4 < golden["env_w256"].max() < 1e-2 and golden["long_env"][-1] > golden["long_env"][0]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_dred_fast_v1.npz")) < 333 * 1024
