"""The DRED encoder's FAST flavour, the parts that need no GPU: the switch's entry points (declared, exported, bound), the packer of the GRUs' sparse
input matrices (lpcnet_amd/csrc/dred_fast_pack.h, driven by tests/tools/dred_enc_fast_pack_host.c) against the blob's own encoder arrays, the fixture
(tests/golden/golden_dred_enc_fast_v1.npz, made by tests/tools/make_golden_dred_enc_fast.py) against the seeded blobs and inputs, and the NumPy
restatement of the FAST definition against the fixture's envelope -- without the compiled reference."""
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
import dred_enc_model as em  # noqa: E402
import make_golden_dred_enc_fast as mk  # noqa: E402
from lpcnet_amd import api  # noqa: E402

C_NAMES = ("lpcnet_batch_dred_enc_set_fast", "lpcnet_batch_dred_enc_get_fast")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_fast_v1.npz"))


@pytest.fixture(scope="module")
def parity():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_v1.npz"))


def test_the_switch_is_declared_exported_and_bound():
    L = api.load_library()
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    for name in C_NAMES:
        assert hasattr(L, name), name
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
        assert name in exported, name
    assert isinstance(api.LPCNetBatch.dred_enc_fast, property) and api.LPCNetBatch.dred_enc_fast.fset is not None
    assert "lpcnet_batch_set_fast and dred_set_fast do not change this kernel; its own switch is dred_enc_set_fast" in header


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dred_enc_fast_pack") / "dred_enc_fast_pack_host")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "lpcnet_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "dred_enc_fast_pack_host.c"), "-o", exe, "-lm"])
    return exe


@pytest.mark.parametrize("name", list(em.SETS))
def test_the_tile_image_holds_the_encoders_weights_and_zero_elsewhere(name, packer, tmp_path):
    blob = em.set_blob(name)
    (tmp_path / "blob.bin").write_bytes(blob)
    out = subprocess.check_output([packer, str(tmp_path / "blob.bin"), str(tmp_path / "image.bin")], text=True)
    assert out.strip().splitlines()[-1] == "ok", out
    raw = np.fromfile(str(tmp_path / "image.bin"), np.int32)
    net = em.DredEncNumpy(blob)
    at, empty = 0, 0
    for k in em.GRU_AT:
        G = net.layers[k]
        N, n_in = G["N"], net.widths[k - 1]
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
            for _ in range(cnt):
                c0 = int(idx[p]); p += 1
                want[grp * 8:grp * 8 + 8, c0:c0 + 4] = G["w"][blk].T          # [4 cols][8 rows] -> rows x cols
                have[grp, c0:c0 + 4] = True
                first_col[grp].add(c0)
                blk += 1
        assert np.array_equal(dense.view(np.uint32)[np.repeat(have, 8, 0)], want.view(np.uint32)[np.repeat(have, 8, 0)]), (name, k)
        assert not dense[~np.repeat(have, 8, 0)].any(), (name, k, "a weight where the row group has no block")
        assert want.any()
        # every tile's list: ascending, and the union of its row groups' blocks (the narrow set's tiles are partial: 16, 8 and 24 units)
        assert start[0] == 0 and start[-1] == blocks and (np.diff(start) >= 0).all()
        for t in range(tiles):
            for gate in range(3):
                mine = pos[start[3 * t + gate]:start[3 * t + gate + 1]]
                assert (np.diff(mine) > 0).all()
                g0 = (gate * N + 32 * t) // 8
                assert mine.tolist() == sorted(set().union(*first_col[g0:g0 + min(4, (N - 32 * t) // 8)])), (name, k, t, gate)
    assert at == raw.size
    assert empty > 0 or name == "narrow"          # (row groups without blocks: zero rows inside a union; the narrow set's few groups may all have some)


def test_the_fixtures_crcs_match_the_seeded_blobs_and_inputs(golden):
    feat = em.inputs()
    assert np.uint32(zlib.crc32(feat.tobytes())) == golden["in_crc"]
    for name in em.SETS:
        assert np.uint32(zlib.crc32(em.set_blob(name))) == golden["blob_crc_" + name]
        for kind in ("lat", "init"):
            assert golden["env_%s_%s" % (kind, name)].shape == (em.N_DFRAMES,) and (golden["env_%s_%s" % (kind, name)] > 0).all()
        for kind in ("gru", "mem"):          # (the final state's envelope stands at the index of a stream's last double frame)
            last = np.array([(em.COUNT == d + 1).any() for d in range(em.N_DFRAMES)])
            assert ((golden["env_%s_%s" % (kind, name)] > 0) == last).all()
    feat, count = mk.tile_inputs(), mk.tile_counts()
    assert np.uint32(zlib.crc32(feat.tobytes() + count.tobytes())) == golden["tile_in_crc"]
    assert golden["tile_lat"].shape == (mk.TILE_STREAMS, em.N_DFRAMES, em.SETS[mk.TILE_SET]["latent_dim"])
    assert {0, 1, em.N_DFRAMES} <= set(count.tolist())
    for T in (16, 32):
        for t0 in range(0, mk.TILE_STREAMS, T):
            assert len(set(count[t0:t0 + T].tolist())) > 1, (T, t0)
    assert np.uint32(zlib.crc32(em.long_inputs().tobytes())) == golden["long_in_crc"]
    assert golden["long_lat"].shape == (len(mk.LONG_GF_STREAMS), em.LONG_DFRAMES, 80) and golden["long_env_lat"].shape == (em.LONG_DFRAMES,)
    assert (golden["long_env_lat"] > 0).all() and (golden["long_env_init"] > 0).all()
    # the envelope is neither zero nor loose: the AVX2 build's approximations, far above the table tanh's 5e-6, far below the latents
    assert 1e-4 < golden["env_lat_tf"].max() < 1e-2
    for case in ("tf", "w256", "narrow", "tile", "long"):
        assert 0 < float(golden["restated_worst_" + case]) <= mk.RESTATED_CAP
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_dred_enc_fast_v1.npz")) < 333 * 1024


def test_the_numpy_restatement_sits_inside_the_envelope(golden, parity):
    """the FAST definition in NumPy against the fixture's gf values and envelope, no compiled reference: the narrow set whole, and the streams of the
    training widths that are through after one and two double frames (their outputs and their final states)"""
    feat = em.inputs()
    for name, pick in (("narrow", np.arange(em.N_STREAMS)), ("tf", np.array([1, 3]))):
        gruf = parity["gru_" + name].shape[1]
        env = np.stack([golden["env_%s_%s" % (k, name)] for k in ("lat", "init", "gru", "mem")])
        count = em.COUNT[pick]
        got = mk.FastEncNumpy(em.set_blob(name)).encode_all(feat[pick], count)
        gf = (parity["lat_" + name][pick], parity["init_" + name][pick], parity["gru_" + name][pick])
        worst = mk.worst_ratio(got, gf, env, count, gruf, what=name + " restated", kinds=(0, 1, 2))
        if name == "narrow":
            gf = gf[:2] + (np.concatenate([gf[2], golden["mem_gf_narrow"]], 1),)
            worst = max(worst, mk.worst_ratio(got, gf, env, count, gruf, what=name + " restated", kinds=(3,)))
        print(name, "restatement worst deviation / envelope %.4f" % worst)
        assert worst <= mk.RESTATED_CAP
