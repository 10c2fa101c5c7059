"""Host tests of the twelve-wave image of GRU-A (lpcnet_amd/csrc/model_pack.c: lpcn_model_pack_x3; the two-group sample kernel at three waves per
SIMD): every block of the recurrent matrix in exactly one item, a row's blocks in the blob's order with the head of a cut candidate slot before its
tail, at most 16 items per lane, and no image -- not an error -- for the models that do not fit."""
import numpy as np
import pytest

from lpcnet_amd import api, synth

NW, SEGS, CHAIN_WAVES, LEADER = 16, 4, 4, 4
NONE, WHOLE, HEAD, TAIL = 0, 1, 2, 3


def group_counts(model):
    idx = np.asarray(model.get("sparse_gru_a_recurrent_weights_idx")).astype(int).ravel()
    out, i = [], 0
    while i < idx.size:
        out.append(int(idx[i]))
        i += idx[i] + 1
    assert len(out) == 144
    return out


MODELS = {
    "bench": dict(),
    "sparseA": dict(densities=(0.03, 0.03, 0.12)),
    "midA": dict(densities=(0.045, 0.045, 0.18)),
    "unshaped": dict(shaped=False, densities=(0.04, 0.06, 0.15), seed=77),
    "offgrid": dict(off_grid=True),
}


@pytest.mark.parametrize("name", list(MODELS))
def test_image_covers_every_block_in_order_within_sixteen_items(name, hip_lib):
    model = synth.make_model(**MODELS[name])
    blob = synth.blob_bytes(model)
    have, desc, rows, st = api.x3_image_info(blob)
    rc, info = api.check_model(blob)
    assert rc == 0 and info[5] == 0                      # with or without the image the blob is not reported as broken
    if name == "bench":
        assert have == 1                                 # the flagship model must have it
    if not have:
        pytest.skip("this model does not fit twelve waves x 16 items: the eight-wave kernels run it")
    assert st == 0
    counts = group_counts(model)
    summed = np.zeros(1152, int)                         # blocks of each row placed so far, in running order: heads, then P1
    for segs in ((0,), range(1, 1 + SEGS)):
        for w in range(12):
            for k in segs:
                kind, first, n, skip = desc[w, k]
                if kind == NONE:
                    assert (rows[w, k] < 0).all()
                    continue
                assert 0 <= first and first + n <= NW
                if k == 0:
                    assert w >= CHAIN_WAVES and w != LEADER and kind in (WHOLE, HEAD) and first + n == NW
                else:
                    assert kind in (WHOLE, TAIL) and first + n + desc[w, 0, 2] <= NW
                for r in rows[w, k][rows[w, k] >= 0]:
                    assert (r >= 768) == (k == 0 or kind == TAIL)
                    assert summed[r] == min(skip, counts[r // 8])      # a tail goes on exactly where its head stopped
                    summed[r] += max(0, min(n, counts[r // 8] - skip))
    assert [summed[8 * g] for g in range(144)] == counts and all((summed[8 * g:8 * g + 8] == counts[g]).all() for g in range(144))
    assert desc[:, :, 2].sum(axis=1).max() <= NW
    # a cut slot's head and tail sit on different waves
    for w in range(12):
        for k in range(1, 1 + SEGS):
            if desc[w, k, 0] == TAIL:
                assert not np.intersect1d(rows[w, k], rows[w, 0][rows[w, 0] >= 0]).size


def test_benchmark_model_is_cut_as_designed(hip_lib):
    have, desc, rows, st = api.x3_image_info(synth.blob_bytes(synth.make_model()))
    assert have == 1 and st == 0
    heads = desc[:, 0, :]
    assert (heads[:CHAIN_WAVES, 0] == NONE).all() and heads[LEADER, 0] == NONE
    assert sorted(int(x) for x in heads[heads[:, 0] != NONE][:, 2]) == [15, 16, 16, 16, 16, 16]
    assert sorted(int(x) for x in desc[:, 1:, :][desc[:, 1:, 0] == TAIL][:, 2]) == [2, 3, 5, 6, 14]
    assert int(desc[:, :, 2].sum()) == 188


@pytest.mark.parametrize("kw", [dict(flavour="int8"), dict(grub_density=0.5, seed=5), dict(skew=1.0), dict(densities=(0.05, 0.05, 0.3)),
                                dict(densities=(0.1, 0.1, 0.2))], ids=["int8", "sparse-grub", "skewed", "dense-candidates", "dense-update-reset"])
def test_models_that_do_not_fit_have_no_image_and_still_check_clean(kw, hip_lib):
    blob = synth.blob_bytes(synth.make_model(**kw))
    have, _, _, _ = api.x3_image_info(blob)
    assert have == 0
    rc, info = api.check_model(blob)
    assert rc == 0 and info[5] == 0


def test_malformed_blob_is_reported(hip_lib):
    blob = synth.blob_bytes(synth.make_model())
    assert api.x3_image_info(blob[:1000])[0] == -1
