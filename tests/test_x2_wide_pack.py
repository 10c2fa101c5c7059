"""Host tests of the two-group kernel's wide image of GRU-A (lpcnet_amd/csrc/model_pack.c: lpcn_model_pack_x2_wide; the streamed variants of the
two-group sample kernel, sample_x2w.hip): which models get one, what it looks like, and that the ordinary packer answers as before.  No GPU needed."""
import os
import sys

import pytest

from lpcnet_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = (48, 64, 80, 96)                                  # sample_variants.h: LPCN_VARIANTS_X2W
RESIDENT = 24                                                # lpcnet_engine.h: LPCN_X2W_NR

# model: (items per lane, items of waves 0..7 in P1, candidate-head items of waves 0..7) in today's two-group dealing
WIDE = {
    "densities": (dict(densities=(0.07, 0.07, 0.25)), 36, [20, 22, 26, 27, 10, 12, 14, 13], [0, 0, 0, 0, 24, 24, 22, 23]),
    "skew005": (dict(skew=0.05), 46, [12, 14, 18, 23, 22, 11, 11, 11], [0, 0, 0, 0, 24, 24, 21, 18]),
    "skew01": (dict(skew=0.1), 65, [6, 14, 19, 40, 41, 18, 9, 6], [0, 0, 0, 0, 24, 24, 19, 7]),
    "skew015": (dict(skew=0.15), 74, [2, 6, 21, 66, 50, 22, 2, 1], [0, 0, 0, 0, 24, 24, 18, 9]),
    "skew04": (dict(skew=0.4), 96, [0, 0, 0, 95, 72, 37, 0, 15], [0, 0, 0, 0, 24, 24, 2, 0]),
}


@pytest.mark.parametrize("name", list(WIDE))
def test_models_beyond_32_items_get_a_wide_image(name, hip_lib):
    kw, items, b3, head = WIDE[name]
    blob = synth.blob_bytes(synth.make_model(**kw))
    info = api.x2_wide_info(blob)
    assert info["fits"] == 1 and 33 <= info["items"] <= 96 and info["items"] == items
    assert info["variant"] in VARIANTS and info["variant"] >= info["items"] and info["variant"] == min(v for v in VARIANTS if v >= items)
    assert info["resident"] == RESIDENT and info["selftest"] == 0
    assert info["b3"] == b3 and info["head"] == head
    assert all(b + h <= items for b, h in zip(info["b3"], info["head"])) and max(b + h for b, h in zip(info["b3"], info["head"])) == items
    assert info["head"][:4] == [0, 0, 0, 0]                 # the chain waves carry no head
    rc, ck = api.check_model(blob)
    assert rc == 0 and ck[5] == 0
    assert api.x3_image_info(blob)[0] == 0                   # the twelve-wave form stays out of this


def test_the_heaviest_tail_needs_the_largest_variant(hip_lib):
    assert api.x2_wide_info(synth.blob_bytes(synth.make_model(skew=0.4)))["variant"] == max(VARIANTS)
    assert api.x2_wide_info(synth.blob_bytes(synth.make_model(densities=(0.07, 0.07, 0.25))))["variant"] == min(VARIANTS)


@pytest.mark.parametrize("kw", [dict(), dict(flavour="int8"), dict(grub_density=0.5, seed=5)], ids=["default", "int8", "sparse-grub"])
def test_models_the_wide_image_is_not_for(kw, hip_lib):
    blob = synth.blob_bytes(synth.make_model(**kw))
    info = api.x2_wide_info(blob)
    assert info["fits"] == 0 and info["variant"] == -1 and info["selftest"] == -1
    rc, ck = api.check_model(blob)
    assert rc == 0 and ck[5] == 0


def test_malformed_blob_is_reported(hip_lib):
    blob = synth.blob_bytes(synth.make_model(skew=0.1))
    assert api.x2_wide_info(blob[:1000])["fits"] == -1


def test_the_ordinary_packer_still_builds_no_image_above_32_items(tmp_path, hip_lib):
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    import deal_print
    run = deal_print.build(tmp_path)
    have, nw, waves, maps, err = run(synth.blob_bytes(synth.make_model(skew=0.1)))
    assert have == 0
    have, nw, waves, maps, err = run(synth.blob_bytes(synth.make_model()))
    assert have == 1 and nw == 30
