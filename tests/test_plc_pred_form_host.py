"""The PLC prediction kernels' form rule alone (plc_plan.cpp: lpcn_plc_pred_form through lpcnet_hip_plc_pred_form; no GPU): how many streams a
workgroup of a prediction launch carries, as a function of the number of records, the device's compute units, the network's widths and flavour,
and a pinned value.  The LDS of a form is restated here from the kernel's layout (plc_records.h: plc_pred_lds_bytes): per stream the 57 inputs
padded to 60, dense1's output, both GRU states, two scratch arrays of three gates over the wider GRU and the 20 outputs as floats, an int8 blob's
quantised GRU input and old state at four per dword, the 6-int control record and the live flag."""
import itertools
import os
import re
import subprocess

import pytest

from lpcnet_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 160 * 1024
FORMS = (1, 2, 4, 8)
WIDTHS = [(4, 8, 8), (8, 8, 40), (64, 264, 24), (128, 16, 16), (128, 256, 256), (128, 512, 264), (256, 512, 512), (512, 256, 512), (512, 512, 512)]
CUS = (1, 8, 64, 256, 304)
NS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 304, 305, 511, 512, 513, 608, 609, 1216, 1217, 2048, 2432, 2433, 8192, 1 << 20)


def lds_bytes(S, d1, g1, g2, int8):
    if S == 1:
        return 0                                       # (the S = 1 kernels have static LDS only: tests/test_kernel_resources_plc*.py)
    mg = max(g1, g2)
    dwords = 60 + d1 + g1 + g2 + 6 * mg + 20 + 6 + 1
    if int8:
        dwords += (max(d1, g1) + mg) // 4
    return 4 * S * dwords


def test_names_are_declared_exported_and_bound(hip_lib):
    header = open(os.path.join(ROOT, "include", "lpcnet_batch.h")).read()
    exported = {ln.split()[-1] for ln in subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True).splitlines() if ln.strip()}
    for name in ("lpcnet_batch_plc_set_pred_form", "lpcnet_batch_plc_get_pred_form", "lpcnet_hip_plc_pred_form"):
        assert re.search(r"LPCNET_EXPORT int " + name + r"\(", header), name
        assert name in exported, name
        assert getattr(hip_lib, name).argtypes is not None, name
    assert callable(api.plc_pred_form_table) and callable(api.LPCNetBatch.plc_pred_form)


def test_the_widest_network_fits_at_eight_streams_in_both_flavours(hip_lib):
    assert lds_bytes(8, 512, 512, 512, False) == 150240 and lds_bytes(8, 512, 512, 512, True) == 158432        # 146.7 KB and 154.7 KB of 160
    for int8 in (False, True):
        assert api.plc_pred_form_table(1, 256, 512, 512, 512, int8, pinned=8) == 8


def test_the_table_at_the_measured_rows(hip_lib):
    """profiles/plc_pred_forms.json, one MI355X (256 compute units): the fastest pinned form of every measured row"""
    for int8 in (False, True):
        for widths, at_8192 in (((128, 16, 16), 8), ((128, 256, 256), 4), ((512, 512, 512), 2)):
            got = [api.plc_pred_form_table(n, 256, *widths, int8) for n in (256, 512, 1024, 2048, 4096, 8192)]
            assert got == [1, 1, 1, 2, min(4, at_8192), at_8192], (int8, widths, got)


@pytest.mark.parametrize("int8", [False, True])
def test_table_over_a_grid(int8, hip_lib):
    for (d1, g1, g2), cus in itertools.product(WIDTHS, CUS):
        fits = [S for S in FORMS if lds_bytes(S, d1, g1, g2, int8) <= LIMIT]
        last = 1
        for n in NS:
            S = api.plc_pred_form_table(n, cus, d1, g1, g2, int8)
            assert S in fits, (n, cus, d1, g1, g2, S)
            if n <= cus:
                assert S == 1, (n, cus, S)
            assert S >= last, "not monotone in n: %s" % ((n, cus, d1, g1, g2, last, S),)
            last = S
            # the measured rule: the largest form of which four workgroups share a CU's LDS and whose workgroups fill those four places on every CU
            want = max([1] + [k for k in (2, 4, 8) if lds_bytes(k, d1, g1, g2, int8) <= LIMIT // 4 and (n + k - 1) // k >= 4 * cus])
            assert S == max(k for k in fits if k <= want), (n, cus, S, want)
            for pinned in FORMS:
                got = api.plc_pred_form_table(n, cus, d1, g1, g2, int8, pinned)
                assert got == max(k for k in fits if k <= pinned), (n, cus, d1, g1, g2, pinned, got)


def test_a_form_that_does_not_fit_is_halved(hip_lib):
    """no width the loader admits (up to 512 / 512 / 512) overflows at S = 8, so the fit is pinned on widths beyond them: the rule is a function of its
    arguments alone"""
    d1, g1, g2 = 512, 1024, 1024
    fits = [S for S in FORMS if lds_bytes(S, d1, g1, g2, False) <= LIMIT]
    assert fits == [1, 2, 4]
    assert api.plc_pred_form_table(8, 256, d1, g1, g2, pinned=8) == 4 and api.plc_pred_form_table(1 << 20, 256, d1, g1, g2, pinned=4) == 4
    assert [S for S in FORMS if lds_bytes(S, 512, 2048, 2048, True) <= LIMIT] == [1, 2]
    assert api.plc_pred_form_table(1 << 20, 256, 512, 2048, 2048, True) == 1 and api.plc_pred_form_table(8, 256, 512, 2048, 2048, True, pinned=4) == 2
    assert api.plc_pred_form_table(1 << 20, 256, 512, 8192, 8192, pinned=8) == 1 and api.plc_pred_form_table(1 << 20, 256, 512, 8192, 8192) == 1


def test_refusals(hip_lib):
    for pinned in (-1, 3, 5, 6, 7, 9, 16):
        with pytest.raises(api.LPCNetError, match=r"\(-4\).*pinned"):
            api.plc_pred_form_table(100, 256, 128, 256, 256, False, pinned)
    for args in ((-1, 256, 128, 256, 256), (100, 0, 128, 256, 256), (100, 256, 0, 256, 256), (100, 256, 128, 0, 256), (100, 256, 128, 256, 0)):
        with pytest.raises(api.LPCNetError, match=r"\(-4\)"):
            api.plc_pred_form_table(*args)
