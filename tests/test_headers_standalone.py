"""Every header an engine unit includes compiles as the only include of a translation unit (no GPU needed): it includes what it uses, so a
unit's include order carries no meaning.  Only <hip/hip_runtime.h> goes in front.  The compiler's front end alone runs, with the library's
include paths."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADERS = ["kernel_params.h", "spectral.hip.h", "engine_core.h", "plc_plan.h", "plc_records.h",
           "frame_kernels.hip.h", "decode_kernel.hip.h", "analysis_kernels.hip.h", "encode_kernels.hip.h", "plc_kernels.hip.h",
           "frame_nets.hip.h", "dred_kernels.hip.h", "roster_kernels.hip.h"]


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    from lpcnet_amd import build
    assert os.path.exists(os.path.join(build.CSRC, header))
    tu = tmp_path / "tu.hip"
    tu.write_text('#include <hip/hip_runtime.h>\n#include "%s"\n' % header)
    includes = [x for x in build.HIP_FLAGS if x.startswith("-I")]
    r = subprocess.run([build.HIPCC, "--offload-arch=" + build.ARCH, "-std=c++17", "-fsyntax-only"] + includes + [str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
