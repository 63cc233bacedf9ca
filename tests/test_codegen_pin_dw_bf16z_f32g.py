"""The measured dW kernel over a bf16 Z and an fp32 gradient (gemm_x3ta_kernel,
DESIGN.md §4.25) has its machine code pinned like the other hot kernels
(tools/pin_codegen.py, test_codegen_pin.py), in a pin file of its own:
tests/golden/codegen_pins_dw_bf16z_f32g.json.  A mismatch means "re-measure it
on the GPU (tools/probe_row_linear_bwd_bf16.py) and re-pin" (python
tools/pin_codegen.py --write).  CPU test: hipcc cross-compiles the source with
the library's flags."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="hipcc absent")
def test_dw_bf16z_f32g_kernel_codegen_matches_its_pin():
    import pin_codegen

    with open(pin_codegen.PINS_DW_BF16Z_F32G) as f:
        pins = json.load(f)
    now = pin_codegen.compute(pin_codegen.KERNELS_DW_BF16Z_F32G)
    assert set(now) == set(pins) and len(pins) == len(pin_codegen.KERNELS_DW_BF16Z_F32G)
    for name, p in pins.items():
        assert now[name]["sha256"] == p["sha256"], (
            f"{p['what']}: machine code changed ({p['instructions']} -> {now[name]['instructions']} instructions); "
            "re-measure it on the GPU, then re-pin with python tools/pin_codegen.py --write")
