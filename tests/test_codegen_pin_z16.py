"""The measured kernels of the bf16-Z training path -- the one-kernel forward
writing a bf16 Z (graphconv_ws_bf16oz_kernel) and dW from a bf16 Z and a bf16
gradient (gemm_x1t_kernel), DESIGN.md §4.21 -- have their machine code pinned
like the other hot kernels (tools/pin_codegen.py, test_codegen_pin.py), in a
pin file of their own: tests/golden/codegen_pins_z16.json.  A mismatch means
"re-measure them on the GPU (tools/probe_train_z16.py) and re-pin" (python
tools/pin_codegen.py --write).  CPU test: hipcc cross-compiles the sources with
the library's flags."""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="hipcc absent")
def test_z16_kernels_codegen_matches_their_pins():
    import pin_codegen

    with open(pin_codegen.PINS_Z16) as f:
        pins = json.load(f)
    now = pin_codegen.compute(pin_codegen.KERNELS_Z16)
    assert set(now) == set(pins) and len(pins) == len(pin_codegen.KERNELS_Z16)
    for name, p in pins.items():
        assert now[name]["sha256"] == p["sha256"], (
            f"{p['what']}: machine code changed ({p['instructions']} -> {now[name]['instructions']} instructions); "
            "re-measure it on the GPU, then re-pin with python tools/pin_codegen.py --write")
