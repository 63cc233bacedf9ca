"""Codegen pins for the measured hot kernels.

The C3 headline kernel's time moved by 7 % with an unrelated change to its
argument list (6.71 -> 6.28 ms), so a silent change of its
machine code can move the headline.  This tool compiles the kernel sources
with the library's own flags (csrc/Makefile) to gfx950 assembly, extracts
the pinned kernels' instruction streams (comments, directives and label
names normalised away) and hashes them.  tests/test_codegen_pin.py compares
the hashes with tests/golden/codegen_pins.json: a mismatch means "re-measure
the kernel on the GPU and re-pin" (python tools/pin_codegen.py --write).
KERNELS_DW_BF16G is a second pin set with a file and a test of its own
(tests/golden/codegen_pins_dw_bf16g.json, tests/test_codegen_pin_dw_bf16g.py);
KERNELS_Z16 and KERNELS_DW_BF16Z_F32G likewise.

--all [--root TREE] hashes every kernel of every source in the Makefile's SRCS
instead, each file with its own flags (the per-object HIPFLAGS additions
included), and prints {source: {kernel symbol: {instructions, sha256}}}: two
trees whose outputs are equal build the same machine code.  It reads and
writes no pin.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "graph-representation-learning_amd", "csrc")
PINS = os.path.join(ROOT, "tests", "golden", "codegen_pins.json")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-Wall",
         "-Wno-unused-result", "--cuda-device-only", "-S"]

# (source, kernel-name prefix of the pinned instance, what it is)
KERNELS = [
    ("spmm.hip", "_ZN3grl12_GLOBAL__N_111spmm_kernelILi4ELi1ELi8ELb0ELb0ELb0EE",
     "C3 headline: typed-SpMM forward, whole 1 KiB rows (bench.py roofline.kernel)"),
    ("graphconv.hip", "_ZN3grl12_GLOBAL__N_119graphconv_ws_kernelILi16ELb0ELb0ELi1ELi8EEE",
     "one-kernel GraphConv forward at F=256 (inference / training forward)"),
    ("graphconv.hip", "_ZN3grl12_GLOBAL__N_119graphconv_ws_kernelILi16ELb0ELb1ELi1ELi8EEE",
     "one-kernel GraphConv data gradient at C=256 (grl_graphconv_bwd_data)"),
    ("graphconv.hip", "_ZN3grl12_GLOBAL__N_119graphconv_ws_kernelILi16ELb0ELb0ELi2ELi8EEE",
     "one-kernel GraphConv forward at F=512, C<=256 (gcn3 at d=256: two 256-column virtual segments)"),
    ("graphconv.hip", "_ZN3grl12_GLOBAL__N_119graphconv_ws_kernelILi16ELb0ELb0ELi2ELi4EEE",
     "one-kernel GraphConv forward at F=512, C<=512 (C5 shape: 4 gather + 8 MFMA waves)"),
]
# a pin set of its own (tests/test_codegen_pin_dw_bf16g.py; --write writes it too)
PINS_DW_BF16G = os.path.join(ROOT, "tests", "golden", "codegen_pins_dw_bf16g.json")
KERNELS_DW_BF16G = [
    ("linear.hip", "_ZN3grl12_GLOBAL__N_115gemm_x3t_kernelILi2EEE",
     "dW from a bf16 gradient, split-K slabs (grl_linear_bwd_weight_bf16g at C3: profiles/"
     "linear_bwd_weight_bf16g_c3.json)"),
]

# the bf16-Z training forward and its dW (tests/test_codegen_pin_z16.py; profiles/train_z16_c3.json)
PINS_Z16 = os.path.join(ROOT, "tests", "golden", "codegen_pins_z16.json")
KERNELS_Z16 = [
    ("graphconv.hip", "_ZN3grl12_GLOBAL__N_126graphconv_ws_bf16oz_kernelILi16ELb0ELi1ELi8EEE",
     "one-kernel GraphConv training forward at F=256 writing a bf16 out and a bf16 Z "
     "(grl_graphconv_fwd_train_bf16_z16)"),
    ("graphconv.hip", "_ZN3grl12_GLOBAL__N_126graphconv_ws_bf16oz_kernelILi16ELb0ELi2ELi8EEE",
     "the same at F=512, C<=256 (gcn3 at d=256)"),
    ("linear.hip", "_ZN3grl12_GLOBAL__N_115gemm_x1t_kernelILi2EEE",
     "dW from a bf16 Z and a bf16 gradient, split-K slabs (grl_linear_bwd_weight_bf16zg at C3)"),
]

# dW from a bf16 Z and an fp32 gradient (tests/test_codegen_pin_dw_bf16z_f32g.py; profiles/row_linear_bwd_bf16_c3.json)
PINS_DW_BF16Z_F32G = os.path.join(ROOT, "tests", "golden", "codegen_pins_dw_bf16z_f32g.json")
KERNELS_DW_BF16Z_F32G = [
    ("linear.hip", "_ZN3grl12_GLOBAL__N_116gemm_x3ta_kernelILi2EEE",
     "dW from a bf16 Z and an fp32 gradient, split-K slabs (grl_linear_bwd_weight_bf16z at emb2's shape and C3: "
     "profiles/row_linear_bwd_bf16_c3.json)"),
]


def kernel_stream(asm: str, prefix: str):
    m = re.search(r"^(" + re.escape(prefix) + r"[^:\s]*):", asm, re.M)
    if not m:
        raise KeyError(prefix)
    end = asm.find(".Lfunc_end", m.end())
    labels, out = {}, []
    for line in asm[m.end():end].split("\n"):
        t = line.split(";")[0].strip()
        if not t or (t.startswith(".") and not t.endswith(":")):
            continue
        if t.endswith(":"):
            labels.setdefault(t[:-1], f"L{len(labels)}")
            out.append(labels[t[:-1]] + ":")
            continue
        out.append(t)
    text = "\n".join(out)
    text = re.sub(r"\.LBB\d+_\d+", lambda mm: labels.get(mm.group(0), "L?"), text)
    return text, sum(1 for t in out if not t.endswith(":"))


def compute(kernels=None):
    kernels = KERNELS if kernels is None else kernels
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        asm = {}
        for src in sorted({s for s, _, _ in kernels}):
            out = os.path.join(tmp, src + ".s")
            subprocess.run([HIPCC] + FLAGS + [os.path.join(CSRC, src), "-o", out], check=True, capture_output=True)
            asm[src] = open(out).read()
        for src, prefix, what in kernels:
            text, n = kernel_stream(asm[src], prefix)
            res[prefix] = {"source": src, "what": what, "instructions": n,
                           "sha256": hashlib.sha256(text.encode()).hexdigest()}
    return res


def makefile_flags(csrc):
    """SRCS and each source's HIPFLAGS as csrc/Makefile gives them to the object rule."""
    mk = open(os.path.join(csrc, "Makefile")).read()
    root = os.path.abspath(os.path.join(csrc, "..", ".."))
    var = {"ARCH": "gfx950", "ROOT": root}
    sub = lambda v: re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], v)
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", mk, re.M).group(1).split()
    base = sub(re.search(r"^HIPFLAGS\s*:=\s*(.*)$", mk, re.M).group(1)).split()
    flags = {}
    for src in srcs:
        stem = src[:-len(".hip")]
        extra = re.findall(r"^\$\(OBJDIR\)/" + re.escape(stem) + r"\.o:\s*HIPFLAGS\s*\+=\s*(.*)$", mk, re.M)
        flags[src] = base + [f for e in extra for f in sub(e).split()] + ["-cuid=grl_" + stem]
    return srcs, flags


def compute_all(root):
    csrc = os.path.join(root, "graph-representation-learning_amd", "csrc")
    srcs, flags = makefile_flags(csrc)

    def one(src):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, src + ".s")
            subprocess.run([HIPCC] + flags[src] + ["--cuda-device-only", "-S", src, "-o", out], cwd=csrc, check=True,
                           capture_output=True)
            asm = open(out).read()
        res = {}
        for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
            text, n = kernel_stream(asm, sym)
            res[sym] = {"instructions": n, "sha256": hashlib.sha256(text.encode()).hexdigest()}
        return src, res

    with ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        return dict(ex.map(one, srcs))


if __name__ == "__main__":
    if "--all" in sys.argv:
        root = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else ROOT
        print(json.dumps(compute_all(os.path.abspath(root)), indent=1, sort_keys=True))
        sys.exit(0)
    for path, kernels in ((PINS, KERNELS), (PINS_DW_BF16G, KERNELS_DW_BF16G), (PINS_Z16, KERNELS_Z16),
                          (PINS_DW_BF16Z_F32G, KERNELS_DW_BF16Z_F32G)):
        pins = compute(kernels)
        if "--write" in sys.argv:
            with open(path, "w") as f:
                json.dump(pins, f, indent=1)
                f.write("\n")
        print(json.dumps(pins, indent=1))
