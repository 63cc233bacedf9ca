"""Diagnostic: the forward GEMM over an X stored as bf16 read as stored
(grl_linear_fwd_bf16x: X DMA'd into one LDS plane, three plane products per
block, no widened copy), forms alternating in one process.

Cases, M = 1M rows: emb2's shape (K = 512, C = 128, w_layout 1, bias + ReLU)
and the GraphConv GEMM's (K = 1792, C = 256, w_layout 0).  X16 is a bf16
[M, K] table.  The forms:
  new    grl_linear_fwd_bf16x on X16;
  chain  X16.float() then grl_linear_fwd_ex: the path without the bf16 entry;
  bare   grl_linear_fwd_ex alone on an fp32 table made outside the timed region.
Per case: ROUNDS rounds of 3 warm-up and CALLS timed calls between device
events, the forms taking turns, so each form's round-to-round spread is
visible next to the differences.  new and chain must leave the same bits in
out, and new must have taken the bf16 entry (a nonzero workspace query).

Prints one JSON line per case and writes them to --out.  new_not_slower_than_chain
is the default's decision rule: new's best round is not above chain's best
round by more than the largest round-to-round spread of either form.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graph-representation-learning_amd"))
import torch  # noqa: E402

from grl import _lib  # noqa: E402
from grl.ops import linear_fwd_bf16x, linear_fwd_ex  # noqa: E402

# (K, C, w_layout, bias + ReLU)
CASES = [("emb2", 512, 128, 1, True), ("graphconv_gemm", 1792, 256, 0, False)]
BF16 = torch.bfloat16


def timeit(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls


def rounds_of(forms, rounds, calls):
    times = {k: [] for k in forms}
    for _ in range(rounds):
        for name, fn in forms.items():
            times[name].append(timeit(fn, calls))
    return {k: {"ms_rounds": [round(x, 4) for x in t], "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                "spread_ms": round(max(t) - min(t), 4)} for k, t in times.items()}


def not_slower(new, old):
    """new's best round is not above old's by more than the spread seen between rounds."""
    return bool(new["ms_min"] <= old["ms_min"] + max(new["spread_ms"], old["spread_ms"]))


def probe_case(name, M, K, C, layout, epi, rounds, calls, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    X16 = torch.randn(M, K, device=dev, generator=gen).to(BF16)
    X32 = X16.float()
    W = torch.randn((C, K) if layout else (K, C), device=dev, generator=gen) / K ** 0.5
    b = torch.randn(C, device=dev, generator=gen) if epi else None
    ws = _lib.lib().grl_linear_fwd_bf16x_workspace_query(X16.data_ptr(), X16.stride(0), W.data_ptr(), M, K, C, 0)
    if ws == 0:
        raise RuntimeError("the bf16 forward is not eligible here (linear_bf16x = 0?)")
    res = {}

    def new():
        res["new"] = linear_fwd_bf16x(X16, W, layout, b, epi, 0)
        if res["new"] is None:
            raise RuntimeError("form new fell off the bf16 entry")

    def chain():
        res["chain"] = linear_fwd_ex(X16.float(), W, layout, b, epi, 0)

    forms = {"new_bf16_entry": new, "chain_widen_then_fp32_entry": chain,
             "bare_fp32_entry_alone": lambda: linear_fwd_ex(X32, W, layout, b, epi, 0)}
    with torch.no_grad():
        t = rounds_of(forms, rounds, calls)
        new()
        chain()
    equal = bool(torch.equal(res["new"].view(torch.int32), res["chain"].view(torch.int32)))
    assert equal, f"{name}: new and chain differ in bits"
    n, c, bare = (t[k] for k in forms)
    return {"tool": "probe_linear_bf16x", "case": name, "M": M, "K": K, "C": C, "w_layout": layout,
            "bias_relu": epi, "out_bits_equal": equal, "workspace_bytes": int(ws),
            # what chain writes and reads back and new does not (the fp32 copy), and the table new reads
            "widened_copy_bytes_written_and_read": 2 * M * K * 4, "x16_bytes": M * K * 2,
            "mfma_per_wave_per_k16_step": {"new": 24, "chain": 48},
            **t,
            "time_ratio_new_over_chain": round(n["ms_min"] / c["ms_min"], 4),
            "time_ratio_new_over_bare": round(n["ms_min"] / bare["ms_min"], 4),
            "new_faster_than_chain": bool(n["ms_max"] < c["ms_min"]),
            "new_not_slower_than_chain": not_slower(n, c), "new_not_slower_than_bare": not_slower(n, bare)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "linear_fwd_bf16x_c3.json"))
    a = ap.parse_args()
    if a.rounds < 3 or a.calls < 20:
        ap.error("at least 3 rounds of 20 timed calls")
    dev = torch.device("cuda:0")
    _lib.set_option("linear_bf16x", 1)  # the forms name their path themselves, whatever the default is
    head = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls, "warmup": 3}
    lines = []
    for name, K, C, layout, epi in CASES:
        lines.append(json.dumps({**head, **probe_case(name, a.rows, K, C, layout, epi, a.rounds, a.calls, dev)}))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
