"""Diagnostic: the two halves of row_linear's backward over a bf16 table
(DESIGN.md §4.25), forms alternating in one process.

dW from a bf16 X and an fp32 g (grl_linear_bwd_weight_bf16z: X staged as one
LDS plane, three plane products per block, no widened copy), M = 1M rows, at
emb2's shape (K = 512, C = 128) and the GraphConv GEMM's (K = 1792, C = 256):
  new    grl_linear_bwd_weight_bf16z on X16;
  chain  X16.float() then grl_linear_bwd_weight: the path without the entry;
  bare   grl_linear_bwd_weight alone on an fp32 table made outside the timed
         region (the chain's GEMM alone).
dX stored as bf16 by the GEMM (grl_linear_fwd_to_bf16), emb2's data gradient
g [M, 128] x W [128, 512]:
  new    grl_linear_fwd_to_bf16;
  chain  grl_linear_fwd_ex then .to(bfloat16);
  bare   grl_linear_fwd_ex alone.
Per case: ROUNDS rounds of 3 warm-up and CALLS timed calls between device
events, the forms taking turns, so each form's round-to-round spread is
visible next to the differences.  new and chain must leave the same bits, and
new must have taken its entry (a nonzero workspace query).

Prints one JSON line per case and writes them to --out.
new_beats_chain_by_more_than_the_spread is the options' default rule, read at
emb2's shape: new's best round is below chain's best round by more than the
largest round-to-round spread seen in the whole run.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graph-representation-learning_amd"))
import torch  # noqa: E402

from grl import _lib  # noqa: E402
from grl.ops import linear_bwd_weight, linear_bwd_weight_bf16z_f32g, linear_fwd_ex, linear_fwd_to_bf16  # noqa: E402

BF16 = torch.bfloat16
# (case, kind, K, C): dW of X [M, K] and g [M, C]; dX = g [M, K] x W [K, C] with K = 128, C = 512
CASES = [("dw_emb2", "dw", 512, 128), ("dw_graphconv", "dw", 1792, 256), ("dx_emb2", "dx", 128, 512)]


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


def probe_dw(M, K, C, rounds, calls, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    X16 = torch.randn(M, K, device=dev, generator=gen).to(BF16)
    X32 = X16.float()
    g = torch.randn(M, C, device=dev, generator=gen)
    ws = _lib.lib().grl_linear_bwd_weight_bf16z_workspace_query(X16.data_ptr(), X16.stride(0), g.data_ptr(), M, K, C)
    if ws == 0:
        raise RuntimeError("the bf16-Z dW is not eligible here (dw_bf16z_f32g = 0?)")
    res = {}

    def new():
        res["new"] = linear_bwd_weight_bf16z_f32g(X16, g, True)
        if res["new"] is None:
            raise RuntimeError("form new fell off the bf16-Z entry")

    def chain():
        res["chain"] = linear_bwd_weight(X16.float(), g, None, True)

    forms = {"new_bf16z_entry": new, "chain_widen_then_fp32_entry": chain,
             "bare_fp32_entry_alone": lambda: linear_bwd_weight(X32, g, None, True)}
    t = rounds_of(forms, rounds, calls)
    new()
    chain()
    equal = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(res["new"], res["chain"]))
    assert equal, "dW: new and chain differ in bits"
    return forms, t, {"dw_db_bits_equal": equal, "workspace_bytes": int(ws),
                      # what chain writes and reads back and new does not (the fp32 copy), and the table new reads
                      "widened_copy_bytes_written_and_read": 2 * M * K * 4, "x16_bytes": M * K * 2,
                      "mfma_per_wave_per_k16_step": {"new": 24, "chain": 48}}


def probe_dx(M, K, C, rounds, calls, dev):
    gen = torch.Generator(device=dev).manual_seed(4)
    g = torch.randn(M, K, device=dev, generator=gen)
    W = torch.randn(K, C, device=dev, generator=gen) / K ** 0.5
    out = torch.empty(M, C, dtype=BF16, device=dev)
    ws = _lib.lib().grl_linear_fwd_to_bf16_workspace_query(g.data_ptr(), K, W.data_ptr(), out.data_ptr(), C, M, K, C, 0)
    if ws == 0:
        raise RuntimeError("the bf16-output forward is not eligible here (linear_out_bf16 = 0?)")
    res = {}

    def new():
        res["new"] = linear_fwd_to_bf16(g, W, 0, None, False, 0)
        if res["new"] is None:
            raise RuntimeError("form new fell off the bf16-output entry")

    def chain():
        res["chain"] = linear_fwd_ex(g, W, 0, None, False, 0).to(BF16)

    forms = {"new_bf16_out_entry": new, "chain_fp32_entry_then_cast": chain,
             "bare_fp32_entry_alone": lambda: linear_fwd_ex(g, W, 0, None, False, 0)}
    t = rounds_of(forms, rounds, calls)
    new()
    chain()
    equal = bool(torch.equal(res["new"].view(torch.int16), res["chain"].view(torch.int16)))
    assert equal, "dX: new and chain differ in bits"
    return forms, t, {"dx_bits_equal": equal, "workspace_bytes": int(ws),
                      # what chain writes (fp32 out), reads back and writes again (bf16) where new writes bf16 once
                      "fp32_out_bytes_written_and_read": 2 * M * C * 4, "bf16_out_bytes": M * C * 2}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "row_linear_bwd_bf16_c3.json"))
    a = ap.parse_args()
    if a.rounds < 3 or a.calls < 20:
        ap.error("at least 3 rounds of 20 timed calls")
    dev = torch.device("cuda:0")
    _lib.set_option("dw_bf16z_f32g", 1)  # the forms name their path themselves, whatever the defaults are
    _lib.set_option("linear_out_bf16", 1)
    head = {"tool": "probe_row_linear_bwd_bf16", "device": torch.cuda.get_device_name(0), "rounds": a.rounds,
            "calls": a.calls, "warmup": 3, "lib": os.path.basename(_lib.LIB_PATH)}
    rows = []
    with torch.no_grad():
        for name, kind, K, C in CASES:
            forms, t, extra = (probe_dw if kind == "dw" else probe_dx)(a.rows, K, C, a.rounds, a.calls, dev)
            n, c, bare = (t[k] for k in forms)
            rows.append({**head, "case": name, "M": a.rows, "K": K, "C": C, **extra, **t,
                         "time_ratio_new_over_chain": round(n["ms_min"] / c["ms_min"], 4),
                         "time_ratio_new_over_bare": round(n["ms_min"] / bare["ms_min"], 4),
                         "gain_ms_chain_min_minus_new_min": round(c["ms_min"] - n["ms_min"], 4),
                         "largest_spread_ms": max(v["spread_ms"] for v in t.values())})
            torch.cuda.empty_cache()
    worst = max(r["largest_spread_ms"] for r in rows)  # the largest round-to-round spread seen in this run
    lines = []
    for r in rows:
        r["largest_spread_ms_of_the_run"] = worst
        r["new_beats_chain_by_more_than_the_spread"] = bool(r["gain_ms_chain_min_minus_new_min"] > worst)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
