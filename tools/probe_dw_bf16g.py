"""Diagnostic: the weight gradient dW = Z^T g over a bf16 output gradient read
as stored (grl_linear_bwd_weight_bf16g: three plane products per block, no
widened copy), forms alternating in one process.

Cases: the C3 dW shape (M = 1M nodes, K = 1792, C = 256) and the F = C = 512
layer's (K = 3584, C = 512).  g is a bf16 [M, C] output gradient, out the
layer's bf16 ReLU output.  The forms:
  a  grl_relu_grad_bf16 writing g_eff16 + g_eff32 + db, then
     grl_linear_bwd_weight on g_eff32: the path without the bf16 entry;
  b  grl_relu_grad_bf16 writing g_eff16 + db, then
     grl_linear_bwd_weight_bf16g on g_eff16;
  c  the two GEMM calls alone, on operands made outside the timed region.
Then the whole layer, graph_conv(Xb, ..., relu=True, out_dtype=bfloat16)
forward + backward (X, W and b gradients) at the C3 graph
(TypedGraph.synthetic(1_000_000, 32.0, 6, seed=0)), F = C = 256, p = 0.3, with
the dw_bf16g path option 0 against 1.
Per case: ROUNDS rounds of 3 warm-up and CALLS timed calls between device
events, the forms taking turns, so each form's round-to-round spread is
visible next to the differences.  a and b must leave the same bits in dW, the
two layer forms the same bits in every gradient, and b must have taken the
bf16 entry (a nonzero workspace query).

Prints one JSON line per case and writes them to --out.  b_not_slower_than_a
is the default's decision rule: b's best round is not above a's best round by
more than the largest round-to-round spread of either form.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graph-representation-learning_amd"))
import torch  # noqa: E402

from grl import DropEdge, TypedGraph, _lib  # noqa: E402
from grl.ops import _relu_grad_bf16, graph_conv, linear_bwd_weight, linear_bwd_weight_bf16  # noqa: E402

CASES = [(1_000_000, 1792, 256), (1_000_000, 3584, 512)]
QUERY = "grl_linear_bwd_weight_bf16g_workspace_query"
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


def bit_checksum(t):
    return int(t.contiguous().view(torch.int32).to(torch.int64).sum())


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


def probe_case(M, K, C, rounds, calls, dev):
    gen = torch.Generator(device=dev).manual_seed(3)
    Z = torch.randn(M, K, device=dev, generator=gen)
    g = torch.randn(M, C, device=dev, generator=gen).to(BF16)
    out = torch.randn(M, C, device=dev, generator=gen).clamp_(min=0).to(BF16)  # a ReLU output: half of it zeros
    g16, g32, _ = _relu_grad_bf16(g, out, False, True)
    ws_b = getattr(_lib.lib(), QUERY)(Z.data_ptr(), Z.stride(0), g16.data_ptr(), g16.stride(0), M, K, C)
    if ws_b == 0:
        raise RuntimeError("the bf16 weight gradient is not eligible here (dw_bf16g = 0?)")
    res = {}

    def form_a():
        _, e32, db = _relu_grad_bf16(g, out, True, True)
        res["a"] = (linear_bwd_weight(Z, e32, None, False)[0], db)

    def form_b():
        e16, _, db = _relu_grad_bf16(g, out, True, False)
        r = linear_bwd_weight_bf16(Z, e16, False)
        if r is None:
            raise RuntimeError("form b fell off the bf16 entry")
        res["b"] = (r[0], db)

    forms = {"a_mask_f32_then_fp32_entry": form_a, "b_mask_then_bf16_entry": form_b,
             "c_fp32_entry_alone": lambda: linear_bwd_weight(Z, g32, None, False),
             "c_bf16_entry_alone": lambda: linear_bwd_weight_bf16(Z, g16, False)}
    with torch.no_grad():
        t = rounds_of(forms, rounds, calls)
        form_a()
        form_b()
    a, b, c32, c16 = (t[k] for k in forms)
    return {"tool": "probe_dw_bf16g", "what": "dW", "M": M, "K": K, "C": C,
            "dw_bits_equal": bool(torch.equal(res["a"][0].view(torch.int32), res["b"][0].view(torch.int32))),
            "db_bits_equal": bool(torch.equal(res["a"][1].view(torch.int32), res["b"][1].view(torch.int32))),
            "dw_bits": {"a": bit_checksum(res["a"][0]), "b": bit_checksum(res["b"][0])},
            "b_workspace_bytes": int(ws_b),
            # what a writes and reads back and b does not: the fp32 copy of the masked gradient
            "g_eff32_bytes_written_and_read": 2 * M * C * 4,
            "mfma_per_wave_per_k16_step": {"a": 48, "b": 24},
            **t,
            "time_ratio_b_over_a": round(b["ms_min"] / a["ms_min"], 4),
            "time_ratio_c_bf16_over_c_fp32": round(c16["ms_min"] / c32["ms_min"], 4),
            "b_faster_than_a": bool(b["ms_max"] < a["ms_min"]),
            "b_not_slower_than_a": not_slower(b, a), "c_bf16_not_slower_than_c_fp32": not_slower(c16, c32)}


def probe_layer(g, F, p, rounds, calls):
    dev = g.device
    C = F
    N, S = g.num_rows, g.segments
    gp = g.with_dropedge(DropEdge(p, 2, 0, True))
    gen = torch.Generator(device=dev).manual_seed(2)
    Xb = torch.randn(N, F, device=dev, generator=gen).to(BF16).requires_grad_(True)
    W = (torch.randn(S * F, C, device=dev, generator=gen) / (S * F) ** 0.5).requires_grad_(True)
    b = torch.randn(C, device=dev, generator=gen).requires_grad_(True)
    R = torch.randn(N, C, device=dev, generator=gen).to(BF16)

    def layer(option):
        def run():
            with _lib.options(dw_bf16g=option):
                Xb.grad = W.grad = b.grad = None
                graph_conv(Xb, gp, W, b, relu=True, out_dtype=BF16).backward(R)
        return run

    forms = {"option_0_fp32_dw": layer(0), "option_1_bf16_dw": layer(1)}
    res = rounds_of(forms, rounds, calls)
    grads = {}
    for name, fn in forms.items():
        fn()
        grads[name] = (Xb.grad.clone(), W.grad.clone(), b.grad.clone())
    g0, g1 = grads.values()
    o0, o1 = (res[k] for k in forms)
    return {"tool": "probe_dw_bf16g", "what": "layer fwd+bwd, out_dtype=bfloat16, ReLU, bias", "F": F, "C": C, "p": p,
            "gradient_bits_equal": bool(torch.equal(g0[0].view(torch.int16), g1[0].view(torch.int16))
                                        and torch.equal(g0[1].view(torch.int32), g1[1].view(torch.int32))
                                        and torch.equal(g0[2].view(torch.int32), g1[2].view(torch.int32))),
            **res, "time_ratio_1_over_0": round(o1["ms_min"] / o0["ms_min"], 4),
            "option_1_faster": bool(o1["ms_max"] < o0["ms_min"]), "option_1_not_slower": not_slower(o1, o0)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "linear_bwd_weight_bf16g_c3.json"))
    a = ap.parse_args()
    if a.rounds < 3 or a.calls < 20:
        ap.error("at least 3 rounds of 20 timed calls")
    dev = torch.device("cuda:0")
    _lib.set_option("dw_bf16g", 1)  # the forms name their path themselves, whatever the default is
    head = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls, "warmup": 3}
    lines = []
    for M, K, C in CASES:
        lines.append(json.dumps({**head, **probe_case(a.nodes if M == 1_000_000 else M, K, C, a.rounds, a.calls, dev)}))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    g = TypedGraph.synthetic(a.nodes, 32.0, 6, seed=0, device=dev)
    lines.append(json.dumps({**head, "nodes": a.nodes, "edges": g.nnz, "types": g.num_types,
                             **probe_layer(g, 256, 0.3, a.rounds, a.calls)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
