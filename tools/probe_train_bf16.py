"""Diagnostic: training the three GraphConv layers of GraphCNNDropEdge with
bf16 activations, forms alternating in one process.

The stack is the model's: x0 -> gcn1 -> g1 -> gcn2 -> g2, gcn3(cat[g1, g2]) ->
g3, every layer with ReLU, DropEdge 0.3 and a feature dropout 0.5 after it,
the loss taken on cat[g1, g3] (widened to fp32, as emb2 reads it), forward +
backward with X, W and b gradients, on the C3 graph
(TypedGraph.synthetic(1_000_000, 32.0, 6, seed=0)) with F = C = 256.  Forms:
  a  fp32 tables, outputs and gradients: graph_conv then feature_dropout;
  b  bf16 tables and outputs, the dropout a separate bf16 pass:
     feature_dropout(graph_conv(..., out_dtype=bfloat16));
  c  bf16, the dropout fused into the node: graph_conv(..., fdrop=);
  d  the two dropout entries alone on one [N, C] tensor, fp32 against bf16,
     with their bytes and the fraction of 8 TB/s they reach.
b and c must leave the same bits in every gradient.  Per form: ROUNDS rounds of
3 warm-up and CALLS timed calls between device events, the forms taking turns,
so each form's round-to-round spread is visible next to the differences.
torch.cuda.max_memory_allocated over one forward + backward is reported for a
and c.  A last line measures how far one training step of the whole model with
train_activation_dtype = bfloat16 lies from the fp32 model's (logits, loss and
every parameter gradient, relative Frobenius norm): recorded, not asserted.

Prints one JSON line per case and writes them to --out.  c_not_slower_than_b is
the model's decision rule: c's best round is not above b's best round by more
than the largest round-to-round spread of either form.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graph-representation-learning_amd"))
import torch  # noqa: E402

from grl import DropEdge, TypedGraph  # noqa: E402
from grl.ops import feature_dropout, feature_dropout_apply, graph_conv  # noqa: E402

BF16 = torch.bfloat16
HBM_BYTES_PER_S = 8e12


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
    t = t.contiguous()
    return int(t.view(torch.int16 if t.element_size() == 2 else torch.int32).to(torch.int64).sum())


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


def probe_stack(g, C, rounds, calls):
    dev = g.device
    N, S = g.num_rows, g.segments
    gen = torch.Generator(device=dev).manual_seed(2)
    edges = [g.with_dropedge(DropEdge(0.3, 2, i, True)) for i in range(3)]
    drops = [DropEdge(0.5, 2, (1 << 48) + i) for i in range(3)]
    X32 = torch.randn(N, C, device=dev, generator=gen).requires_grad_(True)
    X16 = X32.detach().to(BF16).requires_grad_(True)
    Ws = [(torch.randn(S * F, C, device=dev, generator=gen) / (S * F) ** 0.5).requires_grad_(True)
          for F in (C, C, 2 * C)]
    bs = [torch.randn(C, device=dev, generator=gen).requires_grad_(True) for _ in range(3)]
    R = torch.randn(N, 2 * C, device=dev, generator=gen)
    leaves = [X32, X16] + Ws + bs

    def stack(form):
        X = X32 if form == "a" else X16
        kw = {} if form == "a" else {"out_dtype": BF16}

        def layer(i, x):
            if form == "c":
                return graph_conv(x, edges[i], Ws[i], bs[i], relu=True, fdrop=drops[i], **kw)
            return feature_dropout(graph_conv(x, edges[i], Ws[i], bs[i], relu=True, **kw), drops[i])

        def run():
            for t in leaves:
                t.grad = None
            g1 = layer(0, X)
            g2 = layer(1, g1)
            g3 = layer(2, torch.cat([g1, g2], dim=-1))
            torch.cat([g1, g3], dim=-1).float().backward(R)
        return run

    forms = {"a_fp32": stack("a"), "b_bf16_unfused_dropout": stack("b"), "c_bf16_fused_node": stack("c")}
    res = rounds_of(forms, rounds, calls)
    grads, peak = {}, {}
    for name, fn in forms.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated())
        X = X32 if name == "a_fp32" else X16
        grads[name] = [X.grad.clone()] + [w.grad.clone() for w in Ws] + [b.grad.clone() for b in bs]
    gb, gc = grads["b_bf16_unfused_dropout"], grads["c_bf16_fused_node"]
    a, b, c = (res[k] for k in forms)

    def rel(x, y):
        return float((x.double() - y.double()).norm() / y.double().norm())

    ga = grads["a_fp32"]
    return {"tool": "probe_train_bf16", "what": "three GraphConv layers fwd+bwd, ReLU, DropEdge 0.3, dropout 0.5",
            "F": C, "C": C, **res,
            "b_c_gradient_bits_equal": bool(all(torch.equal(x.view(torch.int16 if x.dtype == BF16 else torch.int32),
                                                            y.view(torch.int16 if y.dtype == BF16 else torch.int32))
                                                for x, y in zip(gb, gc))),
            "gradient_bits": {"b": [bit_checksum(t) for t in gb], "c": [bit_checksum(t) for t in gc]},
            "c_vs_a_rel_fro": {"dX": rel(gc[0], ga[0]), "dW": [rel(gc[i], ga[i]) for i in (1, 2, 3)],
                               "db": [rel(gc[i], ga[i]) for i in (4, 5, 6)]},
            "max_memory_allocated_bytes": {"a_fp32": peak["a_fp32"], "c_bf16_fused_node": peak["c_bf16_fused_node"],
                                           "b_bf16_unfused_dropout": peak["b_bf16_unfused_dropout"]},
            "time_ratio_c_over_a": round(c["ms_min"] / a["ms_min"], 4),
            "time_ratio_c_over_b": round(c["ms_min"] / b["ms_min"], 4),
            "c_faster_than_b": bool(c["ms_max"] < b["ms_min"]), "c_not_slower_than_b": not_slower(c, b),
            "c_faster_than_a": bool(c["ms_max"] < a["ms_min"])}


def probe_dropout(N, C, rounds, calls, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    x32 = torch.randn(N, C, device=dev, generator=gen)
    x16 = x32.to(BF16)
    o32, o16 = torch.empty_like(x32), torch.empty_like(x16)
    de = DropEdge(0.5, 2, (1 << 48) + 1)
    forms = {"d_fp32_entry": lambda: feature_dropout_apply(x32, de, 0, out=o32),
             "d_bf16_entry": lambda: feature_dropout_apply(x16, de, 0, out=o16)}
    res = rounds_of(forms, rounds, calls)
    feature_dropout_apply(x16.float(), de, 0, out=o32)  # the contract's reference: the fp32 entry on the widened x
    same = bool(torch.equal(o16.view(torch.int16), o32.to(BF16).view(torch.int16)))
    bytes_ = {"d_fp32_entry": N * C * 8, "d_bf16_entry": N * C * 4}
    for k in forms:
        res[k]["bytes"] = bytes_[k]
        res[k]["fraction_of_8_TB_per_s"] = round(bytes_[k] / (res[k]["ms_min"] * 1e-3) / HBM_BYTES_PER_S, 4)
    return {"tool": "probe_train_bf16", "what": "feature dropout entries alone", "rows": N, "cols": C, **res,
            "bf16_bits_are_the_fp32_entrys_rounded": same, "bf16_bits": bit_checksum(o16),
            "time_ratio_bf16_over_fp32": round(res["d_bf16_entry"]["ms_min"] / res["d_fp32_entry"]["ms_min"], 4)}


def probe_model_distance(N, dev):
    from gnn.models import GraphCNNDropEdge

    torch.manual_seed(0)
    model = GraphCNNDropEdge(64, 5, 6, net_size=256, dropedge_seed=7).to(dev).train()
    graph = TypedGraph.synthetic(N, 16.0, 6, seed=1, device=dev)
    V = torch.randn(1, N, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    y = torch.randint(0, 5, (N,), device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]

    def step(act):
        model.train_activation_dtype = act
        model.edge_dropout.reset_calls()
        model.dropout.reset_calls()
        logits = model([V, graph])
        loss = torch.nn.functional.cross_entropy(logits[0], y)
        return logits.detach(), float(loss.detach()), torch.autograd.grad(loss, [p for _, p in named])

    l32, loss32, g32 = step(None)
    l16, loss16, g16 = step(BF16)
    model.train_activation_dtype = None

    def rel(x, y):
        return float((x.double() - y.double()).norm() / y.double().norm())

    return {"tool": "probe_train_bf16", "what": "model training step, train_activation_dtype bfloat16 vs None",
            "nodes": N, "net_size": 256, "logits_rel_fro": rel(l16, l32), "loss": {"fp32": loss32, "bf16": loss16},
            "loss_rel": abs(loss16 - loss32) / abs(loss32),
            "grad_rel_fro": {n: rel(a, b) for (n, _), a, b in zip(named, g16, g32)}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--model-nodes", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "train_bf16_c3.json"))
    a = ap.parse_args()
    if a.rounds < 3 or a.calls < 20:
        ap.error("at least 3 rounds of 20 timed calls")
    dev = torch.device("cuda:0")
    head = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls, "warmup": 3}
    lines = []
    g = TypedGraph.synthetic(a.nodes, 32.0, 6, seed=0, device=dev)
    lines.append(json.dumps({**head, "nodes": a.nodes, "edges": g.nnz, "types": g.num_types,
                             **probe_stack(g, 256, a.rounds, a.calls)}))
    print(lines[-1], flush=True)
    del g
    torch.cuda.empty_cache()
    lines.append(json.dumps({**head, **probe_dropout(a.nodes, 256, a.rounds, a.calls, dev)}))
    print(lines[-1], flush=True)
    torch.cuda.empty_cache()
    lines.append(json.dumps({"device": head["device"], **probe_model_distance(a.model_nodes, dev)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
