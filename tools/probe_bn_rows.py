"""Diagnostic: batch norm over rows + LeakyReLU (grl_bn_rows_*, DESIGN.md
§4.26) against the reference's torch chain, forms alternating in one process.

Per table [rows, C] (default 1M x 256 and 1M x 512), three forms each for
  new    grl.ops.batchnorm_rows_fwd_train / _bwd / _fwd_eval on the row-major
         table as it lies;
  torch  the reference's chain on a (1, rows, C) tensor: x.permute(0, 2, 1) ->
         nn.BatchNorm1d -> permute back -> F.leaky_relu(0.2), and its autograd
         backward (deep_rp_robust_gcn.py:39-45);
and the statistics pass of the training forward alone, as the training forward
of `new` less the inference form (one apply pass of the same geometry and
bytes as the training forward's third kernel).  torch's backward alone is
likewise a difference: forward + backward less the forward with its graph kept.

Per form: ROUNDS rounds of 3 warm-up and CALLS timed calls between device
events, the forms taking turns, so each form's round-to-round spread is visible
next to the differences (DESIGN.md §4.22's protocol).  A speed-up is called
only where torch's best round exceeds new's by more than three times the
larger of the two spreads (§4.21's rule).  Byte floors: train forward 3 B,
inference 2 B, backward 7 B with B = rows * C * 4, read against the measured
6.29 TB/s float4 copy rate.

--model also times one DeepRPRobustGCN(4369, 45, 6, 256) forward + backward on
a synthetic 100k-node graph.

Prints one JSON line per case and writes them to --out.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graph-representation-learning_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from grl import TypedGraph, _lib  # noqa: E402
from grl.ops import batchnorm_rows_bwd, batchnorm_rows_fwd_eval, batchnorm_rows_fwd_train  # noqa: E402

COPY_TBPS = 6.29  # measured float4 copy rate of the MI355X
EPS, MOM, SLOPE = 1e-5, 0.1, 0.2


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


def probe_table(rows, C, rounds, calls, dev):
    gen = torch.Generator(device=dev).manual_seed(5)
    x = torch.randn(rows, C, device=dev, generator=gen) * 2 + 1
    dy = torch.randn(rows, C, device=dev, generator=gen)
    w = torch.rand(C, device=dev, generator=gen) + 0.5
    b = torch.randn(C, device=dev, generator=gen)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y, mean, invstd = batchnorm_rows_fwd_train(x, w, b, rm, rv, MOM, EPS, SLOPE)
    dx = torch.empty_like(x)
    scratch = torch.empty_like(x)

    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(w), bn.bias.copy_(b)
    x3 = x.view(1, rows, C)

    def torch_fwd():
        return F.leaky_relu(bn(x3.permute(0, 2, 1)).permute(0, 2, 1), negative_slope=SLOPE)

    state = {}

    def torch_fwd_train():
        bn.train()
        with torch.no_grad():
            state["y"] = torch_fwd()

    def torch_eval():
        bn.eval()
        with torch.no_grad():
            state["y"] = torch_fwd()

    def torch_fwd_bwd():
        bn.train()
        xr = x3.detach().requires_grad_(True)
        yr = F.leaky_relu(bn(xr.permute(0, 2, 1)).permute(0, 2, 1), negative_slope=SLOPE)
        yr.backward(dy.view(1, rows, C))
        bn.weight.grad = bn.bias.grad = None

    def torch_fwd_grad():  # the forward with its graph kept: what torch_fwd_bwd spends before the backward starts
        bn.train()
        xr = x3.detach().requires_grad_(True)
        state["yr"] = F.leaky_relu(bn(xr.permute(0, 2, 1)).permute(0, 2, 1), negative_slope=SLOPE)

    forms = {
        "new_fwd_train": lambda: batchnorm_rows_fwd_train(x, w, b, rm, rv, MOM, EPS, SLOPE, out=y),
        "torch_fwd_train": torch_fwd_train,
        "new_eval": lambda: batchnorm_rows_fwd_eval(x, w, b, rm, rv, EPS, SLOPE, out=scratch),
        "torch_eval": torch_eval,
        "new_bwd": lambda: batchnorm_rows_bwd(dy, y, x, w, mean, invstd, SLOPE, out=dx),
        "torch_fwd_plus_bwd": torch_fwd_bwd,
        "torch_fwd_with_graph": torch_fwd_grad,
    }
    t = rounds_of(forms, rounds, calls)
    state.clear()
    B = rows * C * 4
    floors = {"new_fwd_train": 3 * B, "new_eval": 2 * B, "new_bwd": 7 * B}
    out = {"rows": rows, "C": C, "table_bytes": B, "workspace_bytes": int(_lib.lib().grl_bn_rows_workspace_size(rows, C)),
           **t}
    for k, nbytes in floors.items():
        floor_ms = nbytes / (COPY_TBPS * 1e12) * 1e3
        out[k]["floor_bytes"] = nbytes
        out[k]["floor_ms_at_copy_rate"] = round(floor_ms, 4)
        out[k]["floor_fraction"] = round(floor_ms / t[k]["ms_min"], 4)
    # the statistics pass + finalize: the training forward less an apply pass of the same geometry
    out["stats_pass_ms_fwd_train_minus_eval"] = round(t["new_fwd_train"]["ms_min"] - t["new_eval"]["ms_min"], 4)
    out["stats_pass_floor_fraction"] = round((B / (COPY_TBPS * 1e12) * 1e3)
                                             / max(out["stats_pass_ms_fwd_train_minus_eval"], 1e-9), 4)
    torch_bwd = {"ms_min": round(t["torch_fwd_plus_bwd"]["ms_min"] - t["torch_fwd_with_graph"]["ms_min"], 4),
                 "spread_ms": round(max(t["torch_fwd_plus_bwd"]["spread_ms"], t["torch_fwd_with_graph"]["spread_ms"]), 4)}
    out["torch_bwd_as_difference"] = torch_bwd
    pairs = {"fwd_train": ("new_fwd_train", t["torch_fwd_train"]), "eval": ("new_eval", t["torch_eval"]),
             "bwd": ("new_bwd", torch_bwd)}
    for name, (new, ref) in pairs.items():
        gap = ref["ms_min"] - t[new]["ms_min"]
        spread = max(ref["spread_ms"], t[new]["spread_ms"])
        out[f"{name}_gap_ms_torch_minus_new"] = round(gap, 4)
        out[f"{name}_time_ratio_new_over_torch"] = round(t[new]["ms_min"] / max(ref["ms_min"], 1e-9), 4)
        out[f"{name}_speedup_called"] = bool(gap > 3 * spread)
    return out


def probe_model(n_nodes, rounds, calls, dev):
    from gnn.models import DeepRPRobustGCN

    torch.manual_seed(0)
    model = DeepRPRobustGCN(4369, 45, 6, 256).to(dev).train()
    graph = TypedGraph.synthetic(n_nodes, 6.0, 6, seed=1, device=dev)
    gen = torch.Generator(device=dev).manual_seed(2)
    # bag-of-characters rows: about 7 nonzeros of 4369
    V = (torch.rand(1, n_nodes, 4369, device=dev, generator=gen) < 7.0 / 4369).float()
    y = torch.randint(0, 45, (n_nodes,), device=dev, generator=gen)

    def step():
        model.zero_grad(set_to_none=True)
        logits = model([V, graph])
        F.cross_entropy(logits.view(-1, 45), y).backward()

    def fwd():
        with torch.no_grad():
            model([V, graph])

    t = rounds_of({"fwd_bwd_train": step, "fwd_train_no_grad": fwd}, rounds, calls)
    return {"model": "DeepRPRobustGCN(4369, 45, 6, 256)", "nodes": n_nodes, "edges": int(graph.nnz), **t}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--cols", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--model", type=int, default=0, metavar="NODES", help="also time the model at this many nodes")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "bn_rows.json"))
    a = ap.parse_args()
    if a.rounds < 3 or a.calls < 20:
        ap.error("at least 3 rounds of 20 timed calls")
    dev = torch.device("cuda:0")
    head = {"tool": "probe_bn_rows", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls,
            "warmup": 3, "copy_rate_tbps": COPY_TBPS}
    lines = []
    for C in a.cols:
        lines.append(json.dumps({**head, "case": f"table_{a.rows}x{C}", **probe_table(a.rows, C, a.rounds, a.calls, dev)}))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if a.model:
        lines.append(json.dumps({**head, "case": "model_fwd_bwd", **probe_model(a.model, a.rounds, a.calls, dev)}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
