"""A/B of the attention forward over bf16 key / value tables
on the GPU, the forms alternating in one process: 3 rounds of 3 warm-ups + 20
calls between device events (tools/probe_train_z16.py's protocol).

Shapes: B = 1, dk = 16, dv = 128 at N = 100 000 and N = 131 072; B = 64,
N = 1024 (pages, key split).  Forms of the forward:
(a) fp32        today's fp32 forward (the per-call split pass and six products)
(b) bf16        the bf16 forward on pre-rounded tables
(c) bf16_round  (b) plus the two .to(bfloat16) passes NodeSelfAtten.kv_dtype adds
and the forward + backward of node_self_attention in forms (a) and (c).
(b) counts as a speed-up only where it beats (a) by more than three times the
larger round-to-round spread.  Each shape also records whether row_max /
row_sum are bitwise and out / o_norm equal to the fp32 entry's on the widened
tables.

--model: GraphCNNDropEdge(4369, 53, 6, 256) on one graph of --model-nodes
(bench.py's model_one_graph_100k), eval forward and Adam train step with
kv_dtype None / bfloat16, and the distance of the kv_dtype = bfloat16 model to
the fp32 model (relative Frobenius norm of logits, loss, parameter gradients;
recorded, not asserted).

--once N: three bf16 forwards at N and nothing else (for a counters-only profiler run).

One JSON line per measurement, all of them written to
profiles/attn_bf16kv.json."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "graph-representation-learning_amd"))
import torch  # noqa: E402

from grl import TypedGraph, _lib  # noqa: E402
from grl.ops import node_attention_forward, node_self_attention  # noqa: E402

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


def faster3(new, old):
    """new beats old by more than three times the larger round-to-round spread."""
    return bool(old["ms_min"] - new["ms_min"] > 3.0 * max(new["spread_ms"], old["spread_ms"]))


def operands(B, N, dk, dv, dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    Q = torch.relu(torch.randn(B, N, dk, device=dev, generator=gen))  # f, g, h are Linear + ReLU outputs
    K = torch.relu(torch.randn(B, N, dk, device=dev, generator=gen))
    H = torch.relu(torch.randn(B, N, dv, device=dev, generator=gen))
    V = torch.randn(B, N, dv, device=dev, generator=gen)
    gamma = torch.randn(dv, device=dev, generator=gen)
    return Q, K, H, V, gamma


def probe_shape(B, N, dk, dv, rounds, calls, dev):
    Q, K, H, V, gamma = operands(B, N, dk, dv, dev)
    K16, H16 = K.to(BF16), H.to(BF16)
    Kw, Hw = K16.float(), H16.float()  # the widened tables: what (a) reads, so that the three forms compute one thing
    lib = _lib.lib()
    if not lib.grl_node_attention_fwd_bf16kv_path(B, N, dk, dv):
        raise RuntimeError("no bf16 path for this shape (attn_x6 = 0?)")
    fwd = {"fp32": lambda: node_attention_forward(Q, Kw, Hw, V, gamma, stats=True),
           "bf16": lambda: node_attention_forward(Q, K16, H16, V, gamma, stats=True),
           "bf16_round": lambda: node_attention_forward(Q, Kw.to(BF16), Hw.to(BF16), V, gamma, stats=True)}
    with torch.no_grad():
        t = rounds_of(fwd, rounds, calls)
        a, b = fwd["fp32"](), fwd["bf16"]()
    leaves = [x.clone().requires_grad_(True) for x in (Q, Kw, Hw, V, gamma)]
    dout = torch.randn(V.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3))

    def fb(round_kv):
        def run():
            for x in leaves:
                x.grad = None
            q, k, h, v, g = leaves
            if round_kv:
                k, h = k.to(BF16), h.to(BF16)
            node_self_attention(q, k, h, v, g).backward(dout)
        return run

    tb = rounds_of({"fp32": fb(False), "bf16_round": fb(True)}, rounds, calls)
    return {"what": "attention forward", "B": B, "N": N, "dk": dk, "dv": dv,
            "row_stats_bits_equal": bool(torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
                                         and torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))),
            "out_onorm_equal": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])),
            "out_onorm_bits_equal": bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
                                         and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))),
            "workspace_bytes": {"fp32": int(lib.grl_node_attention_workspace_size(B, N, dk, dv)),
                                "bf16": int(lib.grl_node_attention_fwd_bf16kv_workspace_size(B, N, dk, dv))},
            "forward": t, "forward_time_ratio_bf16_over_fp32": round(t["bf16"]["ms_min"] / t["fp32"]["ms_min"], 4),
            "forward_bf16_is_a_speed_up": faster3(t["bf16"], t["fp32"]),
            "forward_bf16_round_is_a_speed_up": faster3(t["bf16_round"], t["fp32"]),
            "forward_backward": tb,
            "forward_backward_time_ratio": round(tb["bf16_round"]["ms_min"] / tb["fp32"]["ms_min"], 4),
            "forward_backward_bf16_round_is_a_speed_up": faster3(tb["bf16_round"], tb["fp32"])}


def probe_model(N, rounds, calls, dev):
    from gnn.models import GraphCNNDropEdge

    g = TypedGraph.synthetic(N, 16.0, 6, seed=0, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    V = torch.zeros(1, N, 4369, device=dev)
    V[0].scatter_(1, torch.randint(0, 4365, (N, 7), generator=gen, device=dev), 1.0)
    V[0, :, -4:] = torch.rand(N, 4, generator=gen, device=dev)
    torch.manual_seed(0)
    # a fixed mask seed (as tools/probe_train_z16.py): with reset_calls() two steps draw the same DropEdge and
    # dropout masks, which the record checks (the fp32 model against itself: 0)
    model = GraphCNNDropEdge(4369, 53, 6, 256, dropedge_seed=7).to(dev)
    y = torch.randint(0, 53, (N,), generator=gen, device=dev)
    lossf = torch.nn.CrossEntropyLoss()
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]

    # the distance first (the timed Adam steps below move the parameters)
    def step(kv):
        model.self_atten.kv_dtype = kv
        model.train()
        model.edge_dropout.reset_calls()
        model.dropout.reset_calls()
        logits = model([V, g])
        loss = lossf(logits.reshape(-1, 53), y)
        return logits.detach(), float(loss.detach()), torch.autograd.grad(loss, [p for _, p in named])

    def rel(x, ref):
        return float((x.double() - ref.double()).norm() / ref.double().norm())

    ref, again, got = step(None), step(None), step(BF16)
    same_masks = {"logits_rel_fro": rel(again[0], ref[0]), "loss_rel": abs(again[1] - ref[1]) / abs(ref[1]),
                  "grad_rel_fro_max": max(rel(a, b) for a, b in zip(again[2], ref[2]))}
    del again
    model.eval()
    with torch.no_grad():
        model.self_atten.kv_dtype = None
        ev_ref = model([V, g])
        model.self_atten.kv_dtype = BF16
        ev_got = model([V, g])
    dist = {"fp32_model_to_itself_over_two_steps": same_masks, "train_logits_rel_fro": rel(got[0], ref[0]),
            "eval_logits_rel_fro": rel(ev_got, ev_ref),
            "loss": {"fp32": ref[1], "kv_bf16": got[1]}, "loss_rel": abs(got[1] - ref[1]) / abs(ref[1]),
            "grad_rel_fro": {n: rel(a, b) for (n, _), a, b in zip(named, got[2], ref[2])}}
    del ref, got, ev_ref, ev_got

    def eval_form(kv):
        def run():
            model.self_atten.kv_dtype = kv
            with torch.no_grad():
                model([V, g])
        return run

    model.eval()
    ev = rounds_of({"kv_none": eval_form(None), "kv_bf16": eval_form(BF16)}, rounds, calls)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def train_form(kv):
        def run():
            model.self_atten.kv_dtype = kv
            opt.zero_grad(set_to_none=True)
            lossf(model([V, g]).reshape(-1, 53), y).backward()
            opt.step()
        return run

    model.train()
    tr = rounds_of({"kv_none": train_form(None), "kv_bf16": train_form(BF16)}, rounds, calls)
    model.self_atten.kv_dtype = None
    return {"what": "GraphCNNDropEdge(4369, 53, 6, 256), one graph", "nodes": N, "typed_edges": g.nnz,
            "eval_forward": ev, "eval_kv_bf16_is_a_speed_up": faster3(ev["kv_bf16"], ev["kv_none"]),
            "train_step": tr, "train_kv_bf16_is_a_speed_up": faster3(tr["kv_bf16"], tr["kv_none"]),
            "distance_kv_bf16_to_fp32": dist}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--model", action="store_true", help="also the model's eval forward, train step and distance")
    ap.add_argument("--model-nodes", type=int, default=100_000)
    ap.add_argument("--once", type=int, default=0, metavar="N", help="three bf16 forwards at N nodes and nothing else")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "attn_bf16kv.json"))
    ap.add_argument("--attn-fwd8", type=int, default=1, choices=(0, 1), help="0: 4-wave workgroups in both forwards")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.set_option("attn_fwd8", a.attn_fwd8)
    if a.once:
        Q, K, H, V, gamma = operands(1, a.once, 16, 128, dev)
        K16, H16 = K.to(BF16), H.to(BF16)
        for _ in range(3):
            node_attention_forward(Q, K16, H16, V, gamma, stats=True)
        torch.cuda.synchronize()
        return
    if a.rounds < 3 or a.calls < 20:
        ap.error("at least 3 rounds of 20 timed calls")
    head = {"tool": "probe_attn_bf16kv", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls": a.calls,
            "warmup": 3, "lib": os.path.basename(_lib.LIB_PATH), "attn_fwd8": a.attn_fwd8}
    lines = []

    def emit(rec):
        lines.append(json.dumps({**head, **rec}))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()

    for B, N in ((1, 100_000), (1, 131_072), (64, 1024)):
        emit(probe_shape(B, N, 16, 128, a.rounds, a.calls, dev))
    if a.model:
        emit(probe_model(a.model_nodes, a.rounds, a.calls, dev))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
