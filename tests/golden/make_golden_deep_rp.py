#!/usr/bin/env python
"""Generate tests/golden/deep_rp_model.npz from the REFERENCE's
DeepRPRobustGCN (gnn/models/networks/deep_rp_robust_gcn.py).

Run in the build container only (it needs the reference checkout, as
make_golden.py does):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deep_rp.py

The reduced model DeepRPRobustGCN(64, 7, 6, net_size=32, rp_size=None,
lambda_value=1) under torch.manual_seed(1), on a B = 2, N = 23 batch from
inputs.py with two padded (-100) labels:
  init::<key>          the whole initial state_dict (reference keys)
  eval_logits          eval mode (initial running statistics, lambda 1)
  train0_*             train mode, both dropout rates 0, lambda_value = 0.37:
                       logits, loss, grad::<param>, buf::<BN buffer> after the step
  traindrop_*          as train0, with the engine's DropEdge hash masks
                       (p = 0.2, seed SEED_DROPEDGE, calls 0..3, drop_self)
                       injected at the four dropped layers; feature dropout 0
Every case also runs in float64, and the fp32 reference must be within
1e-5 * max(1, |ref|) of it for every stored array: the tests' 1e-4 then has
a tenfold margin the reference itself respects.  No reference source is copied.
"""
from __future__ import annotations

import copy
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as mg  # noqa: E402  (sets the paths, the logging shims)
import inputs as gi  # noqa: E402
from oracle import dense_ref  # noqa: E402

SEED_INPUTS = range(71, 111)  # tried in order: the first whose fp32 reference run is within FP64_TOL of float64
SEED_DROPEDGE = gi.DROPEDGE["seed"]
P_EDGE = 0.2
B, N, L, F_IN, C, OUT = 2, 23, 6, 64, 32, 7
LAMBDA_TRAIN = 0.37
FP64_TOL = 1e-5


def _import_model():
    mg._install_shims()
    os.makedirs(os.environ["OUTPUT_DIR"], exist_ok=True)
    sys.path.insert(0, mg.REF)
    from gnn.models.networks.deep_rp_robust_gcn import DeepRPRobustGCN
    return DeepRPRobustGCN


class InjectedEdgeDropout(torch.nn.Module):
    """nn.Dropout's arithmetic (input.mul(mask).mul_(scale)) with given masks, one per call."""

    def __init__(self, ms):
        super().__init__()
        self.ms, self.i = ms, 0

    def forward(self, a):
        m = self.ms[self.i]
        self.i += 1
        keep = mg._t((m != 0).astype(np.float32)).to(a.dtype)
        scale = float(m.max()) if (m != 0).any() else 1.0
        return a.mul(keep).mul_(scale)


def _min_batch_variances(model, log):
    """Forward pre-hooks on every BatchNorm1d: the smallest biased batch variance of its (B, C, N) input."""
    hooks = []
    for name, mod in model.named_modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            def hook(m, args, name=name):
                log[name] = float(args[0].detach().double().var(dim=(0, 2), unbiased=False).min())
            hooks.append(mod.register_forward_pre_hook(hook))
    return hooks


def run_case(base, V, A, labels, mode, masks=None, dtype=torch.float32, variances=None):
    """One case on a copy of the initial model: arrays by fixture key."""
    model = copy.deepcopy(base).to(dtype)
    Vt, At = mg._t(V).to(dtype), mg._t(A).to(dtype)
    if mode == "eval":
        model.eval()
        with torch.no_grad():
            return {"eval_logits": model([Vt, At]).numpy()}
    model.train()
    model.dropout.p = 0.0
    model.edge_dropout.p = 0.0
    if masks is not None:
        model.edge_dropout = InjectedEdgeDropout(masks)
    model.lambda_value = LAMBDA_TRAIN
    hooks = _min_batch_variances(model, variances) if variances is not None else []
    logits = model([Vt, At])
    for h in hooks:
        h.remove()
    loss = torch.nn.functional.cross_entropy(logits.transpose(1, 2), torch.from_numpy(labels), ignore_index=-100)
    loss.backward()
    out = {f"{mode}_logits": logits.detach().numpy(), f"{mode}_loss": np.array(loss.item())}
    out.update({f"{mode}_grad::{k}": p.grad.numpy() for k, p in model.named_parameters() if p.grad is not None})
    out.update({f"{mode}_buf::{k}": b.detach().numpy() for k, b in model.named_buffers()})
    return out


def build(DeepRPRobustGCN, seed):
    """The fixture's arrays for one input seed, and the worst fp32-vs-float64 error (None, key, err if over)."""
    A = gi.random_adj_bnln(seed, B, N, L, 3.0)
    V = gi.features(seed + 1, B, N, F_IN)
    labels = gi.rng(seed + 2).integers(0, OUT, size=(B, N))
    labels[1, -2:] = -100  # padded nodes (NumpyPadding's label -100)
    torch.manual_seed(1)
    base = DeepRPRobustGCN(F_IN, OUT, L, net_size=C, rp_size=None, lambda_value=1)
    init = {k: v.detach().clone().numpy() for k, v in base.state_dict().items()}
    masks = [dense_ref.dropedge_weights_pre(A, P_EDGE, SEED_DROPEDGE, c, drop_self=True) for c in range(4)]
    out = {"A": A, "V": V, "labels": labels, "dropedge": np.array([P_EDGE, SEED_DROPEDGE]),
           "lambda_train": np.array(LAMBDA_TRAIN), "seed_inputs": np.array(seed)}
    out.update({f"init::{k}": v for k, v in init.items()})
    worst = 0.0
    for mode, ms in (("eval", None), ("train0", None), ("traindrop", masks)):
        variances = {} if mode != "eval" else None
        got = run_case(base, V, A, labels, mode, ms, torch.float32, variances)
        ref = run_case(base, V, A, labels, mode, ms, torch.float64)
        for k, v in got.items():
            r = np.asarray(ref[k], np.float64)
            err = float(np.abs(np.asarray(v, np.float64) - r).max()) / max(1.0, float(np.abs(r).max()))
            worst = max(worst, err)
            if err > FP64_TOL:
                return None, k, err
        if variances is not None:
            print(f"seed {seed} {mode}: smallest batch variance per BN layer: "
                  + ", ".join(f"{k} {v:.3g}" for k, v in variances.items()))
        out.update(got)
    return out, None, worst


def main():
    DeepRPRobustGCN = _import_model()
    for seed in SEED_INPUTS:
        out, key, err = build(DeepRPRobustGCN, seed)
        if out is not None:
            break
        print(f"seed {seed}: {key}: the fp32 reference is {err:.3e} (relative to max(1, |ref|)) from float64: next seed")
    assert out is not None, "no input seed keeps the fp32 reference within FP64_TOL of float64"
    print(f"seed {seed}: state elements {sum(v.size for k, v in out.items() if k.startswith('init::')):,}; "
          f"fp32 reference vs float64: worst {err:.3e} (cap {FP64_TOL:.0e})")
    path = os.path.join(HERE, "deep_rp_model.npz")
    np.savez_compressed(path, **out)
    print(f"deep_rp_model.npz: {os.path.getsize(path):,} bytes, {len(out)} arrays, "
          f"train0 loss {float(out['train0_loss']):.6f}, traindrop loss {float(out['traindrop_loss']):.6f}")


if __name__ == "__main__":
    main()
