"""GPU: bench.py's one-GPU runs.

  * a plain run (`--gpus 1 --steps K --warmup W`) times K steps and prints
    the headline line alone: nothing that takes runs of its own (CPU baseline
    and parity, training-mode aggregation, extras) is in it;
  * `--dump-outputs DIR` writes what the last timed step computed -- here
    checked bitwise against the same aggregation computed in this process
    from the same seeds -- and two runs of the same arguments write the same
    bytes;
  * `--full` brings back the CPU baseline with its bitwise parity check and
    the DropEdge training-mode forward + backward.
The shapes are small (20k and 3k nodes): one over the dump's 32 MiB so that
the seeded row sample is taken, one under it so that Z is written whole."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from grl import TypedGraph
from grl.ops import spmm_forward

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "parity", "dropedge_train_p0.3", "extras", "C4_one_gpu", "node_order_ab")


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + args, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _expected_z(n, deg, dim):
    """The timed path's result from its seeds: graph seed 0, X ~ N(0,1) from
    a device generator seeded 1 + rank."""
    g = TypedGraph.synthetic(n, deg, 6, kind="er", seed=0, device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    X = torch.randn(n, dim, generator=gen, device=DEV, dtype=torch.float32)
    return spmm_forward(X, g).cpu().numpy()


def test_plain_run_is_the_headline_alone_and_dumps_its_last_step(tmp_path):
    n, deg, dim = 20_000, 16.0, 256
    args = ["--workload", "C2", "--nodes-per-gpu", str(n), "--steps", "3", "--warmup", "1"]
    out = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    for k in LINE_KEYS:
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "edges/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["config"]["edges_total"] / (out["ms_per_step"] * 1e-3), rel=1e-9)
    assert out["roofline"]["launches"] == dict(out["roofline"]["launches"], timed=3, warmup=1, other=0)
    for k in FULL_ONLY:
        assert k not in out, k
    assert sorted(os.listdir(tmp_path / "a")) == ["Z.npy"]
    z = np.load(tmp_path / "a" / "Z.npy")
    ref = _expected_z(n, deg, dim)
    keep = (32 << 20) // (ref.shape[1] * 4)
    assert keep < n  # the sampled form
    rows = np.sort(np.random.default_rng(0).choice(n, size=keep, replace=False))
    assert z.dtype == np.float32 and z.shape == (keep, 7 * dim) and z.nbytes <= (64 << 20)
    assert np.array_equal(z, ref[rows])
    # the same arguments again: the same inputs, the same bytes
    _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    assert (tmp_path / "a" / "Z.npy").read_bytes() == (tmp_path / "b" / "Z.npy").read_bytes()


def test_full_run_adds_the_cpu_baseline_parity_and_training_mode(tmp_path):
    n, deg, dim = 3000, 32.0, 64
    out = _bench(["--nodes-per-gpu", str(n), "--dim", str(dim), "--steps", "2", "--warmup", "1", "--full",
                  "--cpu-seconds", "0.2", "--dump-outputs", str(tmp_path)])
    for k in LINE_KEYS:
        assert k in out, k
    assert out["config"]["workload"].startswith("C3") and out["steps"] == 2
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "edges/s"
    assert out["parity"]["bitwise_equal"] is True and out["parity"]["rows_checked"] == n
    assert out["dropedge_train_p0.3"]["fwd_ms"] > 0 and out["dropedge_train_p0.3"]["bwd_ms"] > 0
    assert out["roofline"]["launches"]["other"] == 5
    z = np.load(tmp_path / "Z.npy")  # under 32 MiB: written whole
    assert z.dtype == np.float32 and np.array_equal(z, _expected_z(n, deg, dim))
