"""CPU: DeepRPRobustGCN's public surface -- the registry entry, the
reference's state_dict (keys, order, shapes and torch.manual_seed values,
against tests/golden/deep_rp_model.npz), lambda_value as a property over a
non-persistent buffer, and the refusals: CPU tensors (the engine has no CPU
path) and node-range shards."""
import numpy as np
import pytest
import torch

from gnn import models
from gnn.models import DeepRPRobustGCN
from gnn.models.base_network import BaseNetwork
from gnn.models.networks.deep_rp_robust_gcn import EmbeddingBlock, GCNBlock, RanPACLayer
from grl import GrlError
from grl.dist import ShardedGraph
from grl.ops import batchnorm_rows

ARGS = {"input_dim": 64, "output_dim": 7, "num_edges": 6, "net_size": 32, "rp_size": None, "lambda_value": 1}


def _model():
    torch.manual_seed(1)
    return DeepRPRobustGCN(**ARGS)


def test_registry_builds_it_from_a_config():
    assert "DeepRPRobustGCN" in models.__all__
    torch.manual_seed(1)
    model = BaseNetwork._from_config({"type": "DeepRPRobustGCN", "args": dict(ARGS)})
    assert isinstance(model, DeepRPRobustGCN) and model.net_size == 32 and model.rp_size is None
    with pytest.raises(TypeError, match="Check `args` fields"):
        BaseNetwork._from_config({"type": "DeepRPRobustGCN", "args": {"input_dim": 64, "no_such_arg": 1}})
    with pytest.raises(KeyError):
        BaseNetwork._from_config({"type": "DeepRPGCN", "args": {}})  # not built


def test_defaults_are_the_references():
    import inspect

    sig = inspect.signature(DeepRPRobustGCN.__init__).parameters
    assert list(sig)[1:] == ["input_dim", "output_dim", "num_edges", "net_size", "use_attention", "rp_size",
                             "lambda_value", "dropedge_seed"]
    assert (sig["net_size"].default, sig["use_attention"].default, sig["rp_size"].default,
            sig["lambda_value"].default, sig["dropedge_seed"].default) == (256, True, 10000, 0.01, None)


def test_state_dict_is_the_references(golden):
    g = golden("deep_rp_model.npz")
    want = [k[len("init::"):] for k in g if k.startswith("init::")]
    sd = _model().state_dict()
    assert list(sd) == want  # keys and creation order
    for k, v in sd.items():
        np.testing.assert_array_equal(v.numpy(), g[f"init::{k}"], err_msg=k)  # shapes, init RNG use
    for blk in ("emb1", "emb2") + tuple(f"gcn{i}" for i in range(1, 10)):
        for leaf in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
            assert f"{blk}.bn.{leaf}" in sd


def test_modules_are_the_references():
    m = _model()
    assert isinstance(m.emb1, EmbeddingBlock) and isinstance(m.emb1.emb, torch.nn.Linear)
    assert all(isinstance(getattr(m, f"gcn{i}"), GCNBlock) for i in range(1, 10))
    assert all(type(getattr(m, f"gcn{i}").bn) is torch.nn.BatchNorm1d for i in range(1, 10))
    assert type(m.emb2.bn) is torch.nn.BatchNorm1d
    assert isinstance(m.rp_embed2, RanPACLayer) and not m.rp_embed2.projection.weight.requires_grad
    assert m.gcn3.gcn.F == 64 and m.gcn6.gcn.F == 64 and m.emb2.emb.in_features == 64
    assert m.self_atten is not None and DeepRPRobustGCN(8, 2, 6, net_size=8, use_attention=False).self_atten is not None
    assert (m.dropout.p, m.edge_dropout.p) == (0.3, 0.2)
    assert not hasattr(m, "activation_dtype") and not hasattr(m, "train_activation_dtype")


def test_lambda_value_is_a_property_over_a_buffer_outside_the_state_dict(golden):
    m = _model()
    keys = list(m.state_dict())
    assert m.lambda_value == 1.0 and float(m._lambda) == 1.0
    m.lambda_value = 0.37  # what KVProcedure does every step
    assert m.lambda_value == 0.37 and float(m._lambda) == np.float32(0.37)
    assert list(m.state_dict()) == keys and not any("lambda" in k for k in keys)
    assert "_lambda" in dict(m.named_buffers())
    # a reference-keyed checkpoint loads strictly, and a checkpoint of this model has the reference's keys
    g = golden("deep_rp_model.npz")
    sd = {k[len("init::"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("init::")}
    m.load_state_dict(sd, strict=True)
    assert m.lambda_value == 0.37


def test_cpu_tensors_are_refused():
    x = torch.randn(6, 8)
    with pytest.raises(GrlError, match="ROCm device tensor"):
        batchnorm_rows(x, None, None, None, None, True)
    with pytest.raises(GrlError, match="ROCm device tensor"):
        batchnorm_rows(x, None, None, torch.zeros(8), torch.ones(8), False)
    m = _model()
    V = torch.randn(1, 5, 64)
    A = torch.zeros(1, 5, 6, 5)
    with pytest.raises(GrlError, match="ROCm device tensor"):
        m([V, A])


def test_a_node_range_shard_is_refused():
    m = _model()
    shard = object.__new__(ShardedGraph)  # the type is what is looked at: nothing of the shard is touched
    with pytest.raises(ValueError, match="all-reduce"):
        m([torch.randn(1, 5, 64), shard])
    with pytest.raises(ValueError, match="all-reduce"):
        m.to_graph(shard)
