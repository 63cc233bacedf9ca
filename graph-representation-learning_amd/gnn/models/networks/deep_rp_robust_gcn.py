"""DeepRPRobustGCN on the MI355X engine (drop-in for
gnn/models/networks/deep_rp_robust_gcn.py, the model the reference's
scripts/demo_training.py trains).

Forward (reference :110-168):
    emb1 -> gcn1 -> gcn2 -> gcn3(cat[g1, g2], DropEdge) -> Dropout
         -> gcn4 -> gcn5 -> gcn6(cat[g4, g5], DropEdge) -> Dropout
         -> gcn7 -> gcn8(DropEdge) -> gcn9(DropEdge) -> Dropout
         -> emb2(cat[g8, g9]) -> random projection * lambda -> LeakyReLU
         -> NodeSelfAtten -> Dropout -> classifier
Every GCNBlock is GraphConv -> BatchNorm1d over all B*N rows per channel ->
LeakyReLU(0.2), every EmbeddingBlock Linear -> BatchNorm1d -> LeakyReLU(0.2).
The reference permutes to (B, C, N) around nn.BatchNorm1d; here the norm and
its activation run on the row-major table as it lies (grl.ops.batchnorm_rows:
grl_bn_rows_fwd_train / _bwd / _fwd_eval), reading the parameters and running
buffers of a real nn.BatchNorm1d, so module names, state_dict keys, parameter
shapes, creation order and init RNG use are the reference's: checkpoints load
both ways and torch.manual_seed reproduces its weights bit for bit.

Not here: node-range shards (batch statistics over shards need an all-reduce;
a grl.dist.ShardedGraph raises ValueError) and bfloat16 tables.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from gnn.models.base_network import BaseNetwork
from gnn.models.networks.drop_robust_gcn import BAG_LINEAR_MAX_C, EdgeDropout, FeatureDropout
from gnn.models.networks.robust_gcn import GraphConv, NodeSelfAtten, apply_linear
from grl import TypedGraph
from grl.dist import ShardedGraph
from grl.ops import bag_linear, batchnorm_rows

NEGATIVE_SLOPE = 0.2


def bn_leaky(bn: nn.BatchNorm1d, x: torch.Tensor) -> torch.Tensor:
    """bn over x's last axis (statistics over all rows) then LeakyReLU(0.2):
    x.permute(0, 2, 1) -> bn -> permute back -> F.leaky_relu of the reference
    (:41-44, :59-62), as one grl.ops.batchnorm_rows node on bn's own
    parameters and buffers.  num_batches_tracked counts on the device, as
    nn.BatchNorm1d's forward does."""
    if bn.momentum is None:
        raise ValueError("bn_leaky: nn.BatchNorm1d(momentum=None) (a cumulative average) is not supported")
    training = bn.training or not bn.track_running_stats
    if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    return batchnorm_rows(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps,
                          NEGATIVE_SLOPE)


class RanPACLayer(nn.Module):
    """Frozen Gaussian random projection scaled by sqrt(output_dim) * lambda,
    times the forward's lambda, then LeakyReLU(0.2) (deep_rp_robust_gcn.py:12-27)."""

    def __init__(self, input_dim: int, output_dim: int, lambda_value):
        super().__init__()
        self.projection = nn.Linear(input_dim, output_dim, bias=False)
        for p in self.projection.parameters():
            p.requires_grad = False
        nn.init.normal_(self.projection.weight, mean=0, std=1.0)
        self.projection.weight *= (np.sqrt(output_dim) * lambda_value)

    def forward(self, x: torch.Tensor, lambda_value=1) -> torch.Tensor:
        """lambda_value: a number, or a 1-element tensor read on the device."""
        return F.leaky_relu(apply_linear(self.projection, x) * lambda_value, negative_slope=NEGATIVE_SLOPE)


class GCNBlock(nn.Module):
    """GraphConv, BatchNorm over node rows, LeakyReLU (deep_rp_robust_gcn.py:30-45)."""

    def __init__(self, in_channels: int, out_channels: int, num_edges: int):
        super().__init__()
        self.gcn = GraphConv(in_channels, out_channels, num_edges)
        self.bn = nn.BatchNorm1d(out_channels)

    def forward(self, x: torch.Tensor, A, preprocess_A: bool = True) -> torch.Tensor:
        """A: a TypedGraph (DropEdge-tagged or not), or dense as GraphConv.forward takes it."""
        return bn_leaky(self.bn, self.gcn.propagate(x, self.gcn._graph(A, preprocess_A), relu=False))


class EmbeddingBlock(nn.Module):
    """Linear, BatchNorm over node rows, LeakyReLU (deep_rp_robust_gcn.py:48-63)."""

    def __init__(self, in_channels: int, out_channels: int):
        super().__init__()
        self.emb = nn.Linear(in_channels, out_channels)
        self.bn = nn.BatchNorm1d(out_channels)

    def forward(self, x: torch.Tensor, sparse: bool = False) -> torch.Tensor:
        """sparse: x holds bag-of-characters rows (a few nonzeros of thousands):
        the linear runs as a sparse-row gather (grl_bag_linear_fwd) where one
        output row fits a wave's registers."""
        if sparse and x.is_cuda and self.emb.out_features <= BAG_LINEAR_MAX_C:
            h = bag_linear(x.float(), self.emb.weight, self.emb.bias, relu=False)
        else:
            h = apply_linear(self.emb, x)
        return bn_leaky(self.bn, h)


class DeepRPRobustGCN(BaseNetwork):
    """Deep robust GCN with a random projection layer.

    `lambda_value` is a property: the training procedure assigns it every step
    (kv_procedure.py:286) and the forward multiplies by it, so the value lives
    in a one-element device buffer (non-persistent: no state_dict key) that
    the setter fills.  A training step captured into a HIP graph reads the
    current value on every replay.
    `dropedge_seed` (additive): a fixed seed for the DropEdge and feature
    dropout hashes, calls numbered from reset_calls() -- parity tests."""

    def __init__(self, input_dim: int, output_dim: int, num_edges: int, net_size: int = 256,
                 use_attention: bool = True, rp_size=10000, lambda_value: float = 0.01,
                 dropedge_seed: Optional[int] = None):
        super().__init__()
        self.output_dim = output_dim
        self.net_size = net_size
        self.rp_size = rp_size
        self.register_buffer("_lambda", torch.empty(1, dtype=torch.float32), persistent=False)
        self.lambda_value = lambda_value
        self.use_attention = use_attention
        # emb1's input is a bag-of-characters row: a sparse-row gather; False = the dense linear
        self.sparse_emb1 = True

        self.dropout = FeatureDropout(p=0.3, seed=dropedge_seed)
        self.edge_dropout = EdgeDropout(p=0.2, seed=dropedge_seed)

        self.emb1 = EmbeddingBlock(input_dim, self.net_size)
        self.gcn1 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.gcn2 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.gcn3 = GCNBlock(self.net_size * 2, self.net_size, num_edges)
        self.gcn4 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.gcn5 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.gcn6 = GCNBlock(self.net_size * 2, self.net_size, num_edges)
        self.gcn7 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.gcn8 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.gcn9 = GCNBlock(self.net_size, self.net_size, num_edges)
        self.emb2 = EmbeddingBlock(self.net_size * 2, self.net_size)
        self.rp_embed2 = RanPACLayer(self.net_size, self.net_size, 1)
        self.self_atten = NodeSelfAtten(self.net_size)  # built whatever use_attention says, as in the reference (:105)
        self.classifier = nn.Linear(self.net_size, output_dim)

    @property
    def lambda_value(self) -> float:
        return self._lambda_host

    @lambda_value.setter
    def lambda_value(self, value) -> None:
        self._lambda_host = float(value)
        with torch.no_grad():
            self._lambda.fill_(self._lambda_host)

    def to_graph(self, A) -> TypedGraph:
        """Collate-layout dense A (B, N, L, N) -> TypedGraph on the model's device; a TypedGraph as is."""
        if isinstance(A, ShardedGraph):
            raise ValueError("DeepRPRobustGCN does not run on a node-range shard: its batch statistics over the "
                             "shards' rows would need an all-reduce, which is not built")
        if isinstance(A, TypedGraph):
            return A
        dev = self.classifier.weight.device
        return TypedGraph.from_dense(A if A.device == dev else A.to(dev), layout="bnln")

    def forward(self, inputs, efficient_mode: bool = True):
        V, A = inputs
        graph = self.to_graph(A)
        embedding = self.emb1(V, sparse=self.sparse_emb1)
        self.dropout.begin_forward(V.device, None, V.numel() // max(V.shape[-1], 1))
        # efficient_mode=True: the edge dropout covers the identity block of A_pre (:118, :132)
        ds = bool(efficient_mode)
        plain = graph.with_dropedge(None)
        g1 = self.gcn1(embedding, plain)
        g2 = self.gcn2(g1, plain)
        g3 = self.dropout(self.gcn3(torch.cat([g1, g2], dim=-1), self.edge_dropout(graph, ds)))
        g4 = self.gcn4(g3, plain)
        g5 = self.gcn5(g4, plain)
        g6 = self.dropout(self.gcn6(torch.cat([g4, g5], dim=-1), self.edge_dropout(graph, ds)))
        g7 = self.gcn7(g6, plain)
        g8 = self.gcn8(g7, self.edge_dropout(graph, ds))
        g9 = self.dropout(self.gcn9(g8, self.edge_dropout(graph, ds)))
        feats = self.emb2(torch.cat([g8, g9], dim=-1))
        feats = self.rp_embed2(feats, self._lambda)
        feats = self.self_atten(feats)
        feats = self.dropout(feats)
        return apply_linear(self.classifier, feats)
