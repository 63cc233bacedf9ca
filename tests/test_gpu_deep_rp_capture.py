"""GPU: a DeepRPRobustGCN training step (forward, cross-entropy, backward,
clip, capturable Adam) captured as ONE HIP graph equals the eager step -- the
pattern of tests/test_gpu_graph_capture.py::test_captured_train_step_equals_eager.
lambda_value, which the training procedure reassigns every step, is reassigned
between replays on both twins: the captured step reads it from its device
buffer, not a float baked in at capture.  The BatchNorm buffers (running
statistics, num_batches_tracked) advance inside the graph."""
import copy

import pytest
import torch

from gnn.models import DeepRPRobustGCN
from test_gpu_graph_capture import _batch, _capture, _step

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_captured_train_step_equals_eager():
    V, A, y = _batch()
    torch.manual_seed(0)
    model = DeepRPRobustGCN(64, 15, 6, net_size=32, lambda_value=0.5, dropedge_seed=11).to(DEV)
    model.dropout.p = 0.0
    model.train()
    ref = copy.deepcopy(model)
    graph = model.to_graph(A)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    opt_r = torch.optim.Adam(ref.parameters(), lr=1e-3, capturable=True)
    hg, static_loss = _capture(model, opt, V, graph, y, before=model.edge_dropout.reset_calls)
    for _ in range(3):  # the eager twin takes the same warm-up steps
        ref.edge_dropout.reset_calls()
        opt_r.zero_grad(set_to_none=True)
        _step(ref, opt_r, V, graph, y)
    losses = []
    for i, lam in enumerate((0.5, 0.9, 0.1, 0.1, 1.3)):
        model.lambda_value = lam
        ref.lambda_value = lam
        hg.replay()
        ref.edge_dropout.reset_calls()
        opt_r.zero_grad(set_to_none=True)
        loss_r = _step(ref, opt_r, V, graph, y)
        torch.cuda.synchronize()
        torch.testing.assert_close(static_loss, loss_r, rtol=1e-6, atol=1e-6, msg=f"replay {i}")
        for (n, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
            torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-6, msg=f"replay {i}: {n}")
        for (n, p), (_, q) in zip(model.named_buffers(), ref.named_buffers()):
            torch.testing.assert_close(p, q, rtol=1e-6, atol=1e-6, msg=f"replay {i}: buffer {n}")
        losses.append(float(static_loss))
    assert int(model.gcn9.bn.num_batches_tracked) == 3 + 5
    # the replays saw the new lambdas: a step with lambda baked in at 0.5 would not follow the eager twin, and the
    # loss moves with it
    assert len(set(losses)) == len(losses)
