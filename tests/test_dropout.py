"""Dropout in the bodies on the device: ops.dropout_add (kpgnn_dropout_fwd / _bwd, csrc/dropout.hip) at every site where the
three bodies drop out (models/GNNs.py: after the layers, inside the virtual-node update, after the jumping-knowledge
projection), against the same body with the masks of ops.dropout_mask applied by framework ops; evaluation mode; and what
counter-based masks make possible: a captured training step that draws fresh masks on every replay, and a dataset.StaticBatch
whose masks are those of the exact-shape batch."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, L, H = 4, 4, 32
P = 0.5
SEED = 20240607


def _dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _native_route_on():
    """The native route is opt-in (ops.set_native_dropout): on for every test here, restored afterwards."""
    from kp_gnn_amd import ops
    prev = ops.set_native_dropout(True)
    yield
    ops.set_native_dropout(prev)


def _model(model_name, drop, JK="concat", seed=3):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(seed)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK=JK, norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=True, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=drop)
    with torch.no_grad():
        gnn.virtualnode_embedding.weight.normal_(0.0, 0.5)
    return B.GraphRegression(gnn, "sum")


def _spy(monkeypatch):
    from kp_gnn_amd import _lib
    launches = []
    real = _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    return launches


def _drops(launches):
    return [n for n in launches if n.startswith("kpgnn_dropout_")]


def _train_step(model, b):
    model.zero_grad(set_to_none=True)
    score = model(b)
    loss = (score.squeeze() - b.y.squeeze()).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    got = {n: (torch.zeros_like(q) if q.grad is None else q.grad.clone()) for n, q in model.named_parameters() if q.requires_grad}
    return score.detach().clone(), loss.detach().clone(), got


# ------------------------------------------------------------------------------------------------ 1. native against emulated
@pytest.mark.parametrize("model_name,JK", [("KPGINPlus", "concat"), ("KPGIN", "last"), ("KPGINPrime", "concat")])
def test_native_equals_the_emulated_masks(model_name, JK, monkeypatch):
    """drop_prob = 0.5, residual, virtual node: the native run against a run in which body.dropout_add is a test-local function
    that counts its calls from 0 after dropout_seed, takes its masks from ops.dropout_mask and computes
    where(mask, x * scale, 0) + residual with framework ops.  Score and loss within rtol 2e-4 / atol 2e-5, every parameter
    gradient within rtol 2e-3 / atol 5e-5 (the tolerances of test_bodies_match_reference_goldens); the dropped fraction of the
    first site's mask within 5 binomial standard deviations of p."""
    from kp_gnn_amd import body, ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model(model_name, P, JK).to(dev).train()
    b = synthetic_zinc_batch(48, seed0=11, K=K).to(dev)
    b.build_csr()
    launches = _spy(monkeypatch)
    ops.dropout_seed(SEED, dev)
    native = _train_step(model, b)
    sites = launches.count("kpgnn_dropout_fwd")
    # L - 1 layer sites, L - 1 virtual-node updates, 1 after the projection.  GNN / GNNPlus drop out after every layer but the
    # last.  GNNPrime's rule is `l < num_l1_layer or l != num_layer - 1`: with num_l1_layer = 1 < L the first clause only
    # covers layer 0, which the second covers as well, so it is the same L - 1 layers (it would be L with num_l1_layer == L).
    assert sites == 2 * (L - 1) + 1 and launches.count("kpgnn_dropout_bwd") == sites, _drops(launches)
    assert int(ops.dropout_state(dev)[1]) == sites
    masks = []

    def emulated(x, p, training, residual=None):
        assert training and p == P
        mask = ops.dropout_mask(x.shape, p, SEED, len(masks), x.device)
        masks.append(mask)
        out = torch.where(mask, x * ops.dropout_params(p)[1], torch.zeros_like(x))
        return out if residual is None else out + residual

    monkeypatch.setattr(body, "dropout_add", emulated)
    del launches[:]
    emu = _train_step(model, b)
    assert len(masks) == sites and not _drops([n for n in launches if n != "kpgnn_dropout_mask"])
    assert torch.allclose(native[0], emu[0], rtol=2e-4, atol=2e-5), float((native[0] - emu[0]).abs().max())
    assert torch.allclose(native[1], emu[1], rtol=2e-4, atol=2e-5), (float(native[1]), float(emu[1]))
    for n in emu[2]:
        err = float((native[2][n] - emu[2][n]).abs().max())
        assert torch.allclose(native[2][n], emu[2][n], rtol=2e-3, atol=5e-5), (n, err)
    assert any(float(g.abs().max()) > 0 for g in native[2].values())
    first = masks[0]
    n = first.numel()
    assert tuple(first.shape) == (b.num_nodes, H)
    dropped = 1.0 - float(first.float().mean())
    assert abs(dropped - P) <= 5 * (P * (1 - P) / n) ** 0.5, (dropped, n)


# ------------------------------------------------------------------------------------------------ 2. evaluation mode
def test_evaluation_mode_ignores_drop_prob(monkeypatch):
    """model.eval() under no_grad: drop_prob = 0.5 gives the bits of the same weights built with drop_prob = 0.0, and no
    kpgnn_dropout_* launch is made."""
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    with_p, without = _model("KPGINPlus", P).to(dev).eval(), _model("KPGINPlus", 0.0).to(dev).eval()
    without.load_state_dict(with_p.state_dict())
    b = synthetic_zinc_batch(48, seed0=11, K=K).to(dev)
    b.build_csr()
    launches = _spy(monkeypatch)
    with torch.no_grad():
        got, ref = with_p(b), without(b)
    torch.cuda.synchronize()
    assert launches and not _drops(launches)
    assert torch.equal(got, ref)


# ------------------------------------------------------------------------------------------------ 3. capture
def _dataset(n, seed0=21):
    from test_dataset import molecules
    from kp_gnn_amd.dataset import KHopDataset
    raw = molecules(n, seed0=seed0)
    args = (K, 50, 6, 3, 50, 50, "spd")
    return raw, args, KHopDataset.from_collated(raw.collated(args), raw.node_ptr, _dev())


def _step(model, batch):
    from kp_gnn_amd.ops_dense import regression_loss_and_grad
    score = model(batch)
    loss, dscore = regression_loss_and_grad(score, batch.y, "l1")
    params = [p for p in model.parameters() if p.requires_grad]
    grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
    return loss, score, [g if g is None else g.clone() for g in grads]


def _keep(res):
    loss, score, grads = res
    return loss.clone(), score.detach().clone(), [g if g is None else g.clone() for g in grads]


def _vn_norm_params(model):
    """mlp_virtualnode_list.*.{1,4}.{weight,bias}: finished from fp64 column sums that blocks add with atomics."""
    return {n for n, _ in model.named_parameters() if "mlp_virtualnode_list" in n and n.split(".")[-2] in ("1", "4")}


def test_captured_step_draws_the_eager_masks_on_every_replay():
    """Seed, two eager training steps: their scores differ (the call ids went on).  Seed again, ONE captured step replayed
    twice: replay 1 is eager step 1 and replay 2 eager step 2 - score and loss bit for bit, gradients under the rules of
    tests/test_virtual_node.py::test_training_step_is_captured_and_replays_to_the_eager_bits (bitwise, the BatchNorm
    gamma / beta gradients of the virtual-node MLPs to fp64-sum accuracy).  The call id never travels through a kernel
    argument, or both replays would repeat the mask of the capture."""
    from kp_gnn_amd import ops
    dev = _dev()
    raw, args, ds = _dataset(64, seed0=5)
    model = _model("KPGINPlus", P).to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    b = ds.collate([9, 3, 60, 21, 22, 23, 0, 63, 11, 40, 41, 5])
    assert b.num_graphs == 12
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    eager = []
    with torch.cuda.stream(side):
        _step(model, b)                              # warms the caches that sync (graph pointer, index range checks)
        ops.dropout_seed(SEED, dev)
        for _ in range(2):
            model.load_state_dict(sd)
            eager.append(_keep(_step(model, b)))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    sites = 2 * (L - 1) + 1
    assert int(ops.dropout_state(dev)[1]) == 2 * sites
    assert not torch.equal(eager[0][1], eager[1][1])
    model.load_state_dict(sd)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(model, b)
    ops.dropout_seed(SEED, dev)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    loose = _vn_norm_params(model)
    assert len(loose) == 4 * (L - 1)
    for i in range(2):
        model.load_state_dict(sd)
        graph.replay()
        torch.cuda.synchronize()
        loss_e, score_e, grads_e = eager[i]
        assert torch.equal(out[1].detach(), score_e) and torch.equal(out[0], loss_e), f"replay {i + 1}"
        for n, ge, gg in zip(names, grads_e, out[2]):
            assert (ge is None) == (gg is None), n
            if ge is None:
                continue
            if n in loose:
                assert float((ge - gg).abs().max()) <= 1e-6 * float(ge.abs().max()) + 1e-12, (i, n, float((ge - gg).abs().max()))
            else:
                assert torch.equal(ge, gg), (i, n, float((ge - gg).abs().max()))
    assert int(ops.dropout_state(dev)[1]) == 2 * sites


# ------------------------------------------------------------------------------------------------ 4. static batch
def test_static_batch_equals_exact_shapes_with_dropout():
    """tests/test_dataset.py::test_static_batch_dynamic_rows_equal_exact_shapes for a body that drops out (96 graphs, three id
    sets out of 400 molecules, the capacity above every live count): with the same seed the exact-shape eager step, the static
    batch run eagerly under sb.dynamic() and ONE captured graph replayed on all three agree under that test's tolerances - the
    mask of a row does not depend on how many rows the buffers have."""
    from kp_gnn_amd import ops
    dev = _dev()
    Bsz = 96
    raw, args, ds = _dataset(400)
    model = _model("KPGINPlus", P, seed=0).to(dev).train()
    sb = ds.static_batch(Bsz)
    assert sb.N_cap > int(ds.h_nodes.mean() * Bsz)
    rng = np.random.default_rng(3)
    id_sets = [rng.permutation(400)[:Bsz] for _ in range(3)]
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def reset():
        model.load_state_dict(sd)
        ops.dropout_seed(SEED, dev)

    def check(got, ref, what):
        (l0, s0, g0), (l1, s1, g1) = got, ref
        assert torch.allclose(s0, s1, rtol=2e-5, atol=2e-5), (what, float((s0 - s1).abs().max()))
        assert abs(float(l0) - float(l1)) <= 2e-5 * max(1.0, abs(float(l1))), what
        gscale = max(float(g.abs().max()) for g in g1 if g is not None)
        for a, b in zip(g0, g1):
            assert (a is None) == (b is None), what
            if a is not None:
                tol = 1e-4 * max(float(b.abs().max()), 0.05 * gscale) + 1e-7
                assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)

    refs = []
    for ids in id_sets:
        reset()
        refs.append(_keep(_step(model, ds.collate(ids))))
    with sb.dynamic():
        for ids, ref in zip(id_sets, refs):
            reset()
            sb.stage(ids)
            sb.launch_collate()
            l, s_, g = _step(model, sb.batch)
            assert sb.live[0] < sb.N_cap
            check((l, s_.detach(), g), ref, "eager static batch")
        del l, s_, g
        reset()
        sb.stage(id_sets[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sb.launch_collate()
            _step(model, sb.batch)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sb.launch_collate()
            out = _step(model, sb.batch)
    for ids, ref in zip(id_sets, refs):
        reset()
        sb.stage(ids)
        assert sb.live[0] < sb.N_cap
        graph.replay()
        torch.cuda.synchronize()
        check((out[0], out[1].detach(), out[2]), ref, "replayed static batch")


# ------------------------------------------------------------------------------------------------ 5. the switch
def test_switch_off_runs_the_framework_modules(monkeypatch):
    from kp_gnn_amd import ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model("KPGINPlus", P).to(dev).train()
    b = synthetic_zinc_batch(12, seed0=11, K=K).to(dev)
    b.build_csr()
    gnn = model.embedding_model
    module_calls = []
    hooks = [m.register_forward_hook(lambda mod, a, o: module_calls.append(mod)) for m in (gnn.dropout, gnn.output_proj[2])]
    launches = _spy(monkeypatch)
    assert ops.native_dropout() is True
    prev = ops.set_native_dropout(False)
    try:
        assert prev is True and ops.native_dropout() is False
        score, loss, grads = _train_step(model, b)
        assert launches and not _drops(launches)
        assert len(module_calls) == 2 * (L - 1) + 1
        assert bool(torch.isfinite(score).all())
        del launches[:], module_calls[:]
        ops.set_native_dropout(True)
        _train_step(model, b)
        assert launches.count("kpgnn_dropout_fwd") == 2 * (L - 1) + 1 and not module_calls
    finally:
        ops.set_native_dropout(prev)
        for h in hooks:
            h.remove()
