"""norm_scope="graph" of the bodies on kpgnn_graph_norm_fwd / _bwd (csrc/body_norm_graph.hip) through ops.body_norm: the native
route against the framework per-graph expression on the same device, which launches a body makes, the evaluation forward, a
dataset.StaticBatch under dynamic_rows, a captured step replayed on two id sets, and a graph's bits in a batch of 1 and of 7.

Reference: tests/graph_norm_ref.py (tests/norm_ref.py on each graph's rows)."""
import argparse

import numpy as np
import pytest
import torch

import graph_norm_ref as GR
import norm_ref as NR
import parity_f64 as PF

pytestmark = pytest.mark.gpu

RTOL, ATOL = PF.RTOL, PF.ATOL      # the golden tolerances: |got - ref| <= ATOL * max|ref| + RTOL * |ref|
NORMS = NR.KINDS
FWD, BWD = "kpgnn_graph_norm_fwd", "kpgnn_graph_norm_bwd"
OLD = ("kpgnn_body_norm_fwd", "kpgnn_body_norm_bwd")
BODIES = [("KPGINPlus", 4, 4, 32), ("KPGIN", 3, 3, 33)]


def _dev():
    return torch.device("cuda:0")


def _model(model_name, K, L, H, norm_type, seed=3, norm_scope="graph"):
    """Body + regression head as tests/test_body_norm.py builds them, with a norm_scope; Layer's weight and bias get seeded
    values away from 1 and 0."""
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(seed)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type=norm_type,
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0,
                         norm_scope=norm_scope)
    model = B.GraphRegression(gnn, "sum")
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for m in gnn.norms:
            if isinstance(m, B.LayerNorm):
                m.weight.copy_(1 + 0.3 * torch.randn(H, generator=g))
                m.bias.copy_(0.2 * torch.randn(H, generator=g))
    return model


class _Switch:
    """set_native_norms(on); on the per-graph route every kind follows it, GraphSize on exact-shape batches included."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from kp_gnn_amd import ops
        self.prev = ops.set_native_norms(self.on)

    def __exit__(self, *exc):
        from kp_gnn_amd import ops
        ops.set_native_norms(self.prev)
        return False


# ------------------------------------------------------------------------------------------------ 1. native against framework
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("model_name,K,L,H", BODIES)
def test_native_equals_the_framework_per_graph_expression(model_name, K, L, H, norm):
    """The same model and batch (48 molecules) with set_native_norms(True) and (False) under norm_scope="graph": score, loss
    and every parameter gradient within the golden tolerances; and the scope matters - the whole-batch score is another."""
    from test_jk import _close, _close_grads, _train_step
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model(model_name, K, L, H, norm).to(dev).train()
    b = synthetic_zinc_batch(48, seed0=11, K=K).to(dev)
    b.build_csr()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = {}
    for on in (True, False):
        model.load_state_dict(sd)          # (the layers' own BatchNorm running statistics must not reach the second run)
        with _Switch(on):
            res[on] = _train_step(model, b)
    name = f"{model_name} norm={norm} scope=graph"
    _close(res[True][0], res[False][0], name + ": score")
    _close(res[True][1], res[False][1], name + ": loss")
    _close_grads(res[True][2], res[False][2], name + ": gradients")
    assert any(float(g.abs().max()) > 0 for g in res[True][2].values())
    if norm == "Layer":
        assert all(float(res[True][2][f"embedding_model.norms.{l}.{k}"].abs().max()) > 0 for l in range(L) for k in ("weight", "bias"))
    whole = _model(model_name, K, L, H, norm, norm_scope="batch").to(dev).train()
    whole.load_state_dict(sd)
    assert not torch.allclose(_train_step(whole, b)[0], res[True][0], rtol=1e-3, atol=1e-3)


# ------------------------------------------------------------------------------------------------ 2. which launches
@pytest.mark.parametrize("norm", NORMS)
def test_a_body_launches_the_graph_norm_once_per_layer_and_direction(norm, monkeypatch):
    """GNNPlus K = 3, L = 3, h = 24 on 7 molecules under norm_scope="graph": exactly L kpgnn_graph_norm_fwd and L
    kpgnn_graph_norm_bwd calls per training step and no kpgnn_body_norm_* call, under the DEFAULT settings (GraphSize included);
    neither with the switch off.  norm_scope="batch" makes the calls it made before: L of each kpgnn_body_norm_* entry (none for
    GraphSize, opt-in on exact-shape batches) and no kpgnn_graph_norm_* call."""
    from test_jk import _record, _train_step
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    b = synthetic_zinc_batch(7, seed0=5, K=3).to(dev)
    b.build_csr()
    model = _model("KPGINPlus", 3, 3, 24, norm).to(dev).train()
    launches = _record(monkeypatch)
    _train_step(model, b)
    assert launches.count(FWD) == 3 and launches.count(BWD) == 3, launches
    assert not any(n in launches for n in OLD), launches
    del launches[:]
    with _Switch(False):
        _train_step(model, b)
    assert not any(n in launches for n in (FWD, BWD) + OLD) and launches, launches
    del launches[:]
    _train_step(_model("KPGINPlus", 3, 3, 24, norm, norm_scope="batch").to(dev).train(), b)
    want = 0 if norm == "GraphSize" else 3
    assert launches.count(OLD[0]) == want and launches.count(OLD[1]) == want, launches
    assert FWD not in launches and BWD not in launches, launches


# ------------------------------------------------------------------------------------------------ 3. evaluation
@pytest.mark.parametrize("norm", NORMS)
def test_evaluation_is_the_training_forward_and_saves_nothing(norm, monkeypatch):
    """module.eval() under no_grad gives the bits of the training-mode forward of the same weights, through ONE
    kpgnn_graph_norm_fwd call and no autograd node; with a gradient required a node appears.  Against float64 per graph."""
    from test_jk import _record
    from kp_gnn_amd import body as B
    dev = _dev()
    C = 32
    mod = {"Layer": lambda: B.LayerNorm(C), "Instance": lambda: B.InstanceNorm(C), "GraphSize": B.GraphSizeNorm,
           "Pair": B.PairNorm}[norm]().to(dev)
    sizes = [9, 37, 0, 1, 150, 3]
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    N, G = ptr[-1], len(sizes)
    batch = GR.batch_of(ptr).to(dev)
    g = torch.Generator().manual_seed(4)
    x, res = (0.5 + torch.randn(N, C, generator=g)).to(dev), torch.randn(N, C, generator=g).to(dev)
    launches = _record(monkeypatch)
    train = mod.train()(x.clone().requires_grad_(True), residual=res, batch=batch, num_graphs=G)
    assert train.grad_fn is not None and launches == [FWD], launches
    del launches[:]
    with torch.no_grad():
        ev = mod.eval()(x, residual=res, batch=batch, num_graphs=G)
    assert launches == [FWD], launches
    assert ev.grad_fn is None and not ev.requires_grad
    assert torch.equal(ev, train.detach())
    plain = mod(x, residual=res, batch=batch, num_graphs=G)      # grad mode on, but only Layer's parameters ask for a gradient
    assert (plain.grad_fn is not None) == (norm == "Layer")
    want = GR.norm(norm, x.cpu().double(), ptr, *[q.detach().cpu().double() for q in mod.parameters()], residual=res.cpu().double())
    for _, r0, r1 in GR.blocks(ptr):
        err = (ev[r0:r1].cpu().double() - want[r0:r1]).abs()
        assert bool((err <= ATOL * float(want[r0:r1].abs().max()) + RTOL * want[r0:r1].abs()).all()), (r1 - r0, float(err.max()))


# ------------------------------------------------------------------------------------------------ 4. static batch, 5. capture
def _check_step(got, ref, model, what):
    """(loss, score, gradient list as test_virtual_node._step returns it) of two steps within the golden tolerances."""
    from test_jk import _close, _close_grads
    (l0, s0, g0), (l1, s1, g1) = got, ref
    _close(s0, s1, what + ": score")
    _close(l0, l1, what + ": loss")
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    named = lambda gs: {n: (torch.zeros_like(p) if q is None else q) for (n, p), q in zip(params, gs)}
    assert len(g0) == len(g1) == len(params)
    _close_grads(named(g0), named(g1), what + ": gradients")


def _dataset(n, seed0, K):
    from test_dataset import molecules
    from kp_gnn_amd.dataset import KHopDataset
    raw = molecules(n, seed0=seed0)
    return KHopDataset.from_collated(raw.collated((K, 50, 6, 3, 50, 50, "spd")), raw.node_ptr, _dev())


@pytest.mark.parametrize("norm", NORMS)
def test_static_batch_under_dynamic_rows_equals_exact_shapes(norm):
    """KP-GIN+ (4,4,32) with norm_scope="graph" in training mode on a dataset.StaticBatch (32 graphs out of 120 molecules, two
    id sets) inside sb.dynamic(): the capacity exceeds the live node count and the batch vector's dead tail repeats the last
    graph id, so a dead row that reached a graph's statistics would show.  Score, loss and gradients are those of the
    exact-shape collate of the same ids within the golden tolerances; with the switch off the same call raises (the framework
    expression has no dynamic row count)."""
    from test_virtual_node import _step
    from kp_gnn_amd import _lib
    dev = _dev()
    K, L, H, Bsz = 4, 4, 32, 32
    ds = _dataset(120, 21, K)
    model = _model("KPGINPlus", K, L, H, norm, seed=0).to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sb = ds.static_batch(Bsz)
    rng = np.random.default_rng(3)
    for i in range(2):
        ids = rng.permutation(120)[:Bsz]
        model.load_state_dict(sd)
        l, s, g = _step(model, ds.collate(ids))
        ref = (l.clone(), s.detach().clone(), g)
        model.load_state_dict(sd)
        with sb.dynamic():
            sb.stage(ids)
            sb.launch_collate()
            l, s, g = _step(model, sb.batch)
            torch.cuda.synchronize()
            assert sb.live[0] < sb.N_cap
            _check_step((l, s.detach(), g), ref, model, f"norm {norm} scope graph static batch, set {i}")
            if i == 0:
                with _Switch(False), pytest.raises(_lib.KpgnnError, match="dynamic row count"):
                    model(sb.batch)
    torch.cuda.synchronize()


@pytest.mark.parametrize("norm", NORMS)
def test_training_step_is_captured_and_replays_on_two_id_sets(norm):
    """Collate, forward, L1 loss and backward of the KP-GIN+ (4,4,32) body with norm_scope="graph" on a StaticBatch in ONE
    torch.cuda.graph after an eager warm-up step (a host synchronisation inside the region would fail the capture), replayed on
    two id sets: each replay matches the eager exact-shape step of the same ids within the golden tolerances."""
    from test_virtual_node import _step
    dev = _dev()
    K, L, H, Bsz = 4, 4, 32, 12
    ds = _dataset(64, 5, K)
    model = _model("KPGINPlus", K, L, H, norm).to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(9)
    id_sets = [rng.permutation(64)[:Bsz] for _ in range(2)]
    refs = []
    for ids in id_sets:
        model.load_state_dict(sd)
        l, s, g = _step(model, ds.collate(ids))
        refs.append((l.clone(), s.detach().clone(), g))
    del l, s, g         # (a live autograd graph from another stream makes the engine synchronise streams inside the capture)
    sb = ds.static_batch(Bsz)
    with sb.dynamic():
        model.load_state_dict(sd)
        sb.stage(id_sets[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sb.launch_collate()
            _step(model, sb.batch)                       # the warm-up, and the batch vector's one eager use
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            sb.launch_collate()
            out = _step(model, sb.batch)
    for i, (ids, ref) in enumerate(zip(id_sets, refs)):
        model.load_state_dict(sd)
        sb.stage(ids)
        graph.replay()
        torch.cuda.synchronize()
        _check_step((out[0], out[1].detach(), out[2]), ref, model, f"norm {norm} scope graph replay {i}")


# ------------------------------------------------------------------------------------------------ 6. a graph's bits
def test_a_graphs_rows_are_the_same_bits_in_a_batch_of_1_and_of_7():
    """A model of an embedding and ONE GraphSizeNorm layer - no BatchNorm anywhere, so nothing else ties a graph to its batch:
    with the batch vector handed on, the rows of every graph, and the gradient that reaches them, are bitwise the same in a
    batch of 7 and in a batch of that graph alone; without it (the whole batch as one graph) they are not."""
    from kp_gnn_amd import body as B
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    torch.manual_seed(1)
    emb, norm = torch.nn.Embedding(21, 24).to(dev), B.GraphSizeNorm()

    def run(x, batch, G):
        h = emb(x.view(-1)).detach().requires_grad_(True)
        y = norm(h) if batch is None else norm(h, batch=batch, num_graphs=G)
        (gx,) = torch.autograd.grad(y, h, torch.ones_like(y))
        return y.detach(), gx

    seven = synthetic_zinc_batch(7, seed0=5, K=3).to(dev)
    y7, g7 = run(seven.x, seven.batch, 7)
    w7, _ = run(seven.x, None, 7)
    bounds = torch.searchsorted(seven.batch, torch.arange(8, device=dev)).tolist()
    for i in range(7):
        r0, r1 = bounds[i], bounds[i + 1]
        alone = seven.x[r0:r1].clone()                  # the same molecule as a batch of one graph
        y1, g1 = run(alone, torch.zeros(r1 - r0, dtype=torch.int64, device=dev), 1)
        assert torch.equal(y1.view(torch.int32), y7[r0:r1].view(torch.int32)), i
        assert torch.equal(g1.view(torch.int32), g7[r0:r1].view(torch.int32)), i
        assert not torch.equal(y1, w7[r0:r1]), i
