"""norm_type "Layer", "Instance", "GraphSize" and "Pair" of the three bodies on kpgnn_body_norm_fwd / _bwd (csrc/body_norm.hip)
through ops.body_norm: which launches a body makes, the native route against the framework expression on the same device, two
bodies against the float64 oracle, the evaluation forward, a dataset.StaticBatch under dynamic_rows, and a captured step.

Reference: models/GNNs.py:103-112 and the norm calls of the three forwards; restated in tests/norm_ref.py."""
import argparse

import numpy as np
import pytest
import torch

import norm_ref as NR
import parity_f64 as PF

pytestmark = pytest.mark.gpu

RTOL, ATOL = PF.RTOL, PF.ATOL      # the golden tolerances: |got - ref| <= ATOL * max|ref| + RTOL * |ref|
M_F64 = 3                          # close_to_f64: at most 3 times as far from float64 as the fp32 CPU oracle
NORMS = NR.KINDS
FWD, BWD = "kpgnn_body_norm_fwd", "kpgnn_body_norm_bwd"
BODIES = [("KPGINPlus", 4, 4, 32), ("KPGIN", 3, 3, 24), ("KPGINPrime", 3, 3, 24)]


def _dev():
    return torch.device("cuda:0")


def _model(model_name, K, L, H, norm_type, seed=3):
    """Body + regression head as tests/test_jk.py builds them (JK concat, residual, no dropout, no virtual node); Layer's
    weight and bias get seeded values away from 1 and 0."""
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(seed)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type=norm_type,
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    model = B.GraphRegression(gnn, "sum")
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for m in gnn.norms:
            if isinstance(m, B.LayerNorm):
                m.weight.copy_(1 + 0.3 * torch.randn(H, generator=g))
                m.bias.copy_(0.2 * torch.randn(H, generator=g))
    return model


class _Switch:
    """set_native_norms(on), and GraphSize - opt-in on exact-shape batches - along with it."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from kp_gnn_amd import ops
        self.prev = ops.set_native_norms(self.on)
        self.prev_gs = ops.set_native_norm_exact("GraphSize", self.on)

    def __exit__(self, *exc):
        from kp_gnn_amd import ops
        ops.set_native_norms(self.prev)
        ops.set_native_norm_exact("GraphSize", self.prev_gs)
        return False


# ------------------------------------------------------------------------------------------------ 1. which launches
@pytest.mark.parametrize("norm", NORMS)
def test_a_body_launches_the_norm_once_per_layer_and_direction(norm, monkeypatch):
    """GNNPlus K = 3, L = 3, h = 24 on 7 molecules: exactly L kpgnn_body_norm_fwd and L kpgnn_body_norm_bwd per training step,
    neither with the switch off; norm_type "Batch" makes neither."""
    from test_jk import _close, _record, _train_step
    from kp_gnn_amd import ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model("KPGINPlus", 3, 3, 24, norm).to(dev).train()
    b = synthetic_zinc_batch(7, seed0=5, K=3).to(dev)
    b.build_csr()
    launches = _record(monkeypatch)
    assert ops.native_norms() and ops.native_norm_exact(norm) == (norm != "GraphSize")
    with _Switch(True):
        on = _train_step(model, b)
    assert launches.count(FWD) == 3 and launches.count(BWD) == 3, launches
    del launches[:]
    if norm == "GraphSize":          # opt-in on exact-shape batches: the default setting keeps the framework expression
        _train_step(model, b)
        assert FWD not in launches and BWD not in launches and launches, launches
        del launches[:]
    with _Switch(False):
        off = _train_step(model, b)
    assert FWD not in launches and BWD not in launches and launches, launches
    _close(on[0], off[0], f"{norm}: score, native against the framework expression")
    del launches[:]
    _train_step(_model("KPGINPlus", 3, 3, 24, "Batch").to(dev).train(), b)
    assert FWD not in launches and BWD not in launches and launches, launches


# ------------------------------------------------------------------------------------------------ 2. native against framework
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("model_name,K,L,H", BODIES)
def test_native_equals_the_framework_expression(model_name, K, L, H, norm):
    """The same model and batch (48 molecules) with set_native_norms(True) and (False): score, loss and every parameter
    gradient within the golden tolerances."""
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
    name = f"{model_name} norm={norm}"
    _close(res[True][0], res[False][0], name + ": score")
    _close(res[True][1], res[False][1], name + ": loss")
    _close_grads(res[True][2], res[False][2], name + ": gradients")
    assert any(float(g.abs().max()) > 0 for g in res[True][2].values())
    if norm == "Layer":
        assert all(float(res[True][2][f"embedding_model.norms.{l}.{k}"].abs().max()) > 0 for l in range(L) for k in ("weight", "bias"))


# ------------------------------------------------------------------------------------------------ 3. against float64
def _patched_norm(kind):
    """oracle.kp_model_oracle.batch_norm's signature; the oracle passes the prefix norms.{l}.module of PyG's BatchNorm wrapper,
    Layer's parameters live one level up."""
    def fn(p, prefix, x, training):
        base = prefix[:-len(".module")] if prefix.endswith(".module") else prefix
        return NR.norm(kind, x, p.get(base + ".weight"), p.get(base + ".bias"))
    return fn


_REFS = {}


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("model_name,K,L,H", BODIES[:2])
def test_bodies_vs_float64(model_name, K, L, H, norm, monkeypatch):
    """48 molecules, JK concat, residual, no dropout: score, loss and every parameter gradient through close_to_f64 with M = 3
    against parity_f64.oracle_body in float64, whose per-layer norm is replaced - here, in the test - by tests/norm_ref.py; the
    same oracle in fp32 at 4, 8 and 16 threads is the yardstick.  Measured on the MI355X (E32 / gscale of the gradients; largest
    ratio |ours - float64| / max(e32_k, 0.1 E32) over the gradient tensors, then the score's and the loss's; the printed lines are
    in profiles/norms/f64_parity_bodies.txt):
        KP-GIN+ K4 L4 h32  Layer      2.0e-7   0.63 (regressor.weight)              0.99     0.55
        KP-GIN+ K4 L4 h32  Instance   3.7e-7   0.89 (gnns.0.mlp.3.weight)           0.78     2.48
        KP-GIN+ K4 L4 h32  GraphSize  2.1e-7   1.00 (regressor.weight)              0.70     0.16
        KP-GIN+ K4 L4 h32  Pair       1.6e-7   0.59 (regressor.weight)              0.89     2.57
        KP-GIN  K3 L3 h24  Layer      1.4e-7   2.77 (output_proj.0.weight)          0.70     0.35
        KP-GIN  K3 L3 h24  Instance   3.4e-7   1.11 (output_proj.0.weight)          0.97   121.08
        KP-GIN  K3 L3 h24  GraphSize  8.9e-8   3.99 (output_proj.0.weight)          1.16     1.00
        KP-GIN  K3 L3 h24  Pair       1.8e-7   4.91 (output_proj.0.weight)          0.80     1.00
    A ratio above M = 3 passes where close_to_f64's floor (ATOL * max(|ref_k|, 0.1 gscale) + RTOL * |ref_k|, the golden
    tolerances) is the larger bound: the yardstick is then smaller than fp32 can resolve.  The loss at 121: the three fp32 oracle
    runs happen to land within 5.5e-10 (relative) of the float64 loss, a hundredth of an fp32 ulp; ours is 6.7e-8 off, one ulp.
    output_proj.0.weight at 2.8 - 4.9: the unit is at most E32, so the error is at most 4.91 * 1.76e-7 = 8.7e-7 of gscale, and the
    floor is at least 1e-5 * 0.1 gscale = 1e-6 of gscale."""
    from oracle import kp_model_oracle as MO
    from test_jk import _record, _train_step
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model(model_name, K, L, H, norm)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(48, seed0=11, K=K)
    key = (model_name, norm)
    if key not in _REFS:
        monkeypatch.setattr(MO, "batch_norm", _patched_norm(norm))
        _REFS[key] = PF.oracle_f64_and_f32(sd, host.as_dict(), host.y, model_name=model_name, combine="geometric", K=K, L=L)
        monkeypatch.undo()
    ref64, ref32 = _REFS[key]
    assert all(bool(torch.isfinite(v).all()) for v in ref64[2].values())
    model = model.to(dev).train()
    b = host.to(dev)
    b.build_csr()
    launches = _record(monkeypatch)
    with _Switch(True):
        score, loss, got = _train_step(model, b)
    monkeypatch.undo()
    assert launches.count(FWD) == L and launches.count(BWD) == L, launches
    name = f"norm {norm} {model_name} K{K} L{L} h{H} N{b.num_nodes}"
    PF.print_ratios(name + " score", PF.close_to_f64(score, ref64[0], [r[0] for r in ref32], name + " score", M_F64))
    PF.print_ratios(name + " loss", PF.close_to_f64(loss, ref64[1], [r[1] for r in ref32], name + " loss", M_F64))
    PF.print_ratios(name, PF.close_to_f64(got, ref64[2], [r[2] for r in ref32], name, M_F64))


# ------------------------------------------------------------------------------------------------ 4. evaluation
@pytest.mark.parametrize("norm", NORMS)
def test_evaluation_is_the_training_forward_and_saves_nothing(norm, monkeypatch):
    """None of the four has running statistics: module.eval() under no_grad gives the bits of the training-mode forward of the
    same weights, through ONE kpgnn_body_norm_fwd call and no autograd node; with a gradient required a node appears."""
    from test_jk import _record
    from kp_gnn_amd import body as B
    dev = _dev()
    C = 32
    mod = {"Layer": lambda: B.LayerNorm(C), "Instance": lambda: B.InstanceNorm(C), "GraphSize": B.GraphSizeNorm,
           "Pair": B.PairNorm}[norm]().to(dev)
    g = torch.Generator().manual_seed(4)
    x, res = (0.5 + torch.randn(200, C, generator=g)).to(dev), torch.randn(200, C, generator=g).to(dev)
    launches = _record(monkeypatch)
    with _Switch(True):
        train = mod.train()(x.clone().requires_grad_(True), residual=res)
        assert train.grad_fn is not None and launches == [FWD], launches
        del launches[:]
        with torch.no_grad():
            ev = mod.eval()(x, residual=res)
        assert launches == [FWD], launches
        assert ev.grad_fn is None and not ev.requires_grad
        assert torch.equal(ev, train.detach())
        plain = mod(x, residual=res)          # grad mode on, but nothing but Layer's parameters asks for a gradient
        assert (plain.grad_fn is not None) == (norm == "Layer")
    want = NR.norm(norm, x.cpu().double(), *[q.detach().cpu().double() for q in mod.parameters()], residual=res.cpu().double())
    err = (ev.cpu().double() - want).abs()
    assert bool((err <= ATOL * float(want.abs().max()) + RTOL * want.abs()).all()), float(err.max())


# ------------------------------------------------------------------------------------------------ 5. static batch, 6. capture
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


@pytest.mark.parametrize("norm", NORMS)
def test_static_batch_under_dynamic_rows_equals_exact_shapes(norm):
    """KP-GIN+ (4,4,32) in training mode on a dataset.StaticBatch (32 graphs out of 120 molecules, two id sets) inside
    sb.dynamic(): the capacity exceeds the live node count, so a dead row that reached the statistics would show.  Score,
    loss and gradients are those of the exact-shape collate of the same ids within the golden tolerances - under the DEFAULT
    settings: GraphSize, opt-in on exact-shape batches, is native inside the block all the same (its only route there), and its
    exact-shape reference is the framework expression.  With the switch off the same call raises (the framework expression has
    no dynamic row count)."""
    from test_dataset import molecules
    from test_virtual_node import _step
    from kp_gnn_amd import _lib
    from kp_gnn_amd.dataset import KHopDataset
    dev = _dev()
    K, L, H, Bsz = 4, 4, 32, 32
    raw = molecules(120, seed0=21)
    args = (K, 50, 6, 3, 50, 50, "spd")
    ds = KHopDataset.from_collated(raw.collated(args), raw.node_ptr, dev)
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
            _check_step((l, s.detach(), g), ref, model, f"norm {norm} static batch, set {i}")
            if i == 0:
                with _Switch(False), pytest.raises(_lib.KpgnnError, match="dynamic row count"):
                    model(sb.batch)
    torch.cuda.synchronize()


@pytest.mark.parametrize("norm", NORMS)
def test_training_step_is_captured_and_replays(norm):
    """Forward, L1 loss and backward of the KP-GIN+ (4,4,32) body in ONE torch.cuda.graph after an eager warm-up step (a host
    synchronisation or an allocation outside the graph's pool inside the region would fail the capture), replayed twice: each
    replay matches the eager step within the golden tolerances."""
    from test_dataset import molecules
    from test_virtual_node import _step
    from kp_gnn_amd.dataset import KHopDataset
    dev = _dev()
    K, L, H = 4, 4, 32
    raw = molecules(64, seed0=5)
    ds = KHopDataset.from_collated(raw.collated((K, 50, 6, 3, 50, 50, "spd")), raw.node_ptr, dev)
    model = _model("KPGINPlus", K, L, H, norm).to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    b = ds.collate([9, 3, 60, 21, 22, 23, 0, 63, 11, 40, 41, 5])
    with _Switch(True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            l, s, g = _step(model, b)                    # the eager step: the reference and the warm-up
            ref = (l.clone(), s.detach().clone(), g)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        model.load_state_dict(sd)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _step(model, b)
    for i in range(2):
        model.load_state_dict(sd)
        graph.replay()
        torch.cuda.synchronize()
        _check_step((out[0], out[1].detach(), out[2]), ref, model, f"norm {norm} replay {i}")
