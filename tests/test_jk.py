"""The jumping-knowledge readouts "sum", "max" and "attention" of the bodies on kpgnn_jk_reduce_fwd / _bwd (csrc/jk_reduce.hip)
through ops.jk_reduce: which launches a body makes, the native route against the torch.stack expressions on the same device,
JK = sum against the float64 oracle in both kernel regimes, the evaluation forward, and a dataset.StaticBatch.

Reference: models/GNNs.py, the JK branches of the three bodies; restated for sum / max in oracle/kp_model_oracle.py."""
import argparse

import numpy as np
import pytest
import torch

import parity_f64 as PF

pytestmark = pytest.mark.gpu

RTOL, ATOL = PF.RTOL, PF.ATOL      # the golden tolerances: |got - ref| <= ATOL * max|ref| + RTOL * |ref|
M_F64 = 3                          # close_to_f64: at most 3 times as far from float64 as the fp32 CPU oracle
JKS = ("sum", "max", "attention")
BODIES = [("KPGINPlus", 4, 4, 32), ("KPGIN", 3, 3, 24)]
FWD, BWD = "kpgnn_jk_reduce_fwd", "kpgnn_jk_reduce_bwd"


def _dev():
    return torch.device("cuda:0")


def _model(model_name, K, L, H, JK, seed=3):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(seed)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK=JK, norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    return B.GraphRegression(gnn, "sum")


def _close(got, ref, name):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bound = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    assert bool((err <= bound).all()), (name, float(err.max()))


def _close_grads(got, ref, name):
    """The golden tolerances for a set of parameter gradients, scaled as tests/test_gpu_parity.py scales them."""
    import types
    from test_gpu_parity import _close_param_grads
    _close_param_grads({k: types.SimpleNamespace(grad=v) for k, v in got.items()}, ref, name, RTOL, ATOL)


def _train_step(model, b):
    model.zero_grad(set_to_none=True)
    score = model(b)
    loss = (score.squeeze() - b.y.squeeze()).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    got = {n: (torch.zeros_like(q) if q.grad is None else q.grad.clone()) for n, q in model.named_parameters() if q.requires_grad}
    return score.detach(), loss.detach(), got


def _record(monkeypatch):
    from kp_gnn_amd import _lib
    launches, real = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    return launches


# ------------------------------------------------------------------------------------------------ 1. which launches
@pytest.mark.parametrize("JK", JKS)
def test_a_body_launches_the_reduce_once_per_direction(JK, monkeypatch):
    """GNNPlus K = 3, L = 3, h = 24 on 7 molecules: one kpgnn_jk_reduce_fwd per forward; one kpgnn_jk_reduce_bwd per backward
    for max and attention and none for sum (every state's gradient is the incoming one); neither with the switch off."""
    from kp_gnn_amd import ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model("KPGINPlus", 3, 3, 24, JK).to(dev).train()
    b = synthetic_zinc_batch(7, seed0=5, K=3).to(dev)
    b.build_csr()
    launches = _record(monkeypatch)
    assert ops.native_jk()
    on = _train_step(model, b)
    assert launches.count(FWD) == 1, launches
    assert launches.count(BWD) == (0 if JK == "sum" else 1), launches
    del launches[:]
    prev = ops.set_native_jk(False)
    try:
        off = _train_step(model, b)
    finally:
        ops.set_native_jk(prev)
    assert FWD not in launches and BWD not in launches and launches, launches
    _close(on[0], off[0], f"{JK}: score, native against the framework expression")


# ------------------------------------------------------------------------------------------------ 2. native against framework
@pytest.mark.parametrize("JK", JKS)
@pytest.mark.parametrize("model_name,K,L,H", BODIES)
def test_native_equals_the_framework_expression(model_name, K, L, H, JK):
    """The same model and batch (48 molecules) with set_native_jk(True) and (False): score, loss and every parameter gradient
    within the golden tolerances.  For max this is the body-level check: both runs reduce bit-identical states, so no arg-max
    can flip between them."""
    from kp_gnn_amd import ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model(model_name, K, L, H, JK).to(dev).train()
    b = synthetic_zinc_batch(48, seed0=11, K=K).to(dev)
    b.build_csr()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    res = {}
    for on in (True, False):
        model.load_state_dict(sd)          # (the running statistics of the first run must not reach the second)
        prev = ops.set_native_jk(on)
        try:
            res[on] = _train_step(model, b)
        finally:
            ops.set_native_jk(prev)
    name = f"{model_name} JK={JK}"
    _close(res[True][0], res[False][0], name + ": score")
    _close(res[True][1], res[False][1], name + ": loss")
    _close_grads(res[True][2], res[False][2], name + ": gradients")
    assert any(float(g.abs().max()) > 0 for g in res[True][2].values())


# ------------------------------------------------------------------------------------------------ 3. sum against float64
def _oracle(sd, data, y, dtype, *, model_name, K, L, JK, threads=None, training=True):
    """parity_f64.oracle_body with a JK of the caller's choice (that helper hard-codes JK="concat")."""
    from oracle import kp_model_oracle as MO
    kind, layer_kind = PF.BODY_KIND[model_name]
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        p = {k: (v.detach().to(dtype).clone().requires_grad_(training) if PF.trainable(k, v) else PF.to_dtype(v.detach(), dtype).clone())
             for k, v in sd.items()}
        with torch.set_grad_enabled(training):
            score = MO.graph_regression_forward(p, data, kind=kind, layer_kind=layer_kind, K=K, num_layer=L,
                                                combine_kind="geometric", JK=JK, residual=True, training=training)
        if not training:
            return score.detach()
        loss = (score.squeeze() - y.to(dtype).squeeze()).abs().mean()
        loss.backward()
    finally:
        torch.set_num_threads(before)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items() if v.requires_grad}
    return score.detach(), loss.detach(), grads


_REFS = {}


def _refs(sd, host, **kw):
    """(float64 oracle result, [fp32 oracle results at 4, 8 and 16 threads]), computed once per configuration."""
    key = (tuple(sorted(kw.items())), PF.tensors_sha256(host.as_dict(), sd))
    if key not in _REFS:
        data = host.as_dict()
        _REFS[key] = (_oracle(sd, data, host.y, torch.float64, **kw),
                      [_oracle(sd, data, host.y, torch.float32, threads=t, **kw) for t in PF.THREADS])
    return _REFS[key]


@pytest.mark.parametrize("graphs", [48, 220])
@pytest.mark.parametrize("model_name,K,L,H", BODIES)
def test_sum_bodies_vs_float64(model_name, K, L, H, graphs, monkeypatch):
    """JK = sum, residual, no dropout: score, loss and every parameter gradient through close_to_f64 with M = 3 against the
    float64 oracle (fp32 oracle at 4, 8 and 16 threads as the yardstick).  48 molecules: the small-batch kernels; 220:
    N = 5148 >= 4096, the large-batch paths.  (max is not held to float64 at body level: an element whose two largest states
    differ by less than the fp32 rounding of the layers before it selects another slot in float64 - no kernel tolerance
    describes that; tests/test_jk_cabi.py holds max bitwise at operator level.)  Measured on the MI355X (E32 / gscale of the
    gradients; largest ratio |ours - float64| / max(e32_k, 0.1 E32) over the gradient tensors, then the score's and the loss's):
        KP-GIN+ K4 L4 h32   48 graphs   1.9e-4   0.01 (output_proj.0.weight)   0.54   0.17
        KP-GIN+ K4 L4 h32  220 graphs   6.3e-7   1.18 (output_proj.0.weight)   0.15   0.16
        KP-GIN  K3 L3 h24   48 graphs   4.2e-7   1.04 (output_proj.0.weight)   0.52   0.13
        KP-GIN  K3 L3 h24  220 graphs   2.1e-5   0.13 (output_proj.0.weight)   0.22   0.04"""
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model(model_name, K, L, H, "sum")
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(graphs, seed0=11, K=K)
    ref64, ref32 = _refs(sd, host, model_name=model_name, K=K, L=L, JK="sum")
    model = model.to(dev).train()
    b = host.to(dev)
    b.build_csr()
    assert (b.num_nodes >= 4096) == (graphs == 220)
    launches = _record(monkeypatch)
    score, loss, got = _train_step(model, b)
    monkeypatch.undo()
    assert launches.count(FWD) == 1 and BWD not in launches, launches
    name = f"jk sum {model_name} K{K} L{L} h{H} N{b.num_nodes}"
    PF.print_ratios(name + " score", PF.close_to_f64(score, ref64[0], [r[0] for r in ref32], name + " score", M_F64))
    PF.print_ratios(name + " loss", PF.close_to_f64(loss, ref64[1], [r[1] for r in ref32], name + " loss", M_F64))
    PF.print_ratios(name, PF.close_to_f64(got, ref64[2], [r[2] for r in ref32], name, M_F64))


# ------------------------------------------------------------------------------------------------ 4. evaluation
def _randomise_running_stats(model, seed=41):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():          # running statistics away from their initial 0 / 1
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))


@pytest.mark.parametrize("JK", JKS)
def test_evaluation_forward_saves_nothing(JK, monkeypatch):
    """model.eval() under no_grad: kpgnn_jk_reduce_fwd runs once, asks for no arg / w (nothing is saved), the reduce makes no
    autograd node, and the score equals the framework path's within the golden tolerances."""
    from kp_gnn_amd import _lib, ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _model("KPGINPlus", 4, 4, 32, JK)
    _randomise_running_stats(model)
    model = model.to(dev).eval()
    b = synthetic_zinc_batch(48, seed0=11, K=4).to(dev)
    b.build_csr()
    seen, real = [], _lib.launch

    def spy(name, dev_, *a, **k):
        if name == FWD:
            d = a[0]._obj
            seen.append((d.arg, d.w, d.S, d.mode))
        return real(name, dev_, *a, **k)

    monkeypatch.setattr(_lib, "launch", spy)
    outs, real_reduce = [], ops.jk_reduce
    monkeypatch.setattr("kp_gnn_amd.body.jk_reduce", lambda *a, **k: (outs.append(real_reduce(*a, **k)), outs[-1])[1])
    with torch.no_grad():
        score = model(b)
        prev = ops.set_native_jk(False)
        try:
            ref = model(b)
        finally:
            ops.set_native_jk(prev)
    torch.cuda.synchronize()
    assert seen == [(None, None, 5, ops.JK_MODES["softmax" if JK == "attention" else JK])], seen
    assert len(outs) == 1 and outs[0].grad_fn is None and not outs[0].requires_grad
    assert score.grad_fn is None
    _close(score, ref, f"eval JK={JK}: score, native against the framework expression")


def test_reduce_of_states_that_need_no_gradient_makes_no_autograd_node():
    from kp_gnn_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    states = [torch.randn(50, 24, generator=g).to(dev) for _ in range(3)]
    for mode in ("sum", "max"):
        out = ops.jk_reduce(states, mode)
        assert out.grad_fn is None, mode
    for t in states:
        t.requires_grad_(True)
    for mode in ("sum", "max"):
        out = ops.jk_reduce(states, mode)
        assert out.grad_fn is not None, mode
        with torch.no_grad():
            assert ops.jk_reduce(states, mode).grad_fn is None
    # a state that is a column slice is made contiguous first; S > 32 keeps the framework expression
    wide = torch.randn(50, 40, generator=g).to(dev)
    got = ops.jk_reduce([wide[:, 8:32], states[0].detach()], "max")
    assert torch.equal(got, torch.maximum(wide[:, 8:32], states[0].detach()))
    many = [states[0].detach()] * 33
    assert not ops.jk_native_applies(many) and ops.jk_native_applies(many[:32])
    assert torch.equal(ops.jk_reduce(many, "max"), states[0].detach())


# ------------------------------------------------------------------------------------------------ 5. static batch
def test_sum_on_a_static_batch_under_dynamic_rows():
    """JK = sum, model.eval() under no_grad on a dataset.StaticBatch (32 graphs out of 120 molecules, two id sets) under
    dynamic_rows: the capacity exceeds the live node count, so a dead row that reached the pooled sums would show.  Bound: the
    one tests/test_virtual_node.py holds its evaluation forward on a static batch to - close_to_f64 with M = 3 against the
    float64 oracle (training=False), the fp32 oracle at 4, 8 and 16 threads as the yardstick."""
    from test_dataset import molecules
    from kp_gnn_amd.dataset import KHopDataset
    dev = _dev()
    K, L, H, Bsz = 4, 4, 32, 32
    raw = molecules(120, seed0=21)
    args = (K, 50, 6, 3, 50, 50, "spd")
    ds = KHopDataset.from_collated(raw.collated(args), raw.node_ptr, dev)
    model = _model("KPGINPlus", K, L, H, "sum", seed=0)
    _randomise_running_stats(model)
    model = model.to(dev).eval()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    sb = ds.static_batch(Bsz)
    rng = np.random.default_rng(3)
    kw = dict(model_name="KPGINPlus", K=K, L=L, JK="sum", training=False)
    for i in range(2):
        ids = rng.permutation(120)[:Bsz]
        host = raw.subset(ids).collated(args)
        s64 = _oracle(sd, host.as_dict(), host.y, torch.float64, **kw)
        s32 = [_oracle(sd, host.as_dict(), host.y, torch.float32, threads=t, **kw) for t in PF.THREADS]
        with torch.no_grad(), sb.dynamic():
            sb.stage(ids)
            sb.launch_collate()
            score = model(sb.batch)
            torch.cuda.synchronize()
        assert sb.live[0] < sb.N_cap
        name = f"jk sum eval static batch, set {i}"
        PF.print_ratios(name, PF.close_to_f64(score, s64, s32, name, M_F64))
