"""The virtual node on the device: kpgnn_vn_add_pool (csrc/virtual_node.hip) through ops.virtual_node_add against float64,
its behaviour on capacity-shaped buffers, the three bodies with virtual_node=True against the float64 oracle in both kernel
regimes, and the things the framework formulation could not do: a captured training step, a dataset.StaticBatch, and the
captured evaluation forward on one.

Reference: models/GNNs.py:196-199,227-230 (h + vn[batch]; global_add_pool(h) + vn through the virtual-node MLP), restated in
oracle/kp_model_oracle.py (virtual_node=True)."""
import argparse

import numpy as np
import pytest
import torch

import parity_f64 as PF

pytestmark = pytest.mark.gpu

RTOL, ATOL = PF.RTOL, PF.ATOL      # the golden tolerances: |got - ref| <= ATOL * max|ref| + RTOL * |ref|
M_F64 = 3                          # close_to_f64: at most 3 times as far from float64 as the fp32 CPU oracle (tests/test_gpu_parity.py)
SIZES = [0, 1, 3, 4, 5, 9, 67, 0, 2]   # empty graphs first and in the middle; the 4-row unroll with every tail


def _dev():
    return torch.device("cuda:0")


def _close(got, ref, name):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bound = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    assert bool((err <= bound).all()), (name, float(err.max()))


def _close_grads(got, ref, name):
    """The golden tolerances for a set of parameter gradients, as tests/test_gpu_parity.py reads them (_close_param_grads, here
    with RTOL / ATOL themselves): |got_k - ref_k| <= RTOL * |ref_k| + ATOL * max(max|ref_k|, 0.1 * gscale); a tensor whose
    reference is the rounding noise of an analytically-zero sum (the bias of a Linear that feeds a BatchNorm - every
    mlp_virtualnode_list.*.{0,3}.bias) must be noise here as well."""
    import types
    from test_gpu_parity import _close_param_grads
    _close_param_grads({k: types.SimpleNamespace(grad=v) for k, v in got.items()}, ref, name, RTOL, ATOL)


def _batch_of(sizes, dev):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(dev)


# ------------------------------------------------------------------------------------------------ 1. the op against float64
def _op_case(D, strided, expanded, want_pool, dev):
    from kp_gnn_amd import ops
    g = torch.Generator().manual_seed(1000 * D + 4 * strided + 2 * expanded + want_pool)
    G, N = len(SIZES), sum(SIZES)
    batch = _batch_of(SIZES, dev)
    wide = torch.randn(N, D + 8 if strided else D, generator=g)
    row = torch.randn(1 if expanded else G, D, generator=g)
    go, gp = torch.randn(N, D, generator=g), torch.randn(G, D, generator=g)

    def run(dtype, device):
        xw = wide.to(device=device, dtype=dtype).requires_grad_(True)
        r = row.to(device=device, dtype=dtype).requires_grad_(True)
        x = xw[:, 4:4 + D] if strided else xw
        v = r.expand(G, -1) if expanded else r
        if v.requires_grad:
            v.retain_grad()
        b = batch.to(device)
        if device.type == "cuda":
            if strided:
                assert x.stride(0) > D
            out, pooled = ops.virtual_node_add(x, v, b, G, want_pool)
        else:
            out = x + v[b]
            pooled = torch.zeros(G, D, dtype=dtype).index_add_(0, b, out) + v if want_pool else None
        loss = (out * go.to(device=device, dtype=dtype)).sum()
        if want_pool:
            loss = loss + (pooled * gp.to(device=device, dtype=dtype)).sum()
        loss.backward()
        return out.detach(), None if pooled is None else pooled.detach(), xw.grad, v.grad, r.grad

    got = run(torch.float32, dev)
    again = run(torch.float32, dev)
    ref = run(torch.float64, torch.device("cpu"))
    what = f"D{D} strided{strided} expanded{expanded} pool{want_pool}"
    for name, a, a2, r in zip(("out", "pooled", "gx", "gv", "grow"), got, again, ref):
        if r is None:
            assert a is None and name == "pooled" and not want_pool
            continue
        _close(a, r, f"{what} {name}")
        if D <= 256:       # (the framework expression beyond the kernel's width pools with fp32 atomics: its bits vary from run to run)
            assert torch.equal(a, a2), f"{what} {name}: a second identical call gave other bits"
    if strided:
        gx = got[2]
        assert float(gx[:, :4].abs().max()) == 0 and float(gx[:, 4 + D:].abs().max()) == 0      # only the slice has a gradient


@pytest.mark.parametrize("D", [104, 18, 33, 120, 256, 260])
def test_op_vs_float64(D, monkeypatch):
    """out, pooled and the gradients of x, v and the single row behind an expanded v from random gout / gpooled, against the
    same expression in float64 on the CPU (golden tolerances); x contiguous and as a column slice, v [G,D] and expanded,
    with and without the pooled sum; D = 104 / 120 / 256 move 16 B per lane, 18 moves 8, 33 moves 4; D = 260 is beyond the
    kernel and takes the framework expression.  On the kernel, a second identical call gives identical bits."""
    from kp_gnn_amd import _lib
    dev = _dev()
    launches = []
    real = _lib.launch

    def spy(name, *a, **k):
        launches.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "launch", spy)
    for strided in (False, True):
        for expanded in (False, True):
            for want_pool in (False, True):
                _op_case(D, strided, expanded, want_pool, dev)
    torch.cuda.synchronize()
    assert ("kpgnn_vn_add_pool" in launches) == (D <= 256), launches


def test_op_under_no_grad_makes_no_autograd_node():
    from kp_gnn_amd import ops
    dev = _dev()
    G, N, D = len(SIZES), sum(SIZES), 32
    x, v = torch.randn(N, D, device=dev, requires_grad=True), torch.randn(G, D, device=dev, requires_grad=True)
    with torch.no_grad():
        out, pooled = ops.virtual_node_add(x, v, _batch_of(SIZES, dev), G, True)
    assert out.grad_fn is None and pooled.grad_fn is None and not out.requires_grad
    ref = x.detach() + v.detach()[_batch_of(SIZES, dev)]
    assert torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------ 2. capacity rows
@pytest.mark.parametrize("D", [104, 33])
@pytest.mark.parametrize("dynamic", [True, False])
def test_capacity_rows_are_left_alone(D, dynamic):
    """Buffers of N + 37 rows: the rows of x beyond graph_ptr[G] hold 1e30, `out` is pre-filled with -7.  With a device-side
    live count (ops.dynamic_rows) and without one, out[:N] and pooled are the exact-shape call's bit for bit and out[N:] keeps
    its pre-fill: the work is driven by the graph pointer."""
    from kp_gnn_amd import ops
    dev = _dev()
    torch.manual_seed(D)
    G, N = len(SIZES), sum(SIZES)
    cap = N + 37
    batch = _batch_of(SIZES, dev)
    ptr = ops.graph_ptr_of(batch, G)
    assert int(ptr[-1]) == N
    x = torch.randn(N, D, device=dev)
    v = torch.randn(G, D, device=dev)
    ref_out, ref_pool = ops._vn_launch(x, v, ptr, G, True)
    xc = torch.full((cap, D), 1e30, device=dev)
    xc[:N] = x
    out = torch.full((cap, D), -7.0, device=dev)
    if dynamic:
        cnt = torch.tensor([N], dtype=torch.int32, device=dev)
        with ops.dynamic_rows(cnt, cap):
            assert ops.dyn_ptr(cap) == cnt.data_ptr()
            got_out, got_pool = ops._vn_launch(xc, v, ptr, G, True, out=out)
    else:
        got_out, got_pool = ops._vn_launch(xc, v, ptr, G, True, out=out)
    torch.cuda.synchronize()
    assert got_out is out
    assert torch.equal(out[:N], ref_out) and torch.equal(got_pool, ref_pool)
    assert bool((out[N:] == -7.0).all())
    assert bool(torch.isfinite(got_pool).all()) and float(got_pool.abs().max()) < 1e6


def test_capacity_equal_to_the_graph_count_is_refused():
    """dyn_ptr matches launches by row count: with a capacity equal to the number of graphs the virtual-node MLP's [G,H] launches
    would be handed the live NODE count.  Refused, not guessed."""
    from kp_gnn_amd import _lib, ops
    dev = _dev()
    gnn = _vn_model("KPGINPlus", 3, 3, 32).embedding_model.to(dev).train()
    G = 12
    cnt = torch.tensor([G], dtype=torch.int32, device=dev)
    with ops.dynamic_rows(cnt, G):
        with pytest.raises(_lib.KpgnnError, match="virtual-node MLP"):
            gnn._vn_update(0, torch.randn(G, 32, device=dev), torch.randn(G, 32, device=dev))


def test_one_graph_in_training_mode_raises_what_batchnorm_raises():
    """G == 1: the virtual-node MLP's BatchNorm1d has one value per channel in training mode and raises, as in the reference;
    in eval mode one graph is fine."""
    dev = _dev()
    gnn = _vn_model("KPGINPlus", 3, 3, 32).embedding_model.to(dev).train()
    vn, tmp = torch.randn(1, 32, device=dev), torch.randn(1, 32, device=dev)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        gnn._vn_update(0, vn, tmp)
    gnn.eval()
    with torch.no_grad():
        assert tuple(gnn._vn_update(0, vn, tmp).shape) == (1, 32)


# ------------------------------------------------------------------------------------------------ 3. bodies against float64
def _vn_model(model_name, K, L, H, seed=3):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(seed)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=True, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    with torch.no_grad():          # (the reference zeroes the virtual node's embedding: a live one also exercises its gradient's scale)
        gnn.virtualnode_embedding.weight.normal_(0.0, 0.5)
    return B.GraphRegression(gnn, "sum")


BODY_KIND = {"KPGINPlus": ("GNNPlus", "KPGINPlus"), "KPGIN": ("GNN", "KPGIN"), "KPGINPrime": ("GNNPrime", "KPGIN")}


def _oracle(sd, data, y, dtype, *, model_name, K, L, threads=None, training=True):
    """parity_f64.oracle_body with virtual_node=True (that helper hard-codes its keyword arguments)."""
    from oracle import kp_model_oracle as MO
    kind, layer_kind = BODY_KIND[model_name]
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        p = {k: (v.detach().to(dtype).clone().requires_grad_(training) if PF.trainable(k, v) else PF.to_dtype(v.detach(), dtype).clone())
             for k, v in sd.items()}
        with torch.set_grad_enabled(training):
            score = MO.graph_regression_forward(p, data, kind=kind, layer_kind=layer_kind, K=K, num_layer=L,
                                                combine_kind="geometric", JK="concat", residual=True, virtual_node=True,
                                                training=training)
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


def _train_step(model, b):
    model.zero_grad(set_to_none=True)
    score = model(b)
    loss = (score.squeeze() - b.y.squeeze()).abs().mean()
    loss.backward()
    torch.cuda.synchronize()
    got = {n: (torch.zeros_like(q) if q.grad is None else q.grad.clone()) for n, q in model.named_parameters() if q.requires_grad}
    return score.detach(), loss.detach(), got


def _check_f64(res, ref64, ref32, name):
    score, loss, got = res
    s64, l64, g64 = ref64
    PF.print_ratios(name + " score", PF.close_to_f64(score, s64, [r[0] for r in ref32], name + " score", M_F64))
    PF.print_ratios(name + " loss", PF.close_to_f64(loss, l64, [r[1] for r in ref32], name + " loss", M_F64))
    PF.print_ratios(name, PF.close_to_f64(got, g64, [r[2] for r in ref32], name, M_F64))


@pytest.mark.parametrize("graphs", [48, 220])
@pytest.mark.parametrize("model_name,K,L,H", [("KPGINPlus", 4, 4, 32), ("KPGIN", 3, 3, 24)])
def test_bodies_vs_float64(model_name, K, L, H, graphs, monkeypatch):
    """virtual_node=True, residual, JK concat, no dropout; score, loss and every parameter gradient through close_to_f64 with
    M = 3 against the float64 oracle (fp32 oracle at 4, 8 and 16 threads as the yardstick).  48 molecules: the small-batch
    gathers, 48 rows in the virtual-node MLP; 220: N = 5148 >= 4096, the large-batch paths and the pull gather over states
    that the virtual node replaced.  Measured on the MI355X (E32 / gscale of the gradients; largest ratio
    |ours - float64| / max(e32_k, 0.1 E32) over the gradient tensors, then the score's and the loss's):
        KP-GIN+ K4 L4 h32   48 graphs   1.9e-7   0.83 (regressor.weight)         0.83   0.39
        KP-GIN+ K4 L4 h32  220 graphs   3.3e-5   0.08 (regressor.weight)         0.48   0.26
        KP-GIN  K3 L3 h24   48 graphs   3.0e-7   1.00 (output_proj.0.weight)     0.76   0.59
        KP-GIN  K3 L3 h24  220 graphs   6.9e-7   3.02 (output_proj.0.weight)     0.61   0.06
    The 3.02 is the jumping-knowledge projection's weight gradient: its error is 4.0e-6 of max |dW| (the same body without the
    virtual node: 6.9e-6, and both unchanged under set_dense_math("f32")), three times the fp32 oracle's own for that tensor, and
    under the golden floor that close_to_f64 keeps; the fp32 oracle as a whole sits only 6.9e-7 from float64 here."""
    from kp_gnn_amd import _lib, ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = _vn_model(model_name, K, L, H)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(graphs, seed0=11, K=K)
    ref64, ref32 = _refs(sd, host, model_name=model_name, K=K, L=L)
    model = model.to(dev).train()
    b = host.to(dev)
    b.build_csr()
    N = b.num_nodes
    assert (N >= 4096) == (graphs == 220) and b.num_graphs == graphs
    launches, pulls = [], []
    real, real_pull = _lib.launch, ops.khop_pull_gather
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    monkeypatch.setattr(ops, "khop_pull_gather", lambda *a, **k: (pulls.append(1), real_pull(*a, **k))[1])
    res = _train_step(model, b)
    monkeypatch.undo()
    assert launches.count("kpgnn_vn_add_pool") == 2 * L - 1, launches      # L forward, L - 1 backward (the last layer pools nothing)
    if model_name == "KPGINPlus" and graphs == 220:
        assert ops.pull_applies(N, H) and pulls, "the pull gather did not run over the replaced states"
    _check_f64(res, ref64, ref32, f"vn {model_name} K{K} L{L} h{H} N{N}")


@pytest.mark.parametrize("model_name", ["KPGIN", "KPGINPlus", "KPGINPrime"])
def test_bodies_with_and_without_num_graphs_vs_float64(model_name):
    """K = 3, L = 3 on a handful of molecules: a batch that carries num_graphs (no host read-back in the virtual node) and the
    same batch without it give the same score and gradients within the golden tolerances, and both match the float64 oracle."""
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    K, L, H = 3, 3, 24
    model = _vn_model(model_name, K, L, H)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(7, seed0=5, K=K)
    s64, l64, g64 = _oracle(sd, host.as_dict(), host.y, torch.float64, model_name=model_name, K=K, L=L)
    model = model.to(dev).train()
    b = host.to(dev)
    b.build_csr()
    assert b.num_graphs == 7
    with_count = _train_step(model, b)
    b.num_graphs = None
    without = _train_step(model, b)
    for name, res in (("with num_graphs", with_count), ("without", without)):
        _close(res[0], s64, f"{model_name} {name}: score")
        _close(res[1], l64, f"{model_name} {name}: loss")
        _close_grads(res[2], g64, f"{model_name} {name}: gradients")
    _close(with_count[0], without[0], "score, with against without")
    _close_grads(with_count[2], without[2], f"{model_name}: gradients, with against without")


# ------------------------------------------------------------------------------------------------ 4. capture
def _dataset(n, K, seed0=21):
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


def _vn_norm_params(model):
    """mlp_virtualnode_list.*.{1,4}.{weight,bias}: finished from fp64 column sums that blocks add with atomics."""
    return {n for n, _ in model.named_parameters() if "mlp_virtualnode_list" in n and n.split(".")[-2] in ("1", "4")}


def test_training_step_is_captured_and_replays_to_the_eager_bits():
    """Forward, loss and backward of a virtual-node body in ONE torch.cuda.graph on a batch from KHopDataset.collate (which
    carries num_graphs): a host synchronisation inside the captured region would fail the capture.  The replayed score, loss
    and gradients are the eager ones bit for bit; the BatchNorm gamma / beta gradients of the virtual-node MLPs to fp64-sum
    accuracy."""
    dev = _dev()
    K, L, H = 4, 4, 32
    raw, args, ds = _dataset(64, K, seed0=5)
    model = _vn_model("KPGINPlus", K, L, H).to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    b = ds.collate([9, 3, 60, 21, 22, 23, 0, 63, 11, 40, 41, 5])
    assert b.num_graphs == 12
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(model, b)                              # warms the caches that sync (graph pointer, index range checks)
        model.load_state_dict(sd)
        loss_e, score_e, grads_e = _step(model, b)
        loss_e, score_e = loss_e.clone(), score_e.detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    model.load_state_dict(sd)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, score_g, grads_g = _step(model, b)
    model.load_state_dict(sd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(score_g.detach(), score_e) and torch.equal(loss_g, loss_e)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    loose = _vn_norm_params(model)
    assert len(loose) == 4 * (L - 1)
    for n, ge, gg in zip(names, grads_e, grads_g):
        assert (ge is None) == (gg is None), n
        if ge is None:
            continue
        if n in loose:
            assert float((ge - gg).abs().max()) <= 1e-6 * float(ge.abs().max()) + 1e-12, (n, float((ge - gg).abs().max()))
        else:
            assert torch.equal(ge, gg), (n, float((ge - gg).abs().max()))
    assert any("mlp_virtualnode_list" in n and g is not None and float(g.abs().max()) > 0 for n, g in zip(names, grads_g))


# ------------------------------------------------------------------------------------------------ 5. / 6. static batch
def _static_setup():
    dev = _dev()
    K, L, H, Bsz = 4, 4, 32, 96
    raw, args, ds = _dataset(400, K)
    model = _vn_model("KPGINPlus", K, L, H, seed=0).to(dev).train()
    sb = ds.static_batch(Bsz)
    assert sb.N_cap > int(ds.h_nodes.mean() * Bsz)
    rng = np.random.default_rng(3)
    id_sets = [rng.permutation(400)[:Bsz] for _ in range(3)]
    return dev, raw, args, ds, model, sb, id_sets, (K, L, H)


def test_static_batch_equals_exact_shapes():
    """tests/test_dataset.py::test_static_batch_dynamic_rows_equal_exact_shapes with virtual_node=True (96 graphs, three id sets
    out of 400 molecules): the exact-shape eager step against the static batch run eagerly and against ONE captured graph
    replayed on all three, under that test's tolerances.  The capacity exceeds every live count, so a phantom row in the
    virtual node's sums would show."""
    dev, raw, args, ds, model, sb, id_sets, _ = _static_setup()
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def reset():
        model.load_state_dict(sd)

    def check(got, ref, what):
        (l0, s0, g0), (l1, s1, g1) = got, ref
        assert torch.allclose(s0, s1, rtol=2e-5, atol=2e-5), what
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
        l, s_, g = _step(model, ds.collate(ids))
        refs.append((l.clone(), s_.detach().clone(), g))
    del l, s_, g
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


def test_evaluation_forward_on_a_static_batch_through_one_graph():
    """model.eval() under no_grad on the static batch through ONE captured graph, replayed on three id sets.  Bound: the one
    tests/test_eval_forward.py holds its dynamic-rows case to - close_to_f64 with M = 3 against the float64 oracle
    (training=False, virtual_node=True), the fp32 oracle at 4, 8 and 16 threads as the yardstick - applied to the
    exact-shape eval forward and to the replayed static one alike."""
    dev, raw, args, ds, model, sb, id_sets, (K, L, H) = _static_setup()
    g = torch.Generator().manual_seed(41)
    for m in model.modules():          # running statistics away from their initial 0 / 1
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.copy_(0.3 * torch.randn(m.num_features, generator=g))
            m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    model.eval()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    refs = []
    for ids in id_sets:
        host = raw.subset(ids).collated(args)
        kw = dict(model_name="KPGINPlus", K=K, L=L, training=False)
        refs.append((_oracle(sd, host.as_dict(), host.y, torch.float64, **kw),
                     [_oracle(sd, host.as_dict(), host.y, torch.float32, threads=t, **kw) for t in PF.THREADS]))
    with torch.no_grad():
        for i, (ids, (s64, s32)) in enumerate(zip(id_sets, refs)):
            name = f"vn eval exact shape, set {i}"
            PF.print_ratios(name, PF.close_to_f64(model(ds.collate(ids)), s64, s32, name, M_F64))
        with sb.dynamic():
            sb.stage(id_sets[0])
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                sb.launch_collate()
                model(sb.batch)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                sb.launch_collate()
                score = model(sb.batch)
        for i, (ids, (s64, s32)) in enumerate(zip(id_sets, refs)):
            sb.stage(ids)
            assert sb.live[0] < sb.N_cap
            graph.replay()
            torch.cuda.synchronize()
            name = f"vn eval static batch replay, set {i}"
            PF.print_ratios(name, PF.close_to_f64(score, s64, s32, name, M_F64))
    assert not model.training
