"""GPU (-m gpu): the bodies' rd projection on kpgnn_rd_proj_fwd / _bwd (csrc/rd_proj.hip) through ops.rd_project and the
bodies' _inputs: parity with the framework expression in float64 (ops.rd_project_reference) at the golden tolerances of
tests/parity_f64.py, bitwise repeatability, a capacity-shaped call under dynamic_rows with poisoned dead rows - which the
framework Linear(1, H) cannot survive: its weight and bias gradients sum over every row -, the fallback for H > 256, and
two bodies with use_rd=True against the float64 CPU oracle, eagerly and from one captured graph on a StaticBatch."""
import argparse
import functools

import numpy as np
import pytest
import torch

import parity_f64 as PF

pytestmark = pytest.mark.gpu

RTOL, ATOL = PF.RTOL, PF.ATOL      # the golden tolerances: |got - ref| <= ATOL * max|ref| + RTOL * |ref|
FWD, BWD = "kpgnn_rd_proj_fwd", "kpgnn_rd_proj_bwd"
NS, HS = (1, 63, 257, 1000), (1, 104, 120, 256)
NAN = float("nan")


def _dev():
    return torch.device("cuda:0")


def _close(got, ref, name):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    bound = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    print(f"rd_proj {name}: max err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    assert bool((err <= bound).all()), (name, float(err.max()))


@functools.lru_cache(maxsize=None)
def _case(N, H):
    """Inputs and the float64 reference (forward, dx, dw, db) of one shape, on the CPU; computed once, never modified."""
    from kp_gnn_amd import ops
    g = torch.Generator().manual_seed(1000 * N + H)
    x, dy = torch.randn(N, H, generator=g), torch.randn(N, H, generator=g)
    rd = 3.0 * torch.rand(N, 1, generator=g)            # resistance distances: non-negative, a few units
    w, b = torch.randn(H, 1, generator=g), torch.randn(H, generator=g)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    out = ops.rd_project_reference(xr, rd, wr, br)
    assert out.dtype == torch.float64
    (out * dy.double()).sum().backward()
    return (x, rd, w, b, dy), {"out": out.detach(), "dx": xr.grad.double(), "dw": wr.grad.double(), "db": br.grad.double()}


def _native(x, rd, w, b, dy):
    """One forward and backward through ops.rd_project on the device; every tensor detached."""
    from kp_gnn_amd import ops
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    assert ops.rd_project_applies(xr, rd, wr, br)
    out = ops.rd_project(xr, rd, wr, br)
    out.backward(dy)
    return {"out": out.detach(), "dx": xr.grad, "dw": wr.grad, "db": br.grad}


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("N", NS)
def test_parity_with_float64_and_bitwise_repeatable(N, H, monkeypatch):
    from test_jk import _record
    dev = _dev()
    ins, ref = _case(N, H)
    ins = [t.to(dev) for t in ins]
    launches = _record(monkeypatch)
    got = _native(*ins)
    assert launches == [FWD, BWD], launches
    again = _native(*ins)
    torch.cuda.synchronize()
    assert got["out"].dtype == torch.float32 and tuple(got["dw"].shape) == (H, 1) and tuple(got["db"].shape) == (H,)
    for k in ("out", "dx", "dw", "db"):
        _close(got[k], ref[k], f"N{N} H{H} {k}")
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k
    assert torch.equal(got["dx"], ins[4])                # dx is dy itself


def test_other_layouts_and_no_grad(monkeypatch):
    """rd as [N], a column slice of a wider x (a view, unit column stride), an expanded upstream gradient; under no_grad one
    forward launch and no autograd node."""
    from test_jk import _record
    from kp_gnn_amd import ops
    dev = _dev()
    (x, rd, w, b, dy), ref = _case(257, 104)
    wide = torch.randn(257, 150).to(dev)
    wide[:, 3:107] = x.to(dev)
    xs = wide[:, 3:107]
    assert not xs.is_contiguous()
    rd, w, b = rd.to(dev), w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = ops.rd_project(xs, rd.reshape(-1), w, b)
    _close(out, ref["out"], "strided x")
    out.sum().backward()                                 # the upstream gradient is an expanded scalar
    _close(w.grad, rd.cpu().double().sum().expand(104).reshape(104, 1), "dw of ones")
    _close(b.grad, torch.full((104,), 257.0, dtype=torch.float64), "db of ones")
    launches = _record(monkeypatch)
    with torch.no_grad():
        ev = ops.rd_project(xs, rd, w, b)
    assert launches == [FWD] and ev.grad_fn is None and torch.equal(ev, out.detach())
    plain = ops.rd_project(xs, rd, w.detach(), b.detach())        # nothing asks for a gradient: no node either
    assert plain.grad_fn is None and launches == [FWD, FWD]


@pytest.mark.parametrize("cap,live,H", [(300, 1, 104), (300, 63, 120), (300, 257, 104), (300, 299, 120), (300, 257, 1),
                                        (300, 257, 256), (4500, 4200, 256), (4500, 2049, 120)])
def test_dynamic_rows_with_poisoned_dead_rows(cap, live, H):
    """Capacity `cap`, `live` rows alive, the dead rows of x, rd and dy NaN, every torch.empty of the wrappers NaN-filled
    (tests/test_dynamic_rows_training.py's harness): the live rows of out, dw and db are the bits of the exact-shape call on
    [:live] - the sums do not depend on the capacity -, dw and db are finite, the dead rows of out keep their poison.  The
    framework Linear(1, H) of the parent commit sums dw and db over all `cap` rows: one NaN there poisons the step.
    (4500, 4200, 256) and (4500, 2049, 120) have more rows than one pass of the 256 statistics blocks covers.)"""
    from test_dynamic_rows_training import _dead, _dynamic
    dev = _dev()
    g = torch.Generator().manual_seed(cap + live + H)
    x, dy = torch.randn(cap, H, generator=g), torch.randn(cap, H, generator=g)
    rd = 3.0 * torch.rand(cap, 1, generator=g)
    w, b = torch.randn(H, 1, generator=g).to(dev), torch.randn(H, generator=g).to(dev)
    exact = _native(x[:live].to(dev), rd[:live].to(dev), w, b, dy[:live].to(dev))
    for t in (x, rd, dy):
        t[live:] = NAN
    x, rd, dy = x.to(dev), rd.to(dev), dy.to(dev)
    with _dynamic(live, cap):
        got = _native(x, rd, w, b, dy)
    for k in ("dw", "db"):
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k].view(torch.int32), exact[k].view(torch.int32)), k
    assert torch.equal(got["out"][:live].view(torch.int32), exact["out"].view(torch.int32))
    _dead(got["out"], live, NAN, "out")
    # the framework expression on the same tensors: what a capacity-shaped batch got before
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (x + torch.nn.functional.linear(rd, wr, br)).backward(dy)
    assert not bool(torch.isfinite(wr.grad).all()) and not bool(torch.isfinite(br.grad).all())


def test_wide_rows_fall_back_outside_dynamic_rows_and_raise_inside(monkeypatch):
    from test_jk import _record
    from kp_gnn_amd import _lib, ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    N, H = 40, 257
    x, rd = torch.randn(N, H, generator=g).to(dev), torch.rand(N, 1, generator=g).to(dev)
    w, b = torch.randn(H, 1, generator=g).to(dev).requires_grad_(True), torch.randn(H, generator=g).to(dev).requires_grad_(True)
    assert not ops.rd_project_applies(x, rd, w, b)
    launches = _record(monkeypatch)
    out = ops.rd_project(x, rd, w, b)
    assert launches == [] and torch.equal(out, x + torch.nn.functional.linear(rd, w, b).squeeze())
    cnt = torch.tensor([30], dtype=torch.int32, device=dev)
    with ops.dynamic_rows(cnt, N), pytest.raises(_lib.KpgnnError, match="dynamic row count"):
        ops.rd_project(x, rd, w, b)
    # the switch: off keeps the framework expression on exact shapes, and is overruled inside a dynamic_rows block
    x, w, b = x[:, :120].contiguous(), w[:120].detach().requires_grad_(True), b[:120].detach().requires_grad_(True)
    prev = ops.set_native_rd_proj(False)
    try:
        assert not ops.rd_project_applies(x, rd, w, b)
        assert torch.equal(ops.rd_project(x, rd, w, b), x + torch.nn.functional.linear(rd, w, b).squeeze()) and launches == []
        with ops.dynamic_rows(cnt, N):
            assert ops.rd_project_applies(x, rd, w, b)
            ops.rd_project(x, rd, w, b)
        assert launches == [FWD]
    finally:
        ops.set_native_rd_proj(prev)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ bodies
# The issue names a body of K = 3, L = 2, H = 16.  KP-GIN (the GNN class) splits H over its K hops and asserts H % K == 0, so that
# shape exists for the GNNPlus body alone: it runs at (3, 2, 16) and the GNN body at (3, 2, 18), the next width KP-GIN accepts.
BODIES = [("KPGINPlus", 3, 2, 16), ("KPGIN", 3, 2, 18)]


def _model(model_name, K, L, H, seed=3):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(seed)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=True,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    return B.GraphRegression(gnn, "sum")


class _FWithRd:
    """torch.nn.functional for the oracle (oracle/kp_model_oracle.py has no use_rd): its input embedding gains the reference's
    `x = x + self.rd_projection(data.rd)` (models/GNNs.py), everything else passes through."""

    def __init__(self, p, rd):
        self.p, self.rd = p, rd

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def embedding(self, idx, weight, *a, **k):
        out = torch.nn.functional.embedding(idx, weight, *a, **k)
        if weight is self.p["embedding_model.init_proj.init_proj.weight"]:
            lin = torch.nn.functional.linear(self.rd, self.p["embedding_model.rd_projection.weight"],
                                             self.p["embedding_model.rd_projection.bias"])
            out = out + lin.reshape(out.shape)
        return out


def _oracle_f64(sd, data, rd, y, model_name, K, L, monkeypatch):
    """The float64 CPU run of the same module: PF.oracle_body's steps with the rd projection in place."""
    from oracle import kp_model_oracle as MO
    kind, layer_kind = PF.BODY_KIND[model_name]
    dt = torch.float64
    p = {k: (v.detach().to(dt).clone().requires_grad_(True) if PF.trainable(k, v) else PF.to_dtype(v.detach(), dt).clone())
         for k, v in sd.items()}
    monkeypatch.setattr(MO, "F", _FWithRd(p, rd.to(dt)))
    score = MO.graph_regression_forward(p, data, kind=kind, layer_kind=layer_kind, K=K, num_layer=L, combine_kind="geometric",
                                        JK="concat", residual=True, training=True)
    monkeypatch.undo()
    loss = (score.squeeze() - y.to(dt).squeeze()).abs().mean()
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items() if v.requires_grad}
    return score.detach(), loss.detach(), grads


@pytest.mark.parametrize("model_name,K,L,H", BODIES)
def test_body_with_rd_against_the_float64_oracle(model_name, K, L, H, monkeypatch):
    """Score, loss and EVERY parameter gradient of a use_rd body on a collated batch that carries rd, against the float64 CPU
    run, at the golden tolerances; the rd projection makes one launch per direction and its parameters get a gradient."""
    from test_jk import _close_grads, _record, _train_step
    from kp_gnn_amd.batch import synthetic_zinc_batch
    from kp_gnn_amd.khop_transform import resistance_distance_host
    dev = _dev()
    model = _model(model_name, K, L, H)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(24, seed0=11, K=K)
    ei = host.edge_index.numpy()
    rd = torch.cat([torch.from_numpy(resistance_distance_host(
        host.node_ptr[g + 1] - host.node_ptr[g], ei[:, host.edge_ptr[g]:host.edge_ptr[g + 1]] - host.node_ptr[g]))
        for g in range(24)]).float().reshape(-1, 1)
    ref = _oracle_f64(sd, host.as_dict(), rd, host.y, model_name, K, L, monkeypatch)
    model = model.to(dev).train()
    b = host.to(dev)
    b.rd = rd.to(dev)
    b.build_csr()
    launches = _record(monkeypatch)
    score, loss, got = _train_step(model, b)
    monkeypatch.undo()
    assert launches.count(FWD) == 1 and launches.count(BWD) == 1, launches
    name = f"rd body {model_name} K{K} L{L} h{H} N{b.num_nodes}"
    _close(score, ref[0], name + " score")
    _close(loss, ref[1], name + " loss")
    _close_grads(got, ref[2], name)
    for k in ("embedding_model.rd_projection.weight", "embedding_model.rd_projection.bias"):
        assert float(ref[2][k].abs().max()) > 0 and float(got[k].abs().max()) > 0, k
    # without rd on the batch the projection is skipped, as in the reference
    del b.rd
    del launches[:]
    launches = _record(monkeypatch)
    model(b)
    assert FWD not in launches


def test_captured_step_on_a_static_batch_replays_to_the_eager_exact_shape_results():
    """A use_rd body on a dataset built with_rd=True: ONE torch.cuda.graph of collate + forward + loss + backward on a StaticBatch
    inside sb.dynamic(), replayed for two different id sets, against the eager step on the exact-shape collate of the same ids
    (golden tolerances).  The capacity exceeds both live counts, so a dead row of rd - uninitialised memory - would show.
    H = 64 here, K and L as above: inside a dynamic_rows block the layers' MLPs run on the fused Linear+BatchNorm kernels alone,
    whose widths start at 32 (ops_dense._LIN_WIDTHS), and the jumping-knowledge projection on the grouped-K kernels, which want
    (L + 1) * H > 128 - at H = 16 or 32 the body refuses the capacity-shaped batch before rd matters."""
    from test_dataset import _step, molecules
    from test_jk import _close_grads
    from kp_gnn_amd.dataset import KHopDataset
    dev = _dev()
    model_name, K, L, H = "KPGINPlus", 3, 2, 64
    raw = molecules(64, seed0=5)
    ds = KHopDataset.from_collated(raw.collated((K, 50, 6, 3, 50, 50, "spd")), raw.node_ptr, dev, with_rd=True)
    model = _model(model_name, K, L, H).to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    rng = np.random.default_rng(3)
    id_sets = [rng.permutation(64)[:16] for _ in range(2)]
    params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    names = [n for n, _ in params]
    named = lambda gs: {n: (torch.zeros_like(p) if q is None else q) for (n, p), q in zip(params, gs)}  # noqa: E731
    refs = []
    for ids in id_sets:
        model.load_state_dict(sd)
        b = ds.collate(ids)
        assert tuple(b.rd.shape) == (b.x.shape[0], 1)
        l, s, g = _step(model, b)
        refs.append((l.clone(), s.detach().clone(), g))
    del l, s, g
    sb = ds.static_batch(16)
    with sb.dynamic():
        model.load_state_dict(sd)
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
    for i, (ids, ref) in enumerate(zip(id_sets, refs)):
        model.load_state_dict(sd)
        sb.stage(ids)
        assert sb.live[0] < sb.N_cap
        graph.replay()
        torch.cuda.synchronize()
        _close(out[1], ref[1], f"replay {i} score")
        _close(out[0], ref[0], f"replay {i} loss")
        assert all(q is None or bool(torch.isfinite(q).all()) for q in out[2])
        _close_grads(named(out[2]), named(ref[2]), f"replay {i} gradients")
    rdw = names.index("embedding_model.rd_projection.weight")
    assert float(out[2][rdw].abs().max()) > 0
