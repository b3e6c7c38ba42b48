"""KPGraphSAGEConv and a KP-GraphSAGE body on kpgnn_sage_tail_* (ops_dense.sage_tail), on the device.

The layer with the switch on is held to the float64 CPU oracle (oracle.kp_layers_oracle.kpgraphsage_forward and its autograd)
with the fp32 oracle at PF.THREADS thread counts as the yardstick, for both combines, K == 1 and a hop too wide for the kernel;
with the switch off it is bitwise the expression the layer ran before the kernel existed (restated below).  A three-layer body
trains a step, its captured step replays the eager bits, and its kernel list holds sage_tail launches and no baddbmm."""
import argparse
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_f64 as PF

pytestmark = pytest.mark.gpu
M_F64 = 3
# (combine, K, input_size, output_size, the route the layer must decide on: 2 = one launch, 1 = tail only, 0 = framework)
LAYERS = [("geometric", 3, 33, 33, 2), ("attention", 3, 33, 33, 1), ("geometric", 1, 8, 8, 1), ("geometric", 8, 104, 40, 2),
          ("geometric", 3, 120, 120, 0)]


def _dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def _switch(on):
    from kp_gnn_amd import ops_dense
    prev = ops_dense.set_native_sage_tail(on)
    try:
        yield
    finally:
        ops_dense.set_native_sage_tail(prev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case(combine, K, I, O, seed=0):
    """A seeded CPU layer and a small random K-hop batch: 70 nodes, 600 edges, codes of both tables, live path codes,
    a peripheral term."""
    from kp_gnn_amd.layers import KPGraphSAGEConv
    N, E, n1, npe = 70, 600, 3, 10
    torch.manual_seed(100 + seed + K)
    layer = KPGraphSAGEConv(I, O, K, aggr="add", num_hop1_edge=n1, num_pe=npe, combine=combine)
    with torch.no_grad():
        if K > 1 and combine == "geometric":
            layer.combine.alphas.copy_(torch.randn(O // K))
    rng = np.random.default_rng(7 + K)
    ei = torch.from_numpy(rng.integers(0, N, size=(2, E)))
    act = rng.random((E, K)) < 0.4
    ea = np.zeros((E, K), dtype=np.int64)
    ea[:, 0] = rng.integers(2, n1 + 2, size=E) * act[:, 0]
    if K > 1:
        ea[:, 1:] = rng.integers(2, npe + 2, size=(E, K - 1)) * act[:, 1:]
    g = torch.Generator().manual_seed(seed + 31 * K)
    data = dict(x=torch.randn(N, I, generator=g), ei=ei, ea=torch.from_numpy(ea),
                pe=torch.randint(0, npe, (N, K - 1), generator=g) if K > 1 else None,
                periph=torch.randn(N, K, I // K, generator=g), gout=torch.randn(N, O, generator=g))
    return layer, data


def _oracle(sd, data, K, combine, dtype, threads=None):
    from oracle import kp_layers_oracle as LO
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        p = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
        x = data["x"].to(dtype).requires_grad_(True)
        periph = data["periph"].to(dtype).requires_grad_(True)
        out = LO.kpgraphsage_forward(p, x, data["ei"], data["ea"], data["pe"], periph, K=K, combine_kind=combine)
        names = sorted(p)
        grads = torch.autograd.grad(out, [x, periph] + [p[k] for k in names], data["gout"].to(dtype), allow_unused=True)
    finally:
        torch.set_num_threads(before)
    res = {"out": out.detach(), "dx": grads[0], "dperiph": grads[1]}
    res.update({k: (gk if gk is not None else torch.zeros_like(p[k])) for k, gk in zip(names, grads[2:])})
    return res


def _device_run(layer, data, forward=None):
    dev = _dev()
    x = data["x"].to(dev).requires_grad_(True)
    periph = data["periph"].to(dev).requires_grad_(True)
    pe = data["pe"].to(dev) if data["pe"] is not None else None
    args = (x, data["ei"].to(dev), data["ea"].to(dev), pe, periph)
    out = layer(*args) if forward is None else forward(layer, *args)
    named = dict(layer.named_parameters())
    names = sorted(named)
    grads = torch.autograd.grad(out, [x, periph] + [named[k] for k in names], data["gout"].to(dev), allow_unused=True)
    res = {"out": out.detach(), "dx": grads[0], "dperiph": grads[1]}
    res.update({k: (gk if gk is not None else torch.zeros_like(named[k])) for k, gk in zip(names, grads[2:])})
    torch.cuda.synchronize()
    return res


def _parent_forward(layer, x, edge_index, edge_attr, pe_attr, peripheral_attr):
    """KPGraphSAGEConv.forward as it stood before kpgnn_sage_tail_*: the aggregation, then library ops."""
    from kp_gnn_amd._lib import MODE_SUM
    from kp_gnn_amd.ops import khop_aggregate
    n = x.size(0)
    x = x.reshape(n, layer.K, layer.input_dk)
    csr, k_act = layer._csr(edge_index, edge_attr, n)
    x, xbias = layer._path_encoding(x, pe_attr)
    t0, tk = layer._tables()
    x_n = khop_aggregate(x, csr, k_act, MODE_SUM, table0=t0, tablek=tk, periph=peripheral_attr, xbias=xbias)
    if xbias is not None:
        x = torch.cat([x[:, :1], x[:, 1:] + xbias], dim=1)
    h = torch.cat([x, x_n], dim=-1).transpose(0, 1)
    h = torch.baddbmm(layer.hop_bias.unsqueeze(1), h, layer.hop_proj).transpose(0, 1)
    h = F.normalize(F.relu(h), p=2, dim=-1)
    return layer.combine_proj(layer.combine(h))


@pytest.mark.parametrize("combine,K,I,O,route", LAYERS)
def test_layer_vs_the_float64_oracle(combine, K, I, O, route):
    """Output and the gradients into x, the peripheral term and every parameter through close_to_f64 (M = 3); the layer took
    the route its shape calls for (an input_dk of 40 is beyond the kernel: the framework expression, same check)."""
    layer, data = _case(combine, K, I, O)
    sd = {k: v.clone() for k, v in layer.state_dict().items()}
    ref64 = _oracle(sd, data, K, combine, torch.float64)
    ref32 = [_oracle(sd, data, K, combine, torch.float32, threads=t) for t in PF.THREADS]
    layer = layer.to(_dev()).train()
    with _switch(True):
        got = _device_run(layer, data)
    assert layer._fused_tail == route
    name = f"KPGraphSAGEConv {combine} K{K} {I}->{O}"
    PF.print_ratios(name, PF.close_to_f64(got, ref64, ref32, name, M_F64))


@pytest.mark.parametrize("combine,K,I,O,route", LAYERS[:3])
def test_switch_off_is_bitwise_the_parents_expression(combine, K, I, O, route):
    layer, data = _case(combine, K, I, O, seed=1)
    layer = layer.to(_dev()).train()
    with _switch(False):
        got = _device_run(layer, data)
    want = _device_run(layer, data, forward=_parent_forward)
    assert sorted(got) == sorted(want)
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    with _switch(True):                               # and the switch does select another route: the bits differ somewhere
        native = _device_run(layer, data)
    assert any(not torch.equal(_bits(native[k]), _bits(want[k])) for k in native)


# ------------------------------------------------------------------------------------------------ body
def _body(K=3, L=3, H=33):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name="KPGraphSAGE", hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    return B.GraphRegression(gnn, "sum")


@pytest.fixture(scope="module")
def batch():
    from test_dataset import molecules
    from kp_gnn_amd.dataset import KHopDataset
    raw = molecules(48, seed0=5)
    ds = KHopDataset.from_collated(raw.collated((3, 50, 6, 3, 50, 50, "spd")), raw.node_ptr, _dev())
    return ds.collate([9, 3, 21, 22, 23, 0, 47, 11, 40, 41, 5, 30])


def _step(model, b):
    from kp_gnn_amd.ops_dense import regression_loss_and_grad
    score = model(b)
    loss, dscore = regression_loss_and_grad(score, b.y, "l1")
    params = [p for p in model.parameters() if p.requires_grad]
    grads = torch.autograd.grad(score, params, grad_outputs=dscore, allow_unused=True)
    return loss, score, [g if g is None else g.clone() for g in grads]


def test_body_trains_a_step_and_its_capture_replays_the_eager_bits(batch):
    """Three KP-GraphSAGE layers (hidden 33, K = 3, JK concat, BatchNorm): finite loss and gradients, every layer on the
    one-launch route; forward + loss + backward captured in ONE torch.cuda.graph replay to the eager step's bits."""
    dev = _dev()
    model = _body().to(dev).train()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    with _switch(True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            loss, score, grads = _step(model, batch)
            ref = (loss.clone(), score.detach().clone(), grads)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        assert all(m._fused_tail == 2 for m in model.modules() if type(m).__name__ == "KPGraphSAGEConv")
        assert sum(type(m).__name__ == "KPGraphSAGEConv" for m in model.modules()) >= 3
        assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[1]).all())
        n_grads = 0
        for (n, p), g in zip([(n, p) for n, p in model.named_parameters() if p.requires_grad], ref[2]):
            if g is not None:
                assert bool(torch.isfinite(g).all()), n
                n_grads += 1
            if n.endswith("hop_proj") or n.endswith("hop_bias") or n.endswith("combine.alphas"):
                assert g is not None and bool((g != 0).any()), n
        assert n_grads > 10
        model.load_state_dict(sd)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = _step(model, batch)
        model.load_state_dict(sd)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(_bits(out[0]), _bits(ref[0])), "loss"
    assert torch.equal(_bits(out[1].detach()), _bits(ref[1])), "score"
    for (n, _), a, b in zip([(n, p) for n, p in model.named_parameters() if p.requires_grad], out[2], ref[2]):
        assert (a is None) == (b is None), n
        if a is not None:
            assert torch.equal(_bits(a), _bits(b)), n


def _op_and_launch_names(model, b):
    """(framework op names, device kernel names, C-ABI launch names) of one training step."""
    from kp_gnn_amd import _lib
    from torch.profiler import ProfilerActivity, profile
    launches, real = [], _lib.launch

    def spy(name, *a, **k):
        launches.append(name)
        return real(name, *a, **k)

    _lib.launch = spy
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _step(model, b)
            torch.cuda.synchronize()
    finally:
        _lib.launch = real
    events = prof.events()
    ops = {e.name for e in events if e.device_type == torch.autograd.DeviceType.CPU}
    kernels = {e.name for e in events if e.device_type != torch.autograd.DeviceType.CPU}
    return ops, kernels, launches


def test_a_step_launches_the_kernel_and_no_baddbmm(batch):
    """With the switch on a step's C-ABI launches hold one kpgnn_sage_tail_fwd and one _bwd per layer, the device kernel list
    (when the profiler records device activity) names sage_tail kernels, and no aten::baddbmm / bmm / cat-of-[x, x_n] tail op
    runs; with it off aten::baddbmm is there (so the check can tell the two apart)."""
    model = _body().to(_dev()).train()
    with _switch(True):
        _step(model, batch)
        ops, kernels, launches = _op_and_launch_names(model, batch)
    assert launches.count("kpgnn_sage_tail_fwd") == 3 and launches.count("kpgnn_sage_tail_bwd") == 3, launches
    assert "aten::baddbmm" not in ops and "aten::bmm" not in ops, sorted(o for o in ops if "mm" in o)
    assert not any("baddbmm" in k.lower() for k in kernels)
    if kernels:
        assert any("sage_tail_fwd_kernel" in k for k in kernels) and any("sage_tail_bwd_kernel" in k for k in kernels), kernels
    with _switch(False):
        _step(model, batch)
        ops, kernels, launches = _op_and_launch_names(model, batch)
    assert "aten::baddbmm" in ops and not any("sage_tail" in n for n in launches)
    assert not any("sage_tail" in k for k in kernels)
