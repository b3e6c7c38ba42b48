"""GPU (-m gpu): the task heads on their native kernels - attention readout (kpgnn_attn_pool_*), narrow-output Linear
(kpgnn_head_linear_*) and the classification loss (kpgnn_nll_loss) - and the modules GraphClassification / NodeClassification /
NodeRegression / GraphRegression("attention") built on them, against float64 on the CPU.

References are restated here in torch on the CPU (index_add_ pooling, the per-graph softmax, F.linear, F.log_softmax, F.nll_loss)
and evaluated in float64; the fp32 yardstick is the same code in fp32 at parity_f64.THREADS threads.  Two bounds, both the
project's own: forward outputs and per-row gradients meet the kernel-level bound of tests/test_eval_forward.py,
|got - ref| <= ATOL * max|ref| + RTOL * |ref|; parameter gradients of one case go, in one dict, through parity_f64.close_to_f64
with M = 3 (the gate bias gradient is analytically zero, ~1e-15 in float64: the shared gscale's floor term carries it).  The code
under test never enters a bound."""
import ctypes
import functools
import math
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import parity_f64 as PF

pytestmark = pytest.mark.gpu

M_F64 = 3            # tests/test_gpu_parity.py explains the value
SENTINEL = -777.25


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _assert_close(got, ref, name):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), name
    err = (got - ref).abs()
    bound = PF.ATOL * float(ref.abs().max()) + PF.RTOL * ref.abs()
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"[heads] {name}: max|err| {float(err.max()):.3e}  max|ref| {float(ref.abs().max()):.3e}  err/bound {worst:.3f}")
    assert bool((err <= bound).all()), (name, float(err.max()), worst)


def _at_threads(fn, dtype, threads):
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        return fn(dtype)
    finally:
        torch.set_num_threads(before)


def _f64_and_f32(fn):
    """(fn(float64), [fn(float32) at 4, 8 and 16 threads])."""
    return _at_threads(fn, torch.float64, None), [_at_threads(fn, torch.float32, t) for t in PF.THREADS]


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


class _Spies:
    """Names of the C-ABI launches, and the framework calls F.linear / Tensor.index_add_ / F.log_softmax, made while installed."""

    def __init__(self, monkeypatch):
        from kp_gnn_amd import _lib
        self.launches, self.linear, self.index_add, self.log_softmax = [], [], [], []
        real_launch, real_lin, real_ia, real_ls = _lib.launch, F.linear, torch.Tensor.index_add_, F.log_softmax

        def launch(name, *a, **k):
            self.launches.append(name)
            return real_launch(name, *a, **k)

        def linear(x, *a, **k):
            self.linear.append(tuple(x.shape))
            return real_lin(x, *a, **k)

        def index_add_(t, *a, **k):
            self.index_add.append(tuple(t.shape))
            return real_ia(t, *a, **k)

        def log_softmax(x, *a, **k):
            self.log_softmax.append(tuple(x.shape))
            return real_ls(x, *a, **k)

        monkeypatch.setattr(_lib, "launch", launch)
        monkeypatch.setattr(torch.nn.functional, "linear", linear)
        monkeypatch.setattr(torch.Tensor, "index_add_", index_add_)
        monkeypatch.setattr(torch.nn.functional, "log_softmax", log_softmax)

    def no_framework_calls(self):
        return self.linear == [] and self.index_add == [] and self.log_softmax == []


# ------------------------------------------------------------------------------------------------------ attention readout
def _sizes(which):
    if which == "edges":
        return [1, 0, 7, 64, 65, 3, 0]          # empty graphs mid-batch and last; sizes around the wave width
    if which == "big":
        return [200, 1, 1, 130]
    if which == "many":
        return [23] * 40 + [0] + [37] * 30
    g = torch.Generator().manual_seed(17)        # "grid": more graphs than one grid wave of lane groups
    return torch.randint(15, 38, (300,), generator=g).tolist()


def _attn_ref(x, w, b, batch, G, gout, dtype):
    """(out, alpha, dx), {w, b gradients} of the attention readout in `dtype` on the CPU."""
    x = x.to(dtype).requires_grad_(True)
    w = w.to(dtype).requires_grad_(True)
    b = b.to(dtype).requires_grad_(True)
    gate = F.linear(x, w, b).reshape(-1)
    mx = gate.new_full((G,), float("-inf")).scatter_reduce(0, batch, gate.detach(), reduce="amax")
    e = (gate - mx[batch]).exp()
    alpha = e / (torch.zeros(G, dtype=dtype).index_add_(0, batch, e)[batch] + 1e-16)
    out = torch.zeros(G, x.shape[1], dtype=dtype).index_add_(0, batch, alpha.unsqueeze(-1) * x)
    (out * gout.to(dtype)).sum().backward()
    return (out.detach(), alpha.detach(), x.grad), {"w": w.grad, "b": b.grad}


@functools.lru_cache(maxsize=None)
def _attn_case(D, which, gate_scale=None):
    sizes = _sizes(which)
    g = torch.Generator().manual_seed(1000 + D + len(sizes))
    batch, G = _batch_of(sizes), len(sizes)
    N = int(batch.numel())
    x = torch.relu(torch.randn(N, D, generator=g))           # many exact zeros, as the body's output has
    w = torch.randn(1, D, generator=g) / math.sqrt(D)
    b = torch.randn(1, generator=g)
    if gate_scale is not None:
        w = w * (gate_scale / float((x @ w.t()).abs().max()))
    gout = torch.randn(G, D, generator=g)
    ref64, ref32 = _f64_and_f32(lambda dt: _attn_ref(x, w, b, batch, G, gout, dt))
    return dict(sizes=sizes, batch=batch, G=G, N=N, x=x, w=w, b=b, gout=gout, ref64=ref64, ref32=ref32)


def _attn_run(c, dev):
    """out, alpha and twice the gradients (x, w, b) of ops.attention_pool on the device."""
    from kp_gnn_amd import ops
    lin = nn.Linear(c["x"].shape[1], 1).to(dev)
    with torch.no_grad():
        lin.weight.copy_(c["w"])
        lin.bias.copy_(c["b"])
    x = c["x"].to(dev).requires_grad_(True)
    out, alpha = ops.attention_pool(x, c["batch"].to(dev), c["G"], lin, return_alpha=True)
    gout = c["gout"].to(dev)
    g1 = torch.autograd.grad(out, [x, lin.weight, lin.bias], gout, retain_graph=True)
    g2 = torch.autograd.grad(out, [x, lin.weight, lin.bias], gout)
    torch.cuda.synchronize()
    return out, alpha, g1, g2


def _attn_check(c, name):
    out, alpha, g1, g2 = _attn_run(c, _dev())
    (o64, a64, dx64), p64 = c["ref64"]
    _assert_close(out, o64, name + " out")
    _assert_close(alpha, a64, name + " alpha")
    _assert_close(g1[0], dx64, name + " dx")
    for g, s in enumerate(c["sizes"]):
        if s == 0:
            assert torch.equal(out[g], torch.zeros_like(out[g])), (name, g)      # an empty graph: exactly zero, no NaN
    got = {"w": g1[1], "b": g1[2]}
    PF.print_ratios(name, PF.close_to_f64(got, p64, [r[1] for r in c["ref32"]], name, M_F64))
    for a, b in zip(g1, g2):
        assert torch.equal(a, b), name                               # run to run: the same bits


@pytest.mark.parametrize("which", ["edges", "big", "many", "grid"])
@pytest.mark.parametrize("D", [32, 33, 48, 104, 128])
def test_attention_pool_vs_float64(D, which):
    _attn_check(_attn_case(D, which), f"attn_pool D{D} {which}")


@pytest.mark.parametrize("D", [130, 201, 256])
def test_attention_pool_rows_wider_than_a_sub_group(D):
    """A graph's sub-group is at most one wave: D = 130 (two columns per lane) takes 2 column chunks per lane, D = 201 (one
    column per lane) takes 4 with the last one partly filled, D = 256 fills 64 lanes x 4 columns - the documented limit."""
    _attn_check(_attn_case(D, "edges"), f"attn_pool D{D} edges")


def test_attention_pool_with_large_gates():
    """|gate| reaches about 100: exp(gate) overflows fp32 without the maximum subtracted."""
    c = _attn_case(48, "edges", 100.0)
    assert 99.0 < float((c["x"] @ c["w"].t()).abs().max()) < 101.0
    _attn_check(c, "attn_pool D48 edges |gate|~100")


# ------------------------------------------------------------------------------------------------------ narrow-output Linear
def _lin_ref(x, w, b, dy, dtype):
    x = x.to(dtype).requires_grad_(True)
    w = w.to(dtype).requires_grad_(True)
    b = None if b is None else b.to(dtype).requires_grad_(True)
    y = F.linear(x, w, b)
    (y * dy.to(dtype)).sum().backward()
    grads = {"W": w.grad}
    if b is not None:
        grads["b"] = b.grad
    return (y.detach(), x.grad), grads


@functools.lru_cache(maxsize=None)
def _lin_case(I, O, M, bias=True):
    g = torch.Generator().manual_seed(2000 + I * 37 + O * 5 + M)
    x = torch.relu(torch.randn(M, I, generator=g))
    w = torch.randn(O, I, generator=g) / math.sqrt(I)
    b = torch.randn(O, generator=g) if bias else None
    dy = torch.randn(M, O, generator=g)
    ref64, ref32 = _f64_and_f32(lambda dt: _lin_ref(x, w, b, dy, dt))
    return dict(x=x, w=w, b=b, dy=dy, ref64=ref64, ref32=ref32)


def _lin_module(c, dev):
    O, I = c["w"].shape
    lin = nn.Linear(I, O, bias=c["b"] is not None).to(dev)
    with torch.no_grad():
        lin.weight.copy_(c["w"])
        if c["b"] is not None:
            lin.bias.copy_(c["b"])
    return lin


def _lin_check(c, name, monkeypatch):
    from kp_gnn_amd import ops_dense
    dev = _dev()
    lin = _lin_module(c, dev)
    params = [lin.weight] + ([lin.bias] if lin.bias is not None else [])
    x = c["x"].to(dev).requires_grad_(True)
    dy = c["dy"].to(dev)
    spies = _Spies(monkeypatch)
    y = ops_dense.head_linear(x, lin)
    fwd = list(spies.launches)
    g1 = torch.autograd.grad(y, [x] + params, dy, retain_graph=True)
    bwd = spies.launches[len(fwd):]
    g2 = torch.autograd.grad(y, [x] + params, dy)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert fwd == ["kpgnn_head_linear_fwd"] and bwd == ["kpgnn_head_linear_bwd"], (fwd, bwd)
    assert spies.no_framework_calls(), (spies.linear, spies.index_add)
    (y64, dx64), p64 = c["ref64"]
    _assert_close(y, y64, name + " y")
    _assert_close(g1[0], dx64, name + " dx")
    got = {"W": g1[1]}
    if lin.bias is not None:
        got["b"] = g1[2]
    PF.print_ratios(name, PF.close_to_f64(got, p64, [r[1] for r in c["ref32"]], name, M_F64))
    for a, b in zip(g1, g2):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("M", [1, 77, 5000])
@pytest.mark.parametrize("I,O", [(32, 2), (48, 10), (104, 15), (128, 6), (96, 1), (33, 3), (416, 4)])
def test_head_linear_vs_float64(I, O, M, monkeypatch):
    """One row, a partial tile, and 5000 rows: 40 row tiles of 128, whose partial slabs the second launch adds.  I = 33: one
    column per lane; I = 416: two chunks of the 64 lanes x 4 columns a row's sub-group spans."""
    _lin_check(_lin_case(I, O, M), f"head_linear I{I} O{O} M{M}", monkeypatch)


def test_head_linear_without_bias(monkeypatch):
    _lin_check(_lin_case(48, 10, 5000, bias=False), "head_linear I48 O10 M5000 nobias", monkeypatch)


def test_head_linear_with_many_outputs(monkeypatch):
    """17 .. 32 outputs take the 32-output instantiation of the backward (two columns per lane at the most)."""
    _lin_check(_lin_case(128, 32, 333), "head_linear I128 O32 M333", monkeypatch)


def test_head_linear_at_its_limits(monkeypatch):
    """O = 32, I = 1024: W takes 128 KB of LDS in the forward (beyond the 64 KB a launch gets without asking), four column chunks
    per row in both directions."""
    _lin_check(_lin_case(1024, 32, 77), "head_linear I1024 O32 M77", monkeypatch)


@pytest.mark.parametrize("width", [16, 64, 128])
def test_a_width_mismatch_raises_on_the_device(width):
    """x narrower or wider than the Linear's in_features never reaches a kernel (which would index W with x's width): the module
    raises the framework's shape error, as on the CPU.  width = 128 is NodeClassification's classifier under JK == "concat"
    (hidden_size * (num_layer + 1) inputs) on a body that returns hidden_size = 32 columns."""
    from kp_gnn_amd import body as B, ops, ops_dense
    dev = _dev()
    x = torch.randn(50, 32, device=dev)
    batch = torch.zeros(50, dtype=torch.long, device=dev)
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        ops_dense.head_linear(x, nn.Linear(width, 4).to(dev))
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        ops.attention_pool(x, batch, 1, nn.Linear(width, 1).to(dev))
    if width == 128:
        model = B.NodeClassification(StubBody(x, JK="concat", num_layer=3), 4).to(dev)
        assert model.classifier.in_features == 128
        data = types.SimpleNamespace(batch=batch, num_graphs=1)
        with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
            model(data)
        with torch.no_grad(), pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
            model.eval()(data)
    with pytest.raises(ops_dense._lib.KpgnnError, match="columns"):           # the autograd functions themselves refuse too
        ops_dense.HeadLinear.apply(x, torch.zeros(4, width, device=dev), None)
    with pytest.raises(ops_dense._lib.KpgnnError, match="columns"):
        ops.AttentionPool.apply(x, torch.zeros(1, width, device=dev), None, torch.tensor([0, 50], dtype=torch.int32, device=dev), 1)


# ------------------------------------------------------------------------------------------------------ classification loss
def _nll_ref(logits, y, reduction, dtype):
    lg = logits.to(dtype).requires_grad_(True)
    loss = F.nll_loss(F.log_softmax(lg, -1), y, reduction=reduction)
    loss.backward()
    return loss.detach(), lg.grad


@functools.lru_cache(maxsize=None)
def _nll_case(C, M, scale=3.0, ignore=False):
    g = torch.Generator().manual_seed(3000 + C * 11 + M)
    logits = scale * torch.randn(M, C, generator=g)
    y = torch.randint(0, C, (M,), generator=g)
    if ignore:
        y[M // 3] = -100
    top2 = logits.topk(2, dim=1).values
    assert bool((top2[:, 0] > top2[:, 1]).all())             # no tied maxima: the arg-max is unambiguous
    return dict(logits=logits, y=y, ref={r: _nll_ref(logits, y, r, torch.float64) for r in ("mean", "sum")})


def _nll_check(c, reduction, name, monkeypatch):
    from kp_gnn_amd import ops_dense
    dev = _dev()
    lg = c["logits"].to(dev).requires_grad_(True)
    y = c["y"].to(dev)
    spies = _Spies(monkeypatch)
    loss = ops_dense.classification_loss(lg, y, reduction)
    one = list(spies.launches)
    (dl,) = torch.autograd.grad(loss, [lg])
    loss2, dl2 = ops_dense.classification_loss_and_grad(lg, y, reduction)
    lsum, correct = ops_dense.classification_eval(lg, y)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert one == ["kpgnn_nll_loss"] and spies.launches == ["kpgnn_nll_loss"] * 3, spies.launches     # the backward launches nothing
    assert spies.no_framework_calls(), spies.log_softmax
    l64, d64 = c["ref"][reduction]
    _assert_close(loss, l64, name + " loss")
    _assert_close(dl, d64, name + " dlogits")
    _assert_close(lsum, c["ref"]["sum"][0], name + " loss sum")
    assert torch.equal(loss, loss2) and torch.equal(dl, dl2), name
    assert correct.dtype == torch.int32 and int(correct) == int((c["logits"].argmax(1) == c["y"]).sum()), name


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("M", [1, 128, 5000])
@pytest.mark.parametrize("C", [2, 10, 15, 33])
def test_nll_loss_vs_float64(C, M, reduction, monkeypatch):
    _nll_check(_nll_case(C, M), reduction, f"nll_loss C{C} M{M} {reduction}", monkeypatch)


def test_nll_loss_with_large_logits(monkeypatch):
    _nll_check(_nll_case(10, 128, scale=150.0), "mean", "nll_loss C10 M128 logits x50", monkeypatch)


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_nll_loss_skips_an_ignored_label(reduction, monkeypatch):
    """A -100 label against F.nll_loss's ignore_index: no term, a zero gradient row, not in the mean's denominator."""
    c = _nll_case(15, 128, ignore=True)
    _nll_check(c, reduction, f"nll_loss C15 M128 ignore {reduction}", monkeypatch)
    assert float(c["ref"][reduction][1][128 // 3].abs().max()) == 0.0


def test_nll_loss_of_an_empty_batch():
    """M = 0 through the descriptor: accepted, a sum of exactly 0 and no correct row; nothing else is touched."""
    from kp_gnn_amd import _lib
    dev = _dev()
    loss = torch.full((), SENTINEL, device=dev)
    correct = torch.full((), 77, dtype=torch.int32, device=dev)
    d = _lib.NllLossDesc()
    d.M, d.C, d.reduction = 0, 10, 1
    d.loss, d.correct = loss.data_ptr(), correct.data_ptr()
    _lib.launch("kpgnn_nll_loss", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and int(correct) == 0


# ------------------------------------------------------------------------------------------------------ dynamic rows
CAP = 203


def _dyn_sizes(count):
    sizes, left = [], count
    for s in [1, 40, 0, 65, 33, 64]:
        take = min(s, left)
        sizes.append(take)
        left -= take
    sizes[-1] += left
    assert sum(sizes) == count
    return sizes


@pytest.mark.parametrize("count", [1, CAP - 5, CAP])
def test_attention_pool_under_dynamic_rows(count):
    """Tensors of CAP rows, `count` live ones (graph_ptr ends at the count): the live rows equal the exact-shape call bit for
    bit, and rows at or beyond the count in alpha and gx keep a sentinel written beforehand."""
    from kp_gnn_amd import _lib, ops
    dev = _dev()
    D = 48
    sizes = _dyn_sizes(count)
    G = len(sizes)
    g = torch.Generator().manual_seed(count)
    x_cap = torch.relu(torch.randn(CAP, D, generator=g)).to(dev)
    x_cap[count:] = float("nan")                               # a read of a dead row would show
    lin = nn.Linear(D, 1).to(dev)
    gout = torch.randn(G, D, generator=g).to(dev)
    batch = _batch_of(sizes).to(dev)
    ptr = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=dev)
    # exact shape
    xe = x_cap[:count].clone().requires_grad_(True)
    out_e, alpha_e = ops.attention_pool(xe, batch, G, lin, return_alpha=True)
    ge = torch.autograd.grad(out_e, [xe, lin.weight, lin.bias], gout)
    # capacity shape, through the autograd function under dynamic_rows
    n_dyn = torch.tensor([count], dtype=torch.int32, device=dev)
    xc = x_cap.clone().requires_grad_(True)
    with ops.dynamic_rows(n_dyn, CAP):
        out_c, alpha_c = ops.AttentionPool.apply(xc, lin.weight, lin.bias, ptr, G)
        gc = torch.autograd.grad(out_c, [xc, lin.weight, lin.bias], gout)
    assert torch.equal(out_c, out_e) and torch.equal(alpha_c[:count], alpha_e)
    assert torch.equal(gc[0][:count], ge[0]) and torch.equal(gc[1], ge[1]) and torch.equal(gc[2], ge[2])
    # the same through the descriptors, into buffers that hold a sentinel
    w = lin.weight.detach().reshape(-1).contiguous()
    alpha = torch.full((CAP,), SENTINEL, device=dev)
    out = torch.full((G, D), SENTINEL, device=dev)
    gx = torch.full((CAP, D), SENTINEL, device=dev)
    dw, db = torch.empty(D, device=dev), torch.empty(1, device=dev)
    nb = int(_lib.load().kpgnn_attn_pool_workspace_bytes(G, D))
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    d = _lib.AttnPoolDesc()
    d.N, d.G, d.D, d.n_dyn = CAP, G, D, n_dyn.data_ptr()
    d.graph_ptr, d.x, d.x_stride, d.w, d.bias = ptr.data_ptr(), x_cap.data_ptr(), D, w.data_ptr(), lin.bias.data_ptr()
    d.alpha, d.out, d.gout, d.gx, d.gx_stride = alpha.data_ptr(), out.data_ptr(), gout.data_ptr(), gx.data_ptr(), D
    d.dw, d.db, d.workspace, d.workspace_bytes = dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb
    _lib.launch("kpgnn_attn_pool_fwd", dev, ctypes.byref(d))
    _lib.launch("kpgnn_attn_pool_bwd", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    assert torch.equal(out, out_e) and torch.equal(alpha[:count], alpha_e) and torch.equal(gx[:count], ge[0])
    assert torch.equal(dw, ge[1].reshape(-1)) and torch.equal(db, ge[2])
    assert bool((alpha[count:] == SENTINEL).all()) and bool((gx[count:] == SENTINEL).all())


@pytest.mark.parametrize("count", [1, CAP - 5, CAP])
def test_head_linear_under_dynamic_rows(count):
    """Node rows: y and dx of the live rows, dW and db equal the exact-shape call bit for bit (the row tiles and their order do
    not depend on the live count); rows at or beyond the count in y and dx keep the sentinel."""
    from kp_gnn_amd import _lib, ops, ops_dense
    dev = _dev()
    I, O = 48, 10
    g = torch.Generator().manual_seed(50 + count)
    x_cap = torch.relu(torch.randn(CAP, I, generator=g)).to(dev)
    x_cap[count:] = float("nan")
    dy_cap = torch.randn(CAP, O, generator=g).to(dev)
    dy_cap[count:] = float("nan")
    lin = nn.Linear(I, O).to(dev)
    params = [lin.weight, lin.bias]
    xe = x_cap[:count].clone().requires_grad_(True)
    ye = ops_dense.head_linear(xe, lin)
    ge = torch.autograd.grad(ye, [xe] + params, dy_cap[:count].clone())
    n_dyn = torch.tensor([count], dtype=torch.int32, device=dev)
    xc = x_cap.clone().requires_grad_(True)
    with ops.dynamic_rows(n_dyn, CAP):
        yc = ops_dense.head_linear(xc, lin)
        gc = torch.autograd.grad(yc, [xc] + params, dy_cap)
    assert torch.equal(yc[:count], ye) and torch.equal(gc[0][:count], ge[0])
    # (128-row tiles in both calls, so the same rows meet in the same order; a tile without live rows adds zeros)
    assert torch.equal(gc[1], ge[1]) and torch.equal(gc[2], ge[2])
    # through the descriptor, into buffers that hold a sentinel
    y = torch.full((CAP, O), SENTINEL, device=dev)
    dx = torch.full((CAP, I), SENTINEL, device=dev)
    dw, db = torch.empty(O, I, device=dev), torch.empty(O, device=dev)
    nb = int(_lib.load().kpgnn_head_linear_workspace_bytes(CAP, O, I))
    ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
    w = lin.weight.detach().contiguous()
    d = _lib.HeadLinearDesc()
    d.M, d.O, d.I, d.n_dyn = CAP, O, I, n_dyn.data_ptr()
    d.x, d.x_stride, d.w, d.bias, d.y, d.y_stride = x_cap.data_ptr(), I, w.data_ptr(), lin.bias.data_ptr(), y.data_ptr(), O
    d.dy, d.dy_stride, d.dx, d.dx_stride = dy_cap.data_ptr(), O, dx.data_ptr(), I
    d.dw, d.db, d.workspace, d.workspace_bytes = dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nb
    _lib.launch("kpgnn_head_linear_fwd", dev, ctypes.byref(d))
    _lib.launch("kpgnn_head_linear_bwd", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    assert torch.equal(y[:count], ye) and torch.equal(dx[:count], ge[0])
    assert torch.equal(dw, gc[1]) and torch.equal(db, gc[2])
    assert bool((y[count:] == SENTINEL).all()) and bool((dx[count:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------ launch counts
class StubBody(nn.Module):
    """An embedding model that returns a fixed leaf tensor."""

    def __init__(self, x, JK="last", num_layer=3):
        super().__init__()
        self.hidden_size, self.JK, self.num_layer = x.shape[1], JK, num_layer
        self.x = x

    def reset_parameters(self):
        pass

    def forward(self, data):
        return self.x


def test_heads_on_a_stub_body_launch_only_native_kernels(monkeypatch):
    """Attention readout: 1 launch forward, 1 entry (main + fixed-order reduce, <= 2 kernels) backward; narrow Linear the same;
    the loss 1 launch; and no F.linear, Tensor.index_add_ or F.log_softmax while a head with native shapes runs."""
    from kp_gnn_amd import body as B, ops, ops_dense
    dev = _dev()
    sizes = _sizes("many")
    batch, G = _batch_of(sizes).to(dev), len(sizes)
    torch.manual_seed(5)
    x = torch.relu(torch.randn(int(batch.numel()), 48)).to(dev).requires_grad_(True)
    data = types.SimpleNamespace(batch=batch, num_graphs=G)
    ops.graph_ptr_of(batch, G)                                   # (the one-off order check of a batch vector, as build_csr does)
    y_graph = torch.randint(0, 10, (G,), device=dev)
    y_node = torch.randint(0, 4, (int(batch.numel()),), device=dev)
    t_graph, t_node = torch.randn(G, device=dev), torch.randn(int(batch.numel()), device=dev)

    def run(model, loss_fn):
        model = model.to(dev).train()
        spies = _Spies(monkeypatch)
        loss = loss_fn(model(data))
        n_fwd = len(spies.launches)
        loss.backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        assert spies.no_framework_calls(), (spies.linear, spies.index_add, spies.log_softmax)
        return spies.launches[:n_fwd], spies.launches[n_fwd:]

    fwd, bwd = run(B.GraphClassification(StubBody(x), "attention", 10), lambda o: ops_dense.classification_loss(o, y_graph))
    assert fwd == ["kpgnn_attn_pool_fwd", "kpgnn_head_linear_fwd", "kpgnn_nll_loss"], fwd
    assert bwd == ["kpgnn_head_linear_bwd", "kpgnn_attn_pool_bwd"], bwd
    fwd, bwd = run(B.GraphClassification(StubBody(x), "sum", 2), lambda o: ops_dense.classification_loss(o, y_graph % 2))
    assert fwd == ["kpgnn_segment_pool_fwd", "kpgnn_head_linear_fwd", "kpgnn_nll_loss"], fwd
    assert bwd == ["kpgnn_head_linear_bwd", "kpgnn_segment_pool_bwd"], bwd
    fwd, bwd = run(B.GraphRegression(StubBody(x), "attention"), lambda o: ops_dense.regression_loss(o, t_graph, "mse"))
    assert fwd == ["kpgnn_attn_pool_fwd", "kpgnn_score_head_fwd", "kpgnn_regression_loss"], fwd
    assert bwd == ["kpgnn_score_head_bwd", "kpgnn_attn_pool_bwd"], bwd
    fwd, bwd = run(B.NodeClassification(StubBody(x), 4), lambda o: ops_dense.classification_loss(o, y_node))
    assert fwd == ["kpgnn_head_linear_fwd", "kpgnn_nll_loss"] and bwd == ["kpgnn_head_linear_bwd"], (fwd, bwd)
    fwd, bwd = run(B.NodeRegression(StubBody(x)), lambda o: ops_dense.regression_loss(o, t_node, "mse"))
    assert fwd == ["kpgnn_head_linear_fwd", "kpgnn_regression_loss"] and bwd == ["kpgnn_head_linear_bwd"], (fwd, bwd)


# ------------------------------------------------------------------------------------------------------ whole models
def _body(K, L, H, JK):
    """The seeded KP-GIN+ body of parity_f64.small_body, with the jumping-knowledge mode as a parameter."""
    import argparse
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name="KPGINPlus", hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    return B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK=JK, norm_type="Batch",
                          init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                          num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)


def _head64(p, x, batch, G, head, pooling):
    """The head restated on the oracle body's node rows x: logits or scores."""
    if head in ("GraphClassification", "GraphRegression"):
        if pooling == "attention":
            gate = F.linear(x, p["pool.gate_nn.weight"], p["pool.gate_nn.bias"]).reshape(-1)
            mx = gate.new_full((G,), float("-inf")).scatter_reduce(0, batch, gate.detach(), reduce="amax")
            e = (gate - mx[batch]).exp()
            alpha = e / (x.new_zeros(G).index_add_(0, batch, e)[batch] + 1e-16)
            pooled = x.new_zeros(G, x.shape[1]).index_add_(0, batch, alpha.unsqueeze(-1) * x)
        else:
            pooled = x.new_zeros(G, x.shape[1]).index_add_(0, batch, x)
            if pooling == "mean":
                pooled = pooled / torch.bincount(batch, minlength=G).clamp(min=1).to(x.dtype).unsqueeze(-1)
        if head == "GraphClassification":
            return F.linear(pooled, p["classifier.weight"], p["classifier.bias"])
        return F.linear(pooled, p["regressor.weight"], p["regressor.bias"]).squeeze()
    if head == "NodeClassification":
        return F.linear(x, p["classifier.weight"], p["classifier.bias"])
    return F.linear(x, p["regressor.weight"], p["regressor.bias"]).squeeze()


def _loss64(out, y, head):
    if head.endswith("Classification"):
        return F.nll_loss(F.log_softmax(out, -1), y)
    return ((out - y.to(out.dtype)) ** 2).mean()


def _oracle_model(sd, data, y, G, head, pooling, K, L, JK, dtype):
    from oracle import kp_model_oracle as MO
    p = {k: (v.detach().to(dtype).clone().requires_grad_(True) if PF.trainable(k, v) else PF.to_dtype(v.detach(), dtype).clone())
         for k, v in sd.items()}
    x = MO.body_forward(MO.sub(p, "embedding_model"), data, kind="GNNPlus", layer_kind="KPGINPlus", K=K, num_layer=L,
                        combine_kind="geometric", JK=JK, residual=True, training=True)
    out = _head64(p, x, data["batch"], G, head, pooling)
    loss = _loss64(out, y, head)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items() if v.requires_grad}
    return out.detach(), loss.detach(), grads


def _model_case(head, pooling, C, JK, graphs, K, L, H, seed0):
    from kp_gnn_amd import body as B, ops_dense
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    gnn = _body(K, L, H, JK)
    torch.manual_seed(4)
    model = {"GraphClassification": lambda: B.GraphClassification(gnn, pooling, C),
             "GraphRegression": lambda: B.GraphRegression(gnn, pooling),
             "NodeClassification": lambda: B.NodeClassification(gnn, C),
             "NodeRegression": lambda: B.NodeRegression(gnn)}[head]()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(graphs, seed0=seed0, K=K)
    G, N = host.num_graphs, host.num_nodes
    g = torch.Generator().manual_seed(seed0 + 1)
    rows = G if head.startswith("Graph") else N
    y = torch.randint(0, C, (rows,), generator=g) if head.endswith("Classification") else torch.randn(rows, generator=g)
    ref64, ref32 = _f64_and_f32(lambda dt: _oracle_model(sd, host.as_dict(), y, G, head, pooling, K, L, JK, dt))
    model = model.to(dev).train()
    b = host.to(dev)
    b.build_csr()
    yd = y.to(dev)
    out = model(b)
    loss = ops_dense.classification_loss(out, yd) if head.endswith("Classification") else ops_dense.regression_loss(out, yd, "mse")
    loss.backward()
    torch.cuda.synchronize()
    name = f"{head}/{pooling or '-'} JK={JK} G{G} N{N} K{K} L{L} h{H}"
    got = {n: (torch.zeros_like(q) if q.grad is None else q.grad) for n, q in model.named_parameters() if q.requires_grad}
    PF.print_ratios(name + " out", PF.close_to_f64(out, ref64[0], [r[0] for r in ref32], name + " out", M_F64))
    PF.print_ratios(name + " loss", PF.close_to_f64(loss, ref64[1], [r[1] for r in ref32], name + " loss", M_F64))
    PF.print_ratios(name, PF.close_to_f64(got, ref64[2], [r[2] for r in ref32], name, M_F64))
    return N


@pytest.mark.parametrize("head,pooling,C,JK", [
    ("GraphClassification", "sum", 10, "concat"), ("GraphClassification", "mean", 10, "concat"),
    ("GraphClassification", "attention", 10, "concat"), ("GraphRegression", "attention", None, "concat"),
    ("NodeRegression", None, None, "concat"), ("NodeClassification", None, 4, "last")])
def test_whole_models_vs_float64_oracle_body(head, pooling, C, JK):
    """KP-GIN+, K = 3, L = 3, h = 32 on 24 synthetic molecules with random labels: logits or scores, the loss and every parameter
    gradient against the float64 oracle body plus the head restated above, through close_to_f64 with M = 3."""
    _model_case(head, pooling, C, JK, graphs=24, K=3, L=3, H=32, seed0=31)


def test_graph_classification_at_the_large_batch_shape():
    """220 molecules (N = 5148), K = 8, L = 8, h = 104, attention readout: the heads behind the large-batch kernel paths."""
    N = _model_case("GraphClassification", "attention", 10, "concat", graphs=220, K=8, L=8, H=104, seed0=11)
    assert N == 5148
