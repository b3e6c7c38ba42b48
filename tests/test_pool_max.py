"""GPU (-m gpu): the max graph readout - ops.segment_max / body.global_max_pool on csrc/pool_max.hip (kpgnn_segment_max_*).

Everything about the op itself is compared BIT FOR BIT: a max of fp32 values is exact, a gradient is a copied gout element or
+0.0 (compared through .view(torch.int32), so -0.0 fails).  The reference is written here, on the CPU: the winner of a column is
the first row of the graph that attains the column's max, found by an explicit first-occurrence mask - one winner per (graph,
column), the rule of torch_scatter.scatter_max that PyG 2.1.0's global_max_pool has, not amax's even split.  Inputs come from
randint(-3, 4), so every graph has tied maxima in most columns; one case uses randn.  The only tolerance, where a Linear follows
the readout (the heads), is tests/test_heads.py's |got - ref| <= ATOL * max|ref| + RTOL * |ref| against float64."""
import functools
import types

import pytest
import torch
import torch.nn as nn

from test_dynamic_rows_training import NAN, _dead, _dense_live, _dynamic, _poisoned, _two_poisons
from test_heads import _assert_close

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 37, 0, 6, 0)      # both sides of the 4-row unroll, an empty graph mid-batch and one last
MANY = tuple(1 + i % 9 for i in range(70))         # 16 graphs per block at D = 13: the fifth block is partly filled


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _bits(t):
    return t.detach().contiguous().cpu().view(torch.int32)


def _same_bits(got, want, name):
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    assert torch.equal(_bits(got), _bits(want)), name


# ------------------------------------------------------------------------------------------------------------ reference
def _first_winner(seg):
    """[n,D] bool: the first row of `seg` that attains each column's max (the first NaN row where the column holds one)."""
    m = seg.max(0).values
    hit = torch.where(torch.isnan(m), torch.isnan(seg), seg == m)
    return hit & (hit.cumsum(0) == 1)


def _reference(x, sizes, gout=None):
    """CPU: (out [G,D], arg [G,D] int32, gx [N,D] or None) of the rows x[:sum(sizes)]."""
    G, D = len(sizes), x.shape[1]
    out = torch.full((G, D), float("-inf"))
    arg = torch.full((G, D), -1, dtype=torch.int32)
    gx = None if gout is None else torch.zeros(sum(sizes), D)
    b = 0
    for g, n in enumerate(sizes):
        if n:
            seg = x[b:b + n]
            first = _first_winner(seg)
            assert bool((first.sum(0) == 1).all())
            out[g] = seg.max(0).values
            arg[g] = (first * torch.arange(b, b + n).unsqueeze(1)).sum(0).to(torch.int32)
            if gout is not None:
                gx[b:b + n] = torch.where(first, gout[g].expand(n, D), torch.zeros(()))
        b += n
    return out, arg, gx


@functools.lru_cache(maxsize=None)
def _case(D, sizes, kind="tied", extra=0):
    """Inputs on the CPU and their reference, shared and never modified: x [N, D + extra], gout [G,D]; the op sees x[:, 1:1+D] when
    extra > 0."""
    g = torch.Generator().manual_seed(100 * D + len(sizes) + extra)
    N = sum(sizes)
    wide = torch.randn(N, D + extra, generator=g) if kind == "randn" else torch.randint(-3, 4, (N, D + extra), generator=g).float()
    gout = torch.randn(len(sizes), D, generator=g)
    x = wide[:, 1:1 + D] if extra else wide
    return wide, gout, _reference(x.contiguous(), sizes, gout)


def _launch_spy(monkeypatch):
    """[(name, descriptor)] of the C-ABI launches made while installed."""
    from kp_gnn_amd import _lib
    seen, real = [], _lib.launch

    def launch(name, dev, *a, **k):
        seen.append((name, a[0]._obj if a and hasattr(a[0], "_obj") else None))
        return real(name, dev, *a, **k)

    monkeypatch.setattr(_lib, "launch", launch)
    return seen


# --------------------------------------------------------------------------------- 1. forward, winners, backward vs the reference
CASES = [(1, SIZES, "tied", 0), (2, SIZES, "tied", 0), (13, SIZES, "tied", 0), (104, SIZES, "tied", 0), (256, SIZES, "tied", 0),
         (104, SIZES, "tied", 3),                  # wide[:, 1:105] of [N,107]: odd offset and stride, vec = 1, 128 lanes, no copy
         (13, MANY, "tied", 0), (104, SIZES, "randn", 0)]


@pytest.mark.parametrize("D,sizes,kind,extra", CASES, ids=lambda v: str(len(v)) + "graphs" if isinstance(v, tuple) else str(v))
def test_forward_winners_and_backward(D, sizes, kind, extra, monkeypatch):
    from kp_gnn_amd import ops
    dev, G = _dev(), len(sizes)
    wide, gout, (out_r, arg_r, gx_r) = _case(D, sizes, kind, extra)
    batch = _batch_of(sizes).to(dev)
    seen = _launch_spy(monkeypatch)

    def run():
        x = (wide.to(dev)[:, 1:1 + D] if extra else wide.to(dev)).detach().requires_grad_(True)
        out = ops.segment_max(x, batch, G)
        arg = out.grad_fn.saved_tensors[1]
        assert len(out.grad_fn.saved_tensors) == 2 and arg.dtype == torch.int32          # batch and the winners, nothing else
        out.backward(gout.to(dev))
        return x, out, arg

    x, out, arg = run()
    assert [n for n, _ in seen] == ["kpgnn_segment_max_fwd", "kpgnn_segment_max_bwd"]
    if extra:
        d = seen[0][1]
        assert (d.x, d.x_stride) == (x.data_ptr(), D + extra) and not x.is_contiguous()     # read in place
    _same_bits(out, out_r, "out")
    empty = [g for g, n in enumerate(sizes) if n == 0]
    assert bool(torch.isinf(out[empty]).all()) and bool((out[empty] < 0).all())
    assert torch.equal(arg.cpu(), arg_r), "winners"
    assert bool((arg.cpu()[empty] == -1).all())
    _same_bits(x.grad, gx_r, "x.grad")
    x2, out2, arg2 = run()
    _same_bits(out2, out, "out, second call")
    assert torch.equal(arg2, arg)
    _same_bits(x2.grad, x.grad, "x.grad, second call")


# ------------------------------------------------------------------------------------------------------------------ 2. NaN
def test_nan_wins_and_stays():
    from kp_gnn_amd import ops
    dev, sizes = _dev(), (5, 6)
    g = torch.Generator().manual_seed(2)
    x = torch.randint(-3, 4, (11, 4), generator=g).float()
    x[1, 0], x[2, 0], x[4, 0] = 5.0, NAN, 7.0          # graph 0, column 0: a NaN after a larger finite value, a larger one after it
    x[5, 2], x[6, 2], x[9, 2] = NAN, 9.0, NAN          # graph 1, column 2: a NaN first, a finite value and a second NaN after it
    gout = torch.randn(2, 4, generator=g)
    out_r, arg_r, gx_r = _reference(x, sizes, gout)
    assert int(arg_r[0, 0]) == 2 and int(arg_r[1, 2]) == 5
    xd = x.to(dev).requires_grad_(True)
    out = ops.segment_max(xd, _batch_of(sizes).to(dev), 2)
    arg = out.grad_fn.saved_tensors[1].cpu()
    out.backward(gout.to(dev))
    o = out.detach().cpu()
    assert bool(torch.isnan(o[0, 0])) and bool(torch.isnan(o[1, 2])) and int(torch.isnan(o).sum()) == 2
    assert torch.equal(arg, arg_r)
    keep = ~torch.isnan(out_r)
    assert torch.equal(_bits(o)[keep], _bits(out_r)[keep])          # the other columns are unaffected
    _same_bits(xd.grad, gx_r, "x.grad")


# --------------------------------------------------------------------------------------------------------- 3. dynamic rows
@pytest.mark.parametrize("live", _dense_live(1100))
@pytest.mark.parametrize("D", [104, 13])
def test_dynamic_rows(D, live):
    """tests/test_dynamic_rows_training.py::test_segment_pool for the max readout: the batch vector has capacity length, its dead
    rows repeat graph id G - 1, the graph pointer ends at the live count; dead rows of x hold NaN in one run, 1e30 in the other."""
    from kp_gnn_amd import ops
    dev, CAP, G = _dev(), 1100, 40
    g = torch.Generator().manual_seed(D + live)
    cut = torch.sort(torch.randint(0, live + 1, (G - 1,), generator=g)).values          # (empty graphs where cuts coincide)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), cut, torch.tensor([live])])
    sizes = (ptr[1:] - ptr[:-1]).tolist()
    batch = torch.cat([_batch_of(sizes), torch.full((CAP - live,), G - 1, dtype=torch.long)])
    x = torch.randint(-3, 4, (CAP, D), generator=g).float()
    w = torch.randn(G, D, generator=g)
    out_r, _, gx_r = _reference(x[:live], sizes, w)

    def run(poison):
        xs = x.clone()
        xs[live:] = poison
        xd, bd = xs.to(dev).requires_grad_(True), batch.to(dev)
        setattr(bd, ops._GPTR, ((bd._version, G), ptr.to(torch.int32).to(dev)))
        with _dynamic(live, CAP):
            out = ops.segment_max(xd, bd, G)
            (out * w.to(dev)).sum().backward()
        _dead(xd.grad, live, NAN, "max readout grad")
        got = {"out": out.detach(), "grad": xd.grad[:live]}
        _same_bits(got["out"], out_r, "out")
        _same_bits(got["grad"], gx_r, "x.grad[:live]")
        return got

    _two_poisons("segment_max", run, bitwise=True)


# -------------------------------------------------------------------------------------------------------------- 4. refusals
def test_routes_without_a_row_count_refuse_the_capacity():
    from kp_gnn_amd import body, ops
    from kp_gnn_amd._lib import KpgnnError
    dev, sizes = _dev(), (3, 0, 5, 4)
    N, G = sum(sizes), len(sizes)
    g = torch.Generator().manual_seed(4)
    wide = torch.randint(-3, 4, (N, 300), generator=g).float().to(dev)
    x64 = torch.randint(-3, 4, (N, 8), generator=g).double().to(dev)
    batch = _batch_of(sizes).to(dev)
    cnt = torch.tensor([N], dtype=torch.int32, device=dev)

    def amax(x):
        return x.new_full((G, x.shape[1]), float("-inf")).scatter_reduce(0, batch.view(-1, 1).expand_as(x), x, reduce="amax")

    with ops.dynamic_rows(cnt, N):
        with pytest.raises(KpgnnError, match="max readout of rows wider than 256"):
            ops.segment_max(wide, batch, G)
        with pytest.raises(KpgnnError, match="max readout on the framework path"):
            body.global_max_pool(x64, batch, G)
    with ops.dynamic_rows(cnt, N + 1):                     # the capacity is another number: the same calls run
        assert torch.equal(ops.segment_max(wide, batch, G), amax(wide))
        assert torch.equal(body.global_max_pool(x64, batch, G), amax(x64))


# ----------------------------------------------------------------------------------------------------------------- 5. heads
class StubBody(nn.Module):
    """An embedding model that returns a fixed leaf tensor: hidden_size, JK and num_layer are all the heads read."""

    def __init__(self, x, JK="last", num_layer=3):
        super().__init__()
        self.hidden_size, self.JK, self.num_layer = x.shape[1], JK, num_layer
        self.x = x

    def reset_parameters(self):
        pass

    def forward(self, data):
        return self.x


def _head_inputs():
    g = torch.Generator().manual_seed(11)
    sizes = torch.randint(10, 40, (12,), generator=g)
    sizes[-1] += 300 - int(sizes.sum())
    assert int(sizes.min()) > 0 and int(sizes.sum()) == 300
    return sizes.tolist(), torch.randint(-3, 4, (300, 32), generator=g).float(), g


def _head(kind, x):
    from kp_gnn_amd import body
    torch.manual_seed(7)
    return body.GraphClassification(StubBody(x), "max", 7) if kind == "classification" else body.GraphRegression(StubBody(x), "max")


def _head_f64(lin, x, sizes, w):
    """float64 torch evaluation with the single-winner rule: (result, dx, {parameter: gradient})."""
    x = x.double().requires_grad_(True)
    W, b = lin.weight.detach().cpu().double().requires_grad_(True), lin.bias.detach().cpu().double().requires_grad_(True)
    rows, s = [], 0
    for n in sizes:
        seg = x[s:s + n]
        rows.append(torch.where(_first_winner(seg.detach()), seg, torch.zeros((), dtype=torch.float64)).sum(0))
        s += n
    res = (torch.stack(rows) @ W.t() + b).squeeze()
    (res * w.double()).sum().backward()
    return res.detach(), x.grad, {"weight": W.grad, "bias": b.grad}


@pytest.mark.parametrize("kind", ["classification", "regression"])
def test_heads_run_the_native_readout(kind, monkeypatch):
    dev = _dev()
    sizes, x0, g = _head_inputs()
    x = x0.to(dev).requires_grad_(True)
    model = _head(kind, x).to(dev).train()
    lin = model.classifier if kind == "classification" else model.regressor
    w = torch.randn((12, 7) if kind == "classification" else (12,), generator=g)
    data = types.SimpleNamespace(batch=_batch_of(sizes).to(dev), num_graphs=12)
    seen, scatters, real = _launch_spy(monkeypatch), [], torch.Tensor.scatter_reduce
    monkeypatch.setattr(torch.Tensor, "scatter_reduce", lambda t, *a, **k: (scatters.append(tuple(t.shape)), real(t, *a, **k))[1])
    res = model(data)
    fwd = [n for n, _ in seen]
    (res * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    names = [n for n, _ in seen]
    assert fwd.count("kpgnn_segment_max_fwd") == 1 and "kpgnn_segment_max_bwd" not in fwd
    assert names.count("kpgnn_segment_max_fwd") == 1 and names[len(fwd):].count("kpgnn_segment_max_bwd") == 1
    assert scatters == []
    res_r, dx_r, gp_r = _head_f64(lin, x0, sizes, w)
    _assert_close(res, res_r, f"{kind} result")
    _assert_close(x.grad, dx_r, f"{kind} x.grad")
    _assert_close(lin.weight.grad, gp_r["weight"], f"{kind} weight.grad")
    _assert_close(lin.bias.grad, gp_r["bias"], f"{kind} bias.grad")


# --------------------------------------------------------------------------------------------------------------- 6. no grad
def test_no_grad_keeps_no_winners(monkeypatch):
    from kp_gnn_amd import ops
    dev = _dev()
    wide, _, (out_r, _, _) = _case(104, SIZES)
    batch = _batch_of(SIZES).to(dev)
    seen = _launch_spy(monkeypatch)
    x = wide.to(dev).requires_grad_(True)
    with torch.no_grad():
        a = ops.segment_max(x, batch, len(SIZES))
    b = ops.segment_max(x.detach(), batch, len(SIZES))          # grad enabled, x does not require it
    c = ops.segment_max(x, batch, len(SIZES))
    assert a.grad_fn is None and not a.requires_grad and b.grad_fn is None and c.grad_fn is not None
    assert [n for n, _ in seen] == ["kpgnn_segment_max_fwd"] * 3
    assert seen[0][1].arg is None and seen[1][1].arg is None and seen[2][1].arg is not None
    _same_bits(a, c, "no_grad vs grad")
    _same_bits(b, c, "detached vs grad")
    _same_bits(c, out_r, "out")


# ---------------------------------------------------------------------------------------------------------------- 7. capture
def test_head_step_is_captured_and_replays_on_new_values():
    dev = _dev()
    sizes, x0, g = _head_inputs()
    x = x0.to(dev).requires_grad_(True)
    model = _head("classification", x).to(dev).train()
    w = torch.randn(12, 7, generator=g).to(dev)
    data = types.SimpleNamespace(batch=_batch_of(sizes).to(dev), num_graphs=12)

    def step():
        logits = model(data)
        return logits, torch.autograd.grad(logits, [x], grad_outputs=w)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                        # caches the graph pointer of the batch (its order check syncs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        logits_g, dx_g = step()
    new = torch.randint(-3, 4, (300, 32), generator=g).float().to(dev)
    with torch.no_grad():
        x.copy_(new)
    graph.replay()
    torch.cuda.synchronize()
    logits_g, dx_g = logits_g.detach().clone(), dx_g.clone()
    logits_e, dx_e = step()
    _same_bits(logits_g, logits_e, "replayed logits")
    _same_bits(dx_g, dx_e, "replayed x.grad")
    assert not torch.equal(new, x0.to(dev)) and int((dx_e != 0).sum()) > 0


# ---------------------------------------------------------------------------------------------------- 8. a real StaticBatch
def test_static_batch():
    """A KHopDataset's static batch of 16 graphs, two id lists staged in turn: the readout of the capacity-shaped batch (dead
    rows of x NaN, dead rows of the batch vector whatever the collate left) is the reference on the live rows."""
    from test_virtual_node import _dataset
    from kp_gnn_amd import body
    dev = _dev()
    raw, args, ds = _dataset(64, 4, seed0=5)
    sb = ds.static_batch(16)
    g = torch.Generator().manual_seed(8)
    real_empty = torch.empty
    with sb.dynamic():
        for ids in ([9, 3, 60, 21, 22, 23, 0, 63, 11, 40, 41, 5, 7, 30, 31, 50], list(range(48, 64))):
            sb.stage(ids)
            sb.launch_collate()
            torch.cuda.synchronize()
            live = sb.live[0]
            assert live < sb.N_cap and tuple(sb.batch.batch.shape) == (sb.N_cap,)
            bl = sb.batch.batch[:live].cpu()
            sizes = torch.bincount(bl, minlength=16).tolist()
            assert torch.equal(bl, _batch_of(sizes))
            xs = torch.full((sb.N_cap, 32), NAN)
            xs[:live] = torch.randint(-3, 4, (live, 32), generator=g).float()
            w = torch.randn(16, 32, generator=g)
            out_r, _, gx_r = _reference(xs[:live], sizes, w)
            x = xs.to(dev).requires_grad_(True)
            mp = pytest.MonkeyPatch()
            mp.setattr(torch, "empty", lambda *a, **kw: _poisoned(real_empty(*a, **kw)))
            try:
                out = body.global_max_pool(x, sb.batch.batch, 16)
                (out * w.to(dev)).sum().backward()
                torch.cuda.synchronize()
            finally:
                mp.undo()
            _same_bits(out, out_r, "out")
            _same_bits(x.grad[:live], gx_r, "x.grad[:live]")
            _dead(x.grad, live, NAN, "max readout grad")
