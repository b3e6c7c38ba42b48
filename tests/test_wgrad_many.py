"""GPU (-m gpu): kpgnn_linear_wgrad_many - the weight gradients of up to 8 MLPs (16 problems) in ONE launch of wgrad3_kernel,
whose blocks walk several slices of a problem with the request pipeline running through the slice boundaries.

Every pair keeps the slicing of a launch of its own, so every dw / db must come back BIT FOR BIT as kpgnn_linear_wgrad_pair
gives it on the same operands.  Shapes: 4129 rows are 129 chunks of 32 and a row (more chunks than the 128 slices: slices of 1
and 2 chunks, the last chunk partial); 2081 rows are 65 chunks and a row (fewer than 128: 65 slices).  With 3 pairs a block walks
3 or 4 slices (1 or 2 at 2081 rows), with 8 pairs 8 (4 or 5).  The first problem of every pair has the BatchNorm + ReLU transform of x
on load, as in FusedMLP.  One case runs under a live row count n_dyn = N - 37 with the dead rows NaN.

One case is also held per element to float64 with the bound tests/test_bf16_split_products.py::_hold_wgrad applies:

    rho(y) = max_ij |y_ij - y64_ij| / (u sum_r |dy_ri| |x_rj|),   u = 2^-24,      rho <= M max(rho32, 1) + D

rho32: torch's fp32 CPU product of the same operands (bf3_cases.fp32_samples, without the sequential sample, as for every weight
gradient); D = 8, the three dropped piece products (7.83 u |a b|); M = bf3_cases.M = 3.  db: plain fp32 column sums, D = 0, against
torch's fp32 column sums.

The body-level test runs KP-GIN+ bodies inside ops.deferred_reductions() and counts the launches."""
import ctypes
import functools

import pytest
import torch

import bf3_cases as C
from test_gpu_parity import _dev, _small_body

pytestmark = pytest.mark.gpu

N_MORE, N_FEWER = 4129, 2081       # chunks > slices / chunks < slices
DEAD = 37


@functools.lru_cache(maxsize=2)
def _operands(count, H, N):
    """Per pair: dy2, y1 (+ the transform's mean, invstd, gamma, beta), dy1, h - seeded normals on the CPU; never modified."""
    g = torch.Generator().manual_seed(1000 * count + H + N)
    out = []
    for _ in range(count):
        dy2, y1, dy1, h = (torch.randn(N, H, generator=g) for _ in range(4))
        coef = (torch.randn(H, generator=g) * 0.1, torch.rand(H, generator=g) + 0.5, torch.rand(H, generator=g) + 0.5,
                torch.randn(H, generator=g) * 0.1)
        out.append((dy2, y1, coef, dy1, h))
    return out


def _descs(pair, outs, ws, n_dyn):
    """(a, b) of one pair as FusedMLP.backward fills them: a = (dy2, relu(bn(y1))), b = (dy1, h)."""
    from kp_gnn_amd import _lib
    dy2, y1, coef, dy1, h = pair
    N, H = dy2.shape
    a, b = _lib.WgradDesc(), _lib.WgradDesc()
    for d, dy, x, k in ((a, dy2, y1, 0), (b, dy1, h, 1)):
        d.N, d.O, d.I = N, H, H
        d.dy, d.dy_stride, d.x, d.x_stride = dy.data_ptr(), H, x.data_ptr(), H
        d.dw, d.db = outs[0][k].data_ptr(), outs[1][k].data_ptr()
        if n_dyn is not None:
            d.n_dyn = n_dyn.data_ptr()
    a.x_mean, a.x_invstd, a.x_gamma, a.x_beta, a.x_relu = (*[c.data_ptr() for c in coef], 1)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    return a, b


def _run(pairs_cpu, live=None):
    """([(dw [2,H,H], db [2,H]) per pair] by pair calls, the same by one many call), both from NaN-filled outputs."""
    from kp_gnn_amd import _lib
    lib, dev = _lib.load(), _dev()
    assert _lib.DENSE_MATH == _lib.MATH_AUTO
    N, H = pairs_cpu[0][0].shape
    n_dyn = None
    pairs = []
    for dy2, y1, coef, dy1, h in pairs_cpu:
        t = [dy2.to(dev), y1.to(dev), tuple(c.to(dev) for c in coef), dy1.to(dev), h.to(dev)]
        if live is not None:
            for x in (t[0], t[1], t[3], t[4]):
                x[live:] = float("nan")
        pairs.append(t)
    if live is not None:
        n_dyn = torch.tensor([live], dtype=torch.int32, device=dev)
    nb = 2 * int(lib.kpgnn_wgrad_workspace_bytes(H, H))

    def fresh():
        return [(torch.full((2, H, H), float("nan"), device=dev), torch.full((2, H), float("nan"), device=dev)) for _ in pairs]

    ws = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in pairs]
    want, got = fresh(), fresh()
    for p, o, w in zip(pairs, want, ws):
        a, b = _descs(p, o, w, n_dyn)
        _lib.launch("kpgnn_linear_wgrad_pair", dev, ctypes.byref(a), ctypes.byref(b))
    torch.cuda.synchronize()
    for w in ws:
        w.fill_(0xFF)
    ds = [_descs(p, o, w, n_dyn) for p, o, w in zip(pairs, got, ws)]
    ptrs = ctypes.POINTER(_lib.WgradDesc) * len(ds)
    _lib.launch("kpgnn_linear_wgrad_many", dev, ptrs(*[ctypes.pointer(a) for a, _ in ds]), ptrs(*[ctypes.pointer(b) for _, b in ds]),
                len(ds))
    torch.cuda.synchronize()
    return want, got


def _same_bits(want, got, what):
    for p, ((dw, db), (dw2, db2)) in enumerate(zip(want, got)):
        assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all()), (what, p, "the pair entry's own result is not finite")
        for k in range(2):
            assert torch.equal(dw[k], dw2[k]), (what, "pair", p, "problem", k, "dw", float((dw[k] - dw2[k]).abs().max()))
            assert torch.equal(db[k], db2[k]), (what, "pair", p, "problem", k, "db", float((db[k] - db2[k]).abs().max()))


@pytest.mark.parametrize("N", [N_MORE, N_FEWER])
@pytest.mark.parametrize("H", [104, 32])
@pytest.mark.parametrize("count", [1, 3, 8])
def test_many_gives_the_pair_entrys_bits(count, H, N):
    want, got = _run(_operands(count, H, N))
    _same_bits(want, got, f"count {count} H {H} N {N}")


def test_many_under_a_live_row_count():
    """n_dyn = N - 37 on a capacity of N = 4129: 128 chunks, the last one partial; the dead rows are NaN in all four operands."""
    want, got = _run(_operands(3, 104, N_MORE), live=N_MORE - DEAD)
    _same_bits(want, got, "n_dyn")


def _transformed(y1, coef):
    """relu(fmaf((y1 - mean) * invstd, gamma, beta)) as the kernel forms it: the fp32 product t * gamma is exact in float64."""
    m, s, g, b = coef
    t = (y1 - m) * s
    return (t.double() * g.double() + b.double()).float().clamp_(min=0)


def test_many_against_float64():
    """count 3, H 104, N 4129: every dw and db of the one launch against float64, with _hold_wgrad's bound (restated above)."""
    pairs = _operands(3, 104, N_MORE)
    _, got = _run(pairs)
    for p, ((dy2, y1, coef, dy1, h), (dw, db)) in enumerate(zip(pairs, got)):
        for k, (dy, x) in enumerate(((dy2, _transformed(y1, coef)), (dy1, h))):
            a, b = dy.t().contiguous(), x.t().contiguous()
            y64, den = C.ref64(a, b), C.denominator(a, b)
            r32 = max(C.rho(y, y64, den) for y in C.fp32_samples(a, b, None, sequential=False))
            r = C.rho(dw[k], y64, den)
            print(f"[wgrad_many] pair {p} problem {k} dW: rho {r:.3f}  rho32 {r32:.3f}  bound {C.bound(r32, C.M, C.D_SPLIT):.3f}")
            assert r <= C.bound(r32, C.M, C.D_SPLIT), (p, k, r, r32)
            db64, dbden = dy.double().sum(0), dy.double().abs().sum(0)
            before = torch.get_num_threads()
            try:
                dbr32 = 0.0
                for t in C.THREADS:
                    torch.set_num_threads(t)
                    dbr32 = max(dbr32, C.rho(dy.sum(0), db64, dbden))
            finally:
                torch.set_num_threads(before)
            rb = C.rho(db[k], db64, dbden)
            print(f"[wgrad_many] pair {p} problem {k} db: rho {rb:.3f}  rho32 {dbr32:.3f}  bound {C.bound(dbr32, C.M, 0):.3f}")
            assert rb <= C.bound(dbr32, C.M, 0), (p, k, rb, dbr32)


@pytest.mark.parametrize("L,want_counts", [(4, [4]), (9, [8, 1])])
def test_a_backward_pass_launches_its_weight_gradients_once(L, want_counts, monkeypatch):
    """KP-GIN+ body, K = 3, H = 32, batch 300 (N >= 4096), inside ops.deferred_reductions(): no MLP launches a pair of its own;
    L = 4 ends in one many-launch of 4 pairs, L = 9 in one of 8 pairs and - a single parked pair goes through the pair entry -
    one pair call for the ninth.  Weights and biases equal the plain run's bit for bit; BatchNorm gamma / beta to fp64-sum
    accuracy, for the reason written in tests/test_gpu_parity.py::test_deferred_reductions_give_the_same_bits (their atomics'
    order follows the timing of the launches around them)."""
    from kp_gnn_amd import _lib, ops
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    K, H = 3, 32
    model = _small_body("KPGINPlus", "geometric", K, L, H).to(dev).train()
    b = synthetic_zinc_batch(300, seed0=7, K=K).to(dev)
    b.build_csr()
    assert b.x.shape[0] >= 4096
    params = [p for p in model.parameters() if p.requires_grad]
    seen = []
    real = _lib.launch

    def spy(name, dev_, *args, **kw):
        if name == "kpgnn_linear_wgrad_many":
            seen.append(("many", int(args[2])))
        elif name == "kpgnn_linear_wgrad_pair":
            seen.append(("pair", len(ops._parked_wgrad)))
        return real(name, dev_, *args, **kw)

    def grads(deferred):
        loss = (model(b).squeeze() - b.y.squeeze()).abs().mean()
        if deferred:
            with ops.deferred_reductions():
                g = torch.autograd.grad(loss, params, allow_unused=True)
            assert not ops._parked_wgrad and ops._pending_reduce is None
        else:
            g = torch.autograd.grad(loss, params, allow_unused=True)
        torch.cuda.synchronize()
        return g

    monkeypatch.setattr(_lib, "launch", spy)
    got = grads(True)
    monkeypatch.setattr(_lib, "launch", real)
    assert [kind for kind, _ in seen] == ["many" if c > 1 else "pair" for c in want_counts], seen
    assert [n for kind, n in seen if kind == "many"] == [c for c in want_counts if c > 1], seen
    want = grads(False)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    norm = {f"{mn}.{pn}" for mn, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm1d) for pn, _ in m.named_parameters()}
    for n, x, y in zip(names, got, want):
        assert (x is None) == (y is None), n
        if x is None:
            continue
        if n in norm:
            assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max()) + 1e-12, (n, float((x - y).abs().max()))
        else:
            assert torch.equal(x, y), (n, float((x - y).abs().max()))
