"""GPU (-m gpu): the evaluation-mode forward (model.eval() under torch.no_grad()) on the native kernels kpgnn_mlp_eval /
kpgnn_bn_eval / kpgnn_linear_group_fwd, against float64 on the CPU.

Every BatchNorm here carries seeded, non-trivial running statistics and affine parameters (_seed_norms): a fresh module's
0 / 1 statistics would hide a wrong coefficient.  Kernel-level bound: |got - ref| <= ATOL * max|ref| + RTOL * |ref| with the
goldens' RTOL = 1e-4, ATOL = 1e-5 (tests/parity_f64.py); bodies go through parity_f64.close_to_f64 with the project's M = 3."""
import ctypes

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


def _seed_norms(module, seed):
    """running_mean ~ 0.5 N(0,1), running_var ~ U(0.5, 2), gamma ~ U(0.5, 1.5), beta ~ 0.2 N(0,1), a non-zero batch counter."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, nn.BatchNorm1d):
                C = m.num_features
                m.running_mean.copy_(0.5 * torch.randn(C, generator=g))
                m.running_var.copy_(0.5 + 1.5 * torch.rand(C, generator=g))
                m.weight.copy_(0.5 + torch.rand(C, generator=g))
                m.bias.copy_(0.2 * torch.randn(C, generator=g))
                m.num_batches_tracked.fill_(7)
    return module


def _mlp(I, O, bias=True, seed=0):
    torch.manual_seed(seed)
    mlp = nn.Sequential(nn.Linear(I, O, bias=bias), nn.BatchNorm1d(O), nn.ReLU(), nn.Linear(O, O, bias=bias), nn.BatchNorm1d(O), nn.ReLU())
    return _seed_norms(mlp, seed + 1).eval()


def _norm(C, seed):
    return _seed_norms(nn.BatchNorm1d(C), seed).eval()


def _bn64(bn, v):
    return F.batch_norm(v, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.1, bn.eps)


def _lin64(lin, v):
    return F.linear(v, lin.weight.double(), None if lin.bias is None else lin.bias.double())


def _mlp_ref64(mlp, x, bnO=None, res=None):
    """float64 F.linear / F.batch_norm(training=False) / relu on the CPU modules."""
    with torch.no_grad():
        v = torch.relu(_bn64(mlp[1], _lin64(mlp[0], x.double())))
        v = torch.relu(_bn64(mlp[4], _lin64(mlp[3], v)))
        if bnO is not None:
            v = _bn64(bnO, v)
        if res is not None:
            v = v + res.double()
    return v


def _assert_close(got, ref, name):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = PF.ATOL * float(ref.abs().max()) + PF.RTOL * ref.abs()
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"[eval] {name}: max|err| {float(err.max()):.3e}  max|ref| {float(ref.abs().max()):.3e}  err/bound {worst:.3f}")
    assert bool((err <= bound).all()), (name, float(err.max()), worst)


class _Spies:
    """Names of the C-ABI launches, and the framework calls F.linear / F.batch_norm / torch.cat, made while installed."""

    def __init__(self, monkeypatch):
        from kp_gnn_amd import _lib
        self.launches, self.linear, self.batch_norm, self.cat = [], [], [], []
        real_launch, real_lin, real_bn, real_cat = _lib.launch, F.linear, F.batch_norm, torch.cat

        def launch(name, *a, **k):
            self.launches.append(name)
            return real_launch(name, *a, **k)

        def linear(x, *a, **k):
            self.linear.append(tuple(x.shape))
            return real_lin(x, *a, **k)

        def batch_norm(x, *a, **k):
            self.batch_norm.append(tuple(x.shape))
            return real_bn(x, *a, **k)

        def cat(tensors, *a, **k):
            self.cat.append([tuple(t.shape) for t in tensors])
            return real_cat(tensors, *a, **k)

        monkeypatch.setattr(_lib, "launch", launch)
        monkeypatch.setattr(torch.nn.functional, "linear", linear)
        monkeypatch.setattr(torch.nn.functional, "batch_norm", batch_norm)
        monkeypatch.setattr(torch, "cat", cat)

    def count(self, name):
        return sum(1 for n in self.launches if n == name)


def _frozen(*modules):
    return [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in modules]


def _assert_frozen(before, *modules):
    for sd, m in zip(before, modules):
        now = m.state_dict()
        assert sorted(sd) == sorted(now)
        for k, v in sd.items():
            assert torch.equal(v, now[k]), k        # weights, running statistics and num_batches_tracked: bit for bit


def _cu_count():
    from kp_gnn_amd import _lib
    lib = _lib.load()
    cu, lds, wave = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    arch = ctypes.create_string_buffer(64)
    _lib.check(lib.kpgnn_device_info(ctypes.byref(cu), ctypes.byref(lds), ctypes.byref(wave), arch, 64), "kpgnn_device_info")
    return cu.value


def _eval_plan(N, cu):
    """mfma_tile.h tile_plan(N, slots = 2 * cu, {1, 2}, twice_at_1 = true) as mlp_eval.hip calls it: (m, tiles, grid)."""
    slots = 2 * cu
    need = -(-N // (slots * 32))
    m = 1 if need <= 1 else 2
    tiles = -(-N // (32 * m))
    return m, tiles, min(slots * 2 if m == 1 else slots, tiles)


# ------------------------------------------------------------------------------------------------------ kpgnn_mlp_eval
VARIANTS = ["plain", "nobias", "outer", "outer_res"]


def _mlp_case(I, O, N, variant, monkeypatch, seed=0):
    from kp_gnn_amd import ops_dense
    dev = _dev()
    mlp = _mlp(I, O, bias=variant != "nobias", seed=seed)
    bnO = _norm(O, seed + 2) if variant.startswith("outer") else None
    g = torch.Generator().manual_seed(seed + 3)
    x = torch.randn(N, I, generator=g)
    res_wide = torch.randn(N, 2 * O, generator=g) if variant == "outer_res" else None
    ref = _mlp_ref64(mlp, x, bnO, None if res_wide is None else res_wide[:, :O])
    mlp_d = mlp.to(dev)
    bnO_d = None if bnO is None else bnO.to(dev)
    x_d = x.to(dev)
    res_d = None
    if res_wide is not None:
        res_d = res_wide.to(dev)[:, :O]                 # a column slice: rows 2 * O floats apart
        assert res_d.stride(0) == 2 * O
    x_before = x_d.clone()
    frozen = _frozen(mlp_d, *([bnO_d] if bnO_d is not None else []))
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        y = ops_dense.mlp_linear_bn_relu_x2(mlp_d, x_d, post_norm=None if bnO_d is None else (bnO_d, res_d))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert spies.launches == ["kpgnn_mlp_eval"], spies.launches      # the whole of it is that one launch
    assert spies.linear == [] and spies.batch_norm == [], (spies.linear, spies.batch_norm)
    assert not y.requires_grad and y.grad_fn is None
    assert torch.equal(x_d, x_before)
    _assert_frozen(frozen, mlp_d, *([bnO_d] if bnO_d is not None else []))
    _assert_close(y, ref, f"mlp_eval I{I} O{O} N{N} {variant}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N", [1, 33, 97, 200])
@pytest.mark.parametrize("I,O", [(32, 32), (104, 104), (64, 128), (128, 96)])
def test_mlp_eval_vs_float64(I, O, N, variant, monkeypatch):
    """One partial tile (1), one tile plus a tail (33), several tiles (97, 200); below 2 * CUs * 32 rows the plan's tile height
    is 32 rows, the 64-row tiles are test_mlp_eval_more_tiles_than_blocks's."""
    _mlp_case(I, O, N, variant, monkeypatch, seed=I + O + N)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("I,O", [(104, 104), (128, 128)])
def test_mlp_eval_more_tiles_than_blocks(I, O, variant, monkeypatch):
    """More row tiles than the launch has blocks, at 104 x 104 (and at 128 x 128, where the two weight strips leave the fewest
    registers).  The launch plan (mfma_tile.h tile_plan over 2 * CUs block slots,
    tile heights {32, 64}): with 32-row tiles the grid may be 4 * CUs blocks and 32-row tiles are only chosen up to 2 * CUs * 32
    rows, i.e. at most 2 * CUs tiles - never more tiles than blocks.  Beyond that the tiles are 64 rows and the grid is capped at
    2 * CUs, so N = 2 * CUs * 64 + 64 + 5 has 2 * CUs + 2 tiles: blocks 0 and 1 walk a second tile (the register prefetch and
    the re-use of the LDS buffer), the last of them 5 rows high."""
    cu = _cu_count()
    N = 2 * cu * 64 + 64 + 5
    m, tiles, grid = _eval_plan(N, cu)
    assert (m, tiles, grid) == (2, 2 * cu + 2, 2 * cu) and tiles > grid
    _mlp_case(I, O, N, variant, monkeypatch, seed=11)


@pytest.mark.parametrize("I,O,N,native_linears", [(40, 40, 300, 0), (32, 36, 1500, 1)])
def test_mlp_eval_shapes_it_does_not_take_run_on_the_separate_kernels(I, O, N, native_linears, monkeypatch):
    """A width outside the unrolled set: every norm on kpgnn_bn_eval (the outer one with its residual), a Linear on
    kpgnn_linear_fwd where that kernel takes the shape (N >= 1024, I = 32, O % 4 == 0), else on the library."""
    from kp_gnn_amd import ops_dense
    dev = _dev()
    mlp, bnO = _mlp(I, O, seed=5), _norm(O, 6)
    g = torch.Generator().manual_seed(7)
    x, res = torch.randn(N, I, generator=g), torch.randn(N, O, generator=g)
    ref = _mlp_ref64(mlp, x, bnO, res)
    mlp_d, bnO_d = mlp.to(dev), bnO.to(dev)
    frozen = _frozen(mlp_d, bnO_d)
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        y = ops_dense.mlp_linear_bn_relu_x2(mlp_d, x.to(dev), post_norm=(bnO_d, res.to(dev)))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert spies.count("kpgnn_mlp_eval") == 0 and spies.count("kpgnn_bn_eval") == 3, spies.launches
    assert spies.count("kpgnn_linear_fwd") == native_linears and len(spies.linear) == 2 - native_linears, (spies.launches, spies.linear)
    assert spies.batch_norm == []
    _assert_frozen(frozen, mlp_d, bnO_d)
    _assert_close(y, ref, f"mlp fallback I{I} O{O} N{N}")


# ------------------------------------------------------------------------------------------------------- kpgnn_bn_eval
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("N", [1, 77, 5000])
@pytest.mark.parametrize("C", [13, 32, 104, 256])
def test_bn_eval_vs_float64(C, N, relu, res, monkeypatch):
    from kp_gnn_amd import ops_dense
    dev = _dev()
    bn = _norm(C, C + N)
    g = torch.Generator().manual_seed(C * 7 + N)
    x = torch.randn(N, C, generator=g)
    r = torch.randn(N, C, generator=g) if res else None
    with torch.no_grad():
        ref = _bn64(bn, x.double())
        if relu:
            ref = torch.relu(ref)
        if res:
            ref = ref + r.double()
    bn_d, x_d = bn.to(dev), x.to(dev)
    x_before = x_d.clone()
    frozen = _frozen(bn_d)
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        z = ops_dense.batch_norm_act(x_d, bn_d, relu=relu, residual=None if r is None else r.to(dev))
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert spies.launches == ["kpgnn_bn_eval"] and spies.batch_norm == [], (spies.launches, spies.batch_norm)
    assert torch.equal(x_d, x_before)
    _assert_frozen(frozen, bn_d)
    _assert_close(z, ref, f"bn_eval C{C} N{N} relu{int(relu)} res{int(res)}")


# -------------------------------------------------------------------------------------------------------- dynamic rows
@pytest.mark.parametrize("live", ["one", "all_but_5", "all"])
@pytest.mark.parametrize("entry", ["mlp_eval", "bn_eval"])
def test_eval_entries_under_a_dynamic_row_count(entry, live, monkeypatch):
    """ops.dynamic_rows(count, N) with a preallocated, sentinel-filled output: rows below the count are the exact-shape call's
    bit for bit (tile height and grid come from the capacity; a row's sums do not depend on them), rows at or above it keep
    the sentinel."""
    from kp_gnn_amd import ops, ops_dense
    dev = _dev()
    N, C = 200, 104
    count = {"one": 1, "all_but_5": N - 5, "all": N}[live]
    mlp, bnO = _mlp(C, C, seed=21).to(dev), _norm(C, 22).to(dev)
    g = torch.Generator().manual_seed(23)
    x, res = torch.randn(N, C, generator=g).to(dev), torch.randn(N, C, generator=g).to(dev)

    def run(out):
        if entry == "mlp_eval":
            return ops_dense.mlp_eval_raw(mlp, x, post_norm=(bnO, res), out=out)
        return ops_dense.bn_eval_raw(x, bnO, relu=True, residual=res, out=out)

    spies = _Spies(monkeypatch)
    with torch.no_grad():
        exact = run(None)
        out = torch.full((N, C), SENTINEL, dtype=torch.float32, device=dev)
        cnt = torch.tensor([count], dtype=torch.int32, device=dev)
        with ops.dynamic_rows(cnt, N):
            got = run(out)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert spies.launches == ["kpgnn_" + entry] * 2, spies.launches
    assert got is out
    assert torch.equal(out[:count], exact[:count])
    assert bool((out[count:] == SENTINEL).all())
    assert bool((exact != SENTINEL).all())


# -------------------------------------------------------------------------------------------------------------- bodies
_EVAL_REFS = {}


def _eval_oracle(sd, data, dtype, threads=None, **kw):
    from oracle import kp_model_oracle as MO
    kind, layer_kind = PF.BODY_KIND[kw["model_name"]]
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        with torch.no_grad():
            score = MO.graph_regression_forward(PF.to_dtype(sd, dtype), data, kind=kind, layer_kind=layer_kind,
                                                K=kw["K"], num_layer=kw["L"], combine_kind=kw["combine"], JK="concat",
                                                residual=True, training=False)
    finally:
        torch.set_num_threads(before)
    assert score.dtype == dtype
    return score


def _eval_refs(sd, host, **kw):
    """(float64 eval score, [fp32 eval scores at 4, 8 and 16 threads]); computed once per configuration and inputs."""
    key = (tuple(sorted(kw.items())), PF.tensors_sha256(host.as_dict(), sd))
    if key not in _EVAL_REFS:
        data = host.as_dict()
        _EVAL_REFS[key] = (_eval_oracle(sd, data, torch.float64, **kw),
                           [_eval_oracle(sd, data, torch.float32, threads=t, **kw) for t in PF.THREADS])
    return _EVAL_REFS[key]


def _eval_body(model_name, K, L, H, graphs, seed0):
    from kp_gnn_amd.batch import synthetic_zinc_batch
    model = _seed_norms(PF.small_body(model_name, "geometric", K, L, H), 41).eval()
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    host = synthetic_zinc_batch(graphs, seed0=seed0, K=K)
    return model, sd, host


def test_eval_body_runs_under_a_dynamic_row_count(monkeypatch):
    """The eval / no-grad forward of a KP-GIN+ body no longer refuses ops.dynamic_rows (it used to raise: 'BatchNorm on the
    framework path has no dynamic row count').  With the count equal to the capacity it is held to the float64 oracle by the
    bound of the exact-shape forward (close_to_f64, M = 3) and takes the same evaluation kernels.  It is NOT the exact-shape
    score bit for bit: kpgnn_aggregate_fwd, which this path leaves as it is, keeps its small-batch gather for launches without
    a dynamic count (aggregate.hip: agg_small_fwd) and sums a node's neighbours in another order with one."""
    from kp_gnn_amd import ops
    dev = _dev()
    K, L, H = 3, 3, 32
    model, sd, host = _eval_body("KPGINPlus", K, L, H, 24, seed0=11)
    s64, s32 = _eval_refs(sd, host, model_name="KPGINPlus", combine="geometric", K=K, L=L)
    model = model.to(dev)
    b = host.to(dev)
    b.build_csr()
    cnt = torch.tensor([b.num_nodes], dtype=torch.int32, device=dev)
    frozen = _frozen(model)
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        with ops.dynamic_rows(cnt, b.num_nodes):
            got = model(b)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert spies.linear == [] and spies.batch_norm == [], (spies.linear, spies.batch_norm)
    assert spies.count("kpgnn_mlp_eval") == L and spies.count("kpgnn_linear_group_fwd") == 1, spies.launches
    _assert_frozen(frozen, model)
    name = f"eval KPGINPlus K{K} L{L} h{H} dynamic rows"
    PF.print_ratios(name, PF.close_to_f64(got, s64, s32, name, M_F64))


@pytest.mark.parametrize("model_name,K,L,H,graphs", [("KPGINPlus", 3, 3, 32, 24), ("KPGINPlus", 8, 8, 104, 220), ("KPGIN", 8, 4, 104, 220)])
def test_eval_bodies_vs_float64(model_name, K, L, H, graphs, monkeypatch):
    """model.eval() under no_grad against the float64 oracle with training=False, through close_to_f64 (M = 3, the fp32 oracle
    at 4, 8 and 16 threads as the yardstick: it lies 1.6e-7 to 4.6e-7 of max|score| from float64, so the goldens' floor is the
    binding bound).  KP-GIN+: nothing of the forward is a framework Linear, BatchNorm or concatenation of the states - per layer
    one kpgnn_mlp_eval, one grouped-K projection at the end.  KP-GIN (per-hop MLP without norms): the body's per-layer norms
    on kpgnn_bn_eval and the projection on the grouped-K kernel."""
    dev = _dev()
    plus = model_name == "KPGINPlus"
    model, sd, host = _eval_body(model_name, K, L, H, graphs, seed0=11)
    s64, s32 = _eval_refs(sd, host, model_name=model_name, combine="geometric", K=K, L=L)
    assert bool(torch.isfinite(s64).all()) and float(s64.std()) > 0.1
    model = model.to(dev)
    b = host.to(dev)
    b.build_csr()
    N = b.num_nodes
    if graphs == 220:
        assert N == 5148
    frozen = _frozen(model)
    spies = _Spies(monkeypatch)
    with torch.no_grad():
        score = model(b)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert not model.training
    states_cat = [c for c in spies.cat if len(c) >= 2 and all(s == (N, H) for s in c)]
    assert spies.batch_norm == [] and states_cat == [], (spies.batch_norm, states_cat)
    assert spies.count("kpgnn_linear_group_fwd") == 1, spies.launches
    if plus:
        assert spies.linear == [], spies.linear
        assert spies.count("kpgnn_mlp_eval") == L and spies.count("kpgnn_bn_eval") == 0, spies.launches
        assert spies.count("kpgnn_linear_bn") == 0 and spies.count("kpgnn_bn_fwd") == 0
    else:
        assert spies.count("kpgnn_bn_eval") == L, spies.launches
    _assert_frozen(frozen, model)
    name = f"eval {model_name} K{K} L{L} h{H} N{N}"
    PF.print_ratios(name, PF.close_to_f64(score, s64, s32, name, M_F64))


def test_eval_forward_hipgraph_replay_equals_eager():
    """The K = 3, h = 32 eval forward captured once and replayed twice: the replayed score is the eager one bit for bit
    (nothing in it allocates behind the capture's back or synchronises)."""
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    K, L, H = 3, 3, 32
    model = _seed_norms(PF.small_body("KPGINPlus", "geometric", K, L, H), 51).to(dev).eval()
    b = synthetic_zinc_batch(24, seed0=99, K=K).to(dev)
    b.build_csr()
    frozen = _frozen(model)
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(b)                                   # warms the caches that sync (index packing, CSR, range checks)
            eager = model(b).clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = model(b)
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(captured, eager)
    _assert_frozen(frozen, model)
