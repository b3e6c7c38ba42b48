"""kpgnn_body_norm_fwd / _bwd (csrc/body_norm.hip) through the C ABI, and the four norm modules of kp_gnn_amd.body on the CPU.

CPU: both entries reject malformed descriptors before any device call, N == 0 launches nothing, the binding matches the header,
CPU tensors through the modules are tests/norm_ref.py bit for bit (fp32 and float64, forward and gradients), the state_dict keys
are PyG's, and the three bodies construct with every norm_type.  GPU: every kind and shape against the float64 reference with
the fp32 CPU evaluation as the yardstick (close_to_f64, M = 3), rows beyond *n_dyn left alone in every output of both directions
on a workspace full of NaN, and run-to-run identical bits."""
import argparse
import ctypes
import os
import re

import pytest
import torch

import norm_ref as NR
import parity_f64 as PF

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
OK, EINVAL, ELIMIT = 0, -1, -3
LAYER, INSTANCE, GRAPHSIZE, PAIR = 0, 1, 2, 3
KIND_ID = {"Layer": LAYER, "Instance": INSTANCE, "GraphSize": GRAPHSIZE, "Pair": PAIR}
FWD, BWD = "kpgnn_body_norm_fwd", "kpgnn_body_norm_bwd"
RTOL, ATOL = PF.RTOL, PF.ATOL
M_F64 = 3
# one row; one column; a width that is no multiple of 4 (8-byte accesses); two scalar shapes (33: 64 lanes, 65: 128 lanes); the
# widest row; several partial blocks
SHAPES = [(1, 104), (2, 1), (257, 6), (257, 33), (300, 256), (5000, 104), (70, 65)]
# badly conditioned columns: a mean far from 0 against a spread of 1, and of 1e-3
CONDITIONED = [(N, 104, name) for N in (500, 3000) for name in ("100+randn", "5+1e-3*randn", "1000+randn")]
CASES = [(N, C, "randn") for N, C in SHAPES] + CONDITIONED


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _desc(lib, N=100, C=32, kind=LAYER, **kw):
    """A descriptor that passes every check of both entries (all pointers dummies); kw overrides."""
    from kp_gnn_amd import _lib
    d = _lib.NormDesc()
    d.N, d.C, d.kind, d.eps = N, C, kind, 1e-5
    d.x, d.x_stride, d.weight, d.bias, d.residual, d.res_stride = A, C, A, A, A, C
    d.out, d.out_stride, d.saved = A, C, A
    d.gout, d.gout_stride, d.gx, d.gx_stride, d.gweight, d.gbias = A, C, A, C, A, A
    d.workspace = A
    d.workspace_bytes = lib.kpgnn_body_norm_workspace_bytes(max(N, 0), C) if 1 <= C <= 256 else 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------ CPU
COMMON_BAD = [dict(C=0), dict(C=-4), dict(C=257), dict(kind=-1), dict(kind=4), dict(N=-1), dict(x=None), dict(saved=None),
              dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes=15), dict(kind=LAYER, weight=None),
              dict(x_stride=31), dict(x_stride=-32), dict(eps=-1.0)]
FWD_BAD = COMMON_BAD + [dict(out=None), dict(out_stride=31), dict(res_stride=31)]
BWD_BAD = COMMON_BAD + [dict(gout=None), dict(gx=None), dict(gout_stride=31), dict(gx_stride=31)]


def test_null_descriptors_are_rejected(lib):
    for name in (FWD, BWD):
        assert getattr(lib, name)(None, None) == EINVAL, name
        assert name.encode() + b": NULL descriptor" in lib.kpgnn_last_error()


def _rejected(lib, name, kw):
    rc = getattr(lib, name)(ctypes.byref(_desc(lib, **kw)), None)
    assert rc == (ELIMIT if kw.get("C", 0) > 256 else EINVAL), (kw, rc)
    assert name.encode() in lib.kpgnn_last_error(), lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", FWD_BAD, ids=repr)
def test_malformed_forward_descriptors_are_rejected(lib, kw):
    """A message naming the entry, before any device call (the stream is NULL and every pointer a dummy); C > 256 is a limit."""
    _rejected(lib, FWD, kw)


@pytest.mark.parametrize("kw", BWD_BAD, ids=repr)
def test_malformed_backward_descriptors_are_rejected(lib, kw):
    _rejected(lib, BWD, kw)


def test_a_workspace_one_byte_short_is_rejected(lib):
    need = lib.kpgnn_body_norm_workspace_bytes(5000, 104)
    assert need >= 2 * 104 * 8 * 2 and need % 16 == 0
    for name in (FWD, BWD):
        assert getattr(lib, name)(ctypes.byref(_desc(lib, N=5000, C=104, workspace_bytes=need - 1)), None) == EINVAL
        assert b"workspace" in lib.kpgnn_last_error()
    assert lib.kpgnn_body_norm_workspace_bytes(10, 0) == 0 and lib.kpgnn_body_norm_workspace_bytes(10, 257) == 0
    assert lib.kpgnn_body_norm_workspace_bytes(-1, 8) == 0 and lib.kpgnn_body_norm_workspace_bytes(0, 256) > 0


def test_no_rows_launch_nothing_and_unused_operands_may_be_null(lib):
    """N == 0 returns 0 for a descriptor that passes validation: the forward needs no gout / gx, the backward no out, and only
    Layer needs a weight."""
    for kind in (LAYER, INSTANCE, GRAPHSIZE, PAIR):
        w = A if kind == LAYER else None
        d = _desc(lib, N=0, kind=kind, weight=w, bias=None, residual=None, gout=None, gx=None, gweight=None, gbias=None)
        assert lib.kpgnn_body_norm_fwd(ctypes.byref(d), None) == OK, kind
        d = _desc(lib, N=0, kind=kind, weight=w, bias=None, residual=None, out=None, gweight=None, gbias=None)
        assert lib.kpgnn_body_norm_bwd(ctypes.byref(d), None) == OK, kind
    assert lib.kpgnn_body_norm_fwd(ctypes.byref(_desc(lib, N=0, C=256)), None) == OK       # the maximal C is accepted


def test_the_binding_matches_the_header(lib):
    from kp_gnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "kpgnn.h")).read()
    body = re.search(r"typedef struct kpgnn_norm_desc \{(.*?)\} kpgnn_norm_desc;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*$", part).group(1) for stmt in body.split(";") if stmt.strip() for part in stmt.split(",")]
    assert names == [f[0] for f in _lib.NormDesc._fields_], names
    assert names == ["N", "C", "kind", "eps", "x", "x_stride", "weight", "bias", "residual", "res_stride", "out", "out_stride",
                     "saved", "gout", "gout_stride", "gx", "gx_stride", "gweight", "gbias", "workspace", "workspace_bytes", "n_dyn"]
    assert (_lib.NORM_LAYER, _lib.NORM_INSTANCE, _lib.NORM_GRAPHSIZE, _lib.NORM_PAIR) == (LAYER, INSTANCE, GRAPHSIZE, PAIR)
    assert dict(_lib.NormDesc._fields_)["eps"] is ctypes.c_float and dict(_lib.NormDesc._fields_)["N"] is ctypes.c_int64
    for name in (FWD, BWD):
        assert getattr(lib, name).argtypes[0] == ctypes.POINTER(_lib.NormDesc)
    assert lib.kpgnn_body_norm_workspace_bytes.restype is ctypes.c_size_t


def _module(kind, C):
    from kp_gnn_amd import body as B
    return {"Layer": lambda: B.LayerNorm(C), "Instance": lambda: B.InstanceNorm(C), "GraphSize": B.GraphSizeNorm,
            "Pair": B.PairNorm}[kind]()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_cpu_tensors_through_the_modules_are_the_reference_bit_for_bit(kind, dtype):
    from kp_gnn_amd import ops
    assert ops.native_norms() is True
    g = torch.Generator().manual_seed(7)
    for N, C in [(1, 8), (37, 12), (200, 104)]:
        x = (0.5 + torch.randn(N, C, generator=g)).to(dtype).requires_grad_(True)
        res = torch.randn(N, C, generator=g).to(dtype).requires_grad_(True)
        go = torch.randn(N, C, generator=g).to(dtype)
        mod = _module(kind, C).to(dtype)
        assert not ops.body_norm_applies(x)
        params = list(mod.parameters())
        if kind == "Layer":
            with torch.no_grad():
                mod.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
                mod.bias.copy_(0.2 * torch.randn(C, generator=g))
        for train in (True, False):          # (no running statistics: eval() computes the same)
            mod.train(train)
            for r in (None, res):
                got = mod(x) if r is None else mod(x, residual=r)
                want = NR.norm(kind, x, *params, residual=r)
                assert got.dtype == dtype and torch.equal(got, want), (kind, N, C, train)
                ins = [x] + params + ([] if r is None else [r])
                ga = torch.autograd.grad(got, ins, go)
                gw = torch.autograd.grad(want, ins, go)
                assert all(torch.equal(a, b) for a, b in zip(ga, gw)), (kind, N, C, train)
    with pytest.raises(ValueError):
        ops.body_norm(torch.zeros(3, 4), "Batch")
    with pytest.raises(ValueError):
        ops.body_norm(torch.zeros(3, 4), "Layer")
    with pytest.raises(ValueError):
        ops.body_norm(torch.zeros(3, 4), "Pair", torch.ones(4), torch.zeros(4))
    prev = ops.set_native_norms(False)
    try:
        assert prev is True and ops.native_norms() is False and ops.native_norm_exact("Layer") is False
    finally:
        ops.set_native_norms(True)
    assert ops.native_norms() is True
    # per kind, on exact-shape batches: GraphSize is opt-in (an eager step measured slower with it), the others are on
    assert [ops.native_norm_exact(k) for k in NR.KINDS] == [True, True, False, True]
    prev = ops.set_native_norm_exact("GraphSize", True)
    try:
        assert prev is False and ops.native_norm_exact("GraphSize") is True
    finally:
        ops.set_native_norm_exact("GraphSize", False)
    with pytest.raises(ValueError):
        ops.set_native_norm_exact("Batch", True)


def test_state_dict_keys_are_pygs():
    from kp_gnn_amd import body as B
    assert sorted(B.LayerNorm(6).state_dict()) == ["bias", "weight"]
    for m in (B.InstanceNorm(6), B.GraphSizeNorm(), B.PairNorm()):
        assert list(m.state_dict()) == [] and list(m.buffers()) == []
    ln = B.LayerNorm(6)
    with torch.no_grad():
        ln.weight.fill_(3.0)
        ln.bias.fill_(-2.0)
    ln.reset_parameters()
    assert torch.equal(ln.weight, torch.ones(6)) and torch.equal(ln.bias, torch.zeros(6))


def _body(model_name, norm_type, K=3, L=3, H=24):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    return B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type=norm_type,
                          init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                          num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)


@pytest.mark.parametrize("model_name", ["KPGIN", "KPGINPlus", "KPGINPrime"])
def test_the_bodies_construct_with_every_norm_type(model_name):
    from kp_gnn_amd import body as B
    cls = {"Batch": B.BatchNorm, "Layer": B.LayerNorm, "Instance": B.InstanceNorm, "GraphSize": B.GraphSizeNorm, "Pair": B.PairNorm}
    for norm_type, c in cls.items():
        gnn = _body(model_name, norm_type)
        assert len(gnn.norms) == 3 and all(type(m) is c for m in gnn.norms), norm_type
        keys = sorted(k for k in gnn.state_dict() if k.startswith("norms.0."))
        want = {"Batch": ["norms.0.module." + s for s in ("bias", "num_batches_tracked", "running_mean", "running_var", "weight")],
                "Layer": ["norms.0.bias", "norms.0.weight"]}.get(norm_type, [])
        assert keys == want, (norm_type, keys)
        gnn.reset_parameters()
    for bad in ("batch", "layer", "Group", None):
        with pytest.raises(ValueError, match="Not supported norm method"):
            _body(model_name, bad)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda:0")


def _inputs(N, C, name, seed=0):
    """(x, gout, residual, weight, bias) on the CPU in fp32, seeded by the case."""
    g = torch.Generator().manual_seed(100003 * seed + 1000 * N + C)
    z = torch.randn(N, C, generator=g)
    x = {"randn": z, "100+randn": 100 + z, "5+1e-3*randn": 5 + 1e-3 * z, "1000+randn": 1000 + z}[name]
    gout, res = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    return x, gout, res, 1 + 0.3 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


def _reference(kind, x, gout, res, w, b, dtype):
    """{y, dx[, dweight, dbias]} of norm_ref in `dtype` on the CPU through autograd."""
    x = x.to(dtype).clone().requires_grad_(True)
    params = [t.to(dtype).clone().requires_grad_(True) for t in (w, b)] if kind == "Layer" else []
    y = NR.norm(kind, x, *params, residual=None if res is None else res.to(dtype))
    grads = torch.autograd.grad(y, [x] + params, gout.to(dtype))
    out = {"y": y.detach(), "dx": grads[0]}
    if kind == "Layer":
        out["dweight"], out["dbias"] = grads[1], grads[2]
    return out


def _roundtrip(kind, x, gout, res, w, b, live=None, ws_fill=None, runs=1):
    """{y, dx[, dweight, dbias], saved} of one forward + backward through the C ABI on the device.  x / gout / res: device
    tensors of the CAPACITY; live: the device-side row count (n_dyn); out and gx start as -7 everywhere, the workspace as
    `ws_fill` bytes, and the whole round trip runs `runs` times on the same buffers."""
    from kp_gnn_amd import _lib
    dev = _dev()
    N, C = x.shape
    out, gx = torch.full((N, C), -7.0, device=dev), torch.full((N, C), -7.0, device=dev)
    saved = torch.full((2 * C + 4,), -7.0, device=dev)
    gw, gb = torch.full((C,), -7.0, device=dev), torch.full((C,), -7.0, device=dev)
    nbytes = _lib.load().kpgnn_body_norm_workspace_bytes(N, C)
    ws = torch.full((nbytes,), 0 if ws_fill is None else ws_fill, dtype=torch.uint8, device=dev)
    n_dyn = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
    d = _lib.NormDesc()
    d.N, d.C, d.kind, d.eps = N, C, KIND_ID[kind], 1e-5
    d.x, d.x_stride, d.out, d.out_stride, d.saved = x.data_ptr(), x.stride(0), out.data_ptr(), C, saved.data_ptr()
    d.gout, d.gout_stride, d.gx, d.gx_stride = gout.data_ptr(), gout.stride(0), gx.data_ptr(), C
    if kind == "Layer":
        d.weight, d.bias, d.gweight, d.gbias = w.data_ptr(), b.data_ptr(), gw.data_ptr(), gb.data_ptr()
    if res is not None:
        d.residual, d.res_stride = res.data_ptr(), res.stride(0)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    if n_dyn is not None:
        d.n_dyn = n_dyn.data_ptr()
    for _ in range(runs):
        _lib.launch(FWD, dev, ctypes.byref(d))
        _lib.launch(BWD, dev, ctypes.byref(d))
    torch.cuda.synchronize()
    got = {"y": out.cpu(), "dx": gx.cpu(), "saved": saved.cpu()}
    if kind == "Layer":
        got["dweight"], got["dbias"] = gw.cpu(), gb.cpu()
    return got


_REFS = {}


def _refs(kind, N, C, name, with_res):
    key = (kind, N, C, name, with_res)
    if key not in _REFS:
        x, gout, res, w, b = _inputs(N, C, name)
        r = res if with_res else None
        _REFS[key] = (_reference(kind, x, gout, r, w, b, torch.float64), _reference(kind, x, gout, r, w, b, torch.float32))
    return _REFS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("N,C,name", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("kind", NR.KINDS)
def test_every_kind_and_shape_against_float64(kind, N, C, name):
    """y, dx and Layer's dweight / dbias, each on its own through close_to_f64 with M = 3: the float64 reference is norm_ref
    with autograd, the yardstick norm_ref in fp32 on the CPU; with and without a residual.  One row (N = 1) has the exact answer
    0 for Instance and Pair in y and dx, the yardstick's error is then 0 too, and so the bound is: exact zeros."""
    dev = _dev()
    x, gout, res, w, b = _inputs(N, C, name)
    for with_res in (False, True):
        ref64, ref32 = _refs(kind, N, C, name, with_res)
        got = _roundtrip(kind, x.to(dev), gout.to(dev), res.to(dev) if with_res else None, w.to(dev), b.to(dev))
        for k in ref64:
            tag = f"body_norm {kind} ({N},{C}) {name}{' +res' if with_res else ''} {k}"
            PF.print_ratios(tag, PF.close_to_f64(got[k], ref64[k], [ref32[k]], tag, M_F64))
    if N == 1 and kind in ("Instance", "Pair"):
        got = _roundtrip(kind, x.to(dev), gout.to(dev), None, w.to(dev), b.to(dev))
        assert not bool(got["y"].any()) and not bool(got["dx"].any())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NR.KINDS)
def test_a_constant_column_is_exactly_zero(kind):
    """Column 0 is the constant 3.3 (not a sum of few powers of two): its centred value is exactly 0 in Instance and Pair,
    in y and - gout being constant there as well - in dx; Layer and GraphSize only have to stay finite and right."""
    dev = _dev()
    x, gout, res, w, b = _inputs(300, 8, "randn", seed=5)
    x[:, 0], gout[:, 0] = 3.3, 0.7
    got = _roundtrip(kind, x.to(dev), gout.to(dev), None, w.to(dev), b.to(dev))
    ref64 = _reference(kind, x, gout, None, w, b, torch.float64)
    ref32 = _reference(kind, x, gout, None, w, b, torch.float32)
    if kind in ("Instance", "Pair"):
        assert not bool(got["y"][:, 0].any()) and not bool(got["dx"][:, 0].any())
        for k in ("y", "dx"):       # (the yardstick itself is rounding noise times 316 in that column: compare the others)
            PF.close_to_f64(got[k][:, 1:], ref64[k][:, 1:], [ref32[k][:, 1:]], f"{kind} constant column {k}", M_F64)
    else:
        for k in ref64:
            PF.close_to_f64(got[k], ref64[k], [ref32[k]], f"{kind} constant column {k}", M_F64)


def _close(got, ref, name):
    got, ref = got.double(), ref.double()
    err = (got - ref).abs()
    bound = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    assert bool((err <= bound).all()), (name, float(err.max()))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("cap,live,C", [(300, 257, 104), (5000, 4100, 104), (5000, 37, 104), (300, 257, 33)])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_rows_beyond_the_live_count_are_left_alone(kind, cap, live, C):
    """A capacity with fewer live rows: the dead rows of x, gout and the residual hold 1e30, out and gx a sentinel, the
    workspace NaN in every double, and the round trip runs twice on it (a partial that was never written, or a dead row that
    was summed, shows).  Live rows equal the exact-shape run within the golden tolerances, dead rows keep the sentinel bit for
    bit, Layer's parameter gradients and the saved coefficients are those of the live rows.  (5000, 37): most statistics blocks
    have no live row at all; C = 33: the scalar path."""
    dev = _dev()
    x, gout, res, w, b = _inputs(live, C, "randn", seed=cap)
    exact = _roundtrip(kind, x.to(dev), gout.to(dev), res.to(dev), w.to(dev), b.to(dev))
    pad = lambda t: torch.cat([t, torch.full((cap - live, C), 1e30)]).to(dev)
    got = _roundtrip(kind, pad(x), pad(gout), pad(res), w.to(dev), b.to(dev), live=live, ws_fill=0xFF, runs=2)
    for k in ("y", "dx"):
        assert bool(torch.isfinite(got[k]).all()), k
        _close(got[k][:live], exact[k], f"{kind} cap {cap} live {live} {k}")
        assert torch.equal(_bits(got[k][live:]), _bits(torch.full((cap - live, C), -7.0))), k
    for k in ("dweight", "dbias", "saved"):
        if k in got:
            _close(got[k], exact[k], f"{kind} cap {cap} live {live} {k}")
    assert float(got["saved"][2 * C + 3]) == live


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NR.KINDS)
def test_two_runs_give_identical_bits(kind):
    dev = _dev()
    for N, C in [(5000, 104), (257, 33)]:
        x, gout, res, w, b = (t.to(dev) for t in _inputs(N, C, "randn", seed=9))
        one = _roundtrip(kind, x, gout, res, w, b, ws_fill=0xFF)
        two = _roundtrip(kind, x, gout, res, w, b, ws_fill=0x00)
        assert sorted(one) == sorted(two)
        for k in one:
            assert torch.equal(_bits(one[k]), _bits(two[k])), (kind, N, C, k)
