"""kpgnn_sage_tail_fwd / _bwd (csrc/sage_tail.hip) through the C ABI and ops_dense.sage_tail.

CPU: both entries reject malformed descriptors before any device call, N == 0 launches nothing, the binding matches the header,
the size function answers 0 beyond the limits, and CPU tensors keep the layer's framework expression bit for bit.  GPU: forward
and every gradient are held to the float64 framework expression and its autograd with the fp32 CPU evaluation (at PF.THREADS
thread counts) as the yardstick; a dead hop slot gives exact zeros; the results are bitwise reproducible, independent of N, and
the evaluation form (nothing saved) gives the same bits."""
import ctypes
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import parity_f64 as PF

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
OK, EINVAL, ELIMIT = 0, -1, -3
FWD, BWD, SIZE = "kpgnn_sage_tail_fwd", "kpgnn_sage_tail_bwd", "kpgnn_sage_tail_workspace_bytes"
M_F64 = 3
ROOT = Path(__file__).resolve().parents[1]

# (N, K, DI, DO, H, theta): one row + scalar staging + H no multiple of 4; a full tile and a one-row tail; the golden's shape
# (vector staging of x, DI != DO); the plain [N,K,DO] output; K == 1; two column tiles with 2 DI = 64; DI just past one column
# tile with a tiny DO
SHAPES = [(1, 3, 11, 11, 33, True), (33, 3, 11, 11, 0, True), (257, 8, 13, 5, 40, True), (100, 8, 13, 5, 0, False),
          (65, 1, 8, 8, 0, False), (70, 2, 32, 32, 64, True), (40, 2, 17, 3, 7, True)]
NARROW = (70001, 1, 4, 4, 0, False)               # ceil(N / 32) = 2188 tiles: more than any backward grid (asserted)


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _slab_floats(K, DI, DO, H):
    """Slab row width the size function counts (include/kpgnn.h): [dW | db | dtheta | dWc | dbc]."""
    return K * 2 * DI * DO + 2 * K * DO + H * DO + H


def _desc(lib=None, N=100, K=3, DI=11, DO=11, H=33, **kw):
    """A descriptor that passes every check of both entries (all pointers dummies); kw overrides."""
    from kp_gnn_amd import _lib
    d = _lib.SageTailDesc()
    d.N, d.K, d.DI, d.DO, d.H = N, K, DI, DO, H
    for f in ("x", "xn", "w", "b", "theta", "bc", "y", "rinv", "out", "gout", "gx", "gxn", "gflat", "workspace"):
        setattr(d, f, A)
    d.wc = A if H > 0 else None
    d.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------ CPU
COMMON_BAD = [dict(N=-1), dict(K=0), dict(K=-2), dict(DI=0), dict(DI=-1), dict(DO=0), dict(DO=-3), dict(H=-1),
              dict(x=None), dict(xn=None), dict(w=None), dict(b=None),
              dict(theta=None), dict(H=0, wc=A, theta=None),          # wc without theta
              dict(wc=None), dict(H=0, wc=A)]                         # H and wc disagree
FWD_BAD = COMMON_BAD + [dict(out=None), dict(H=0, theta=None, y=None, rinv=None), dict(y=None), dict(rinv=None)]
BWD_BAD = COMMON_BAD + [dict(gout=None), dict(gx=None), dict(gxn=None), dict(gflat=None), dict(y=None), dict(rinv=None),
                        dict(workspace=None), dict(workspace_bytes=0), dict(workspace_bytes="one short")]


def test_null_descriptors_are_rejected(lib):
    for name in (FWD, BWD):
        assert getattr(lib, name)(None, None) == EINVAL, name
        assert name.encode() + b": NULL descriptor" in lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", FWD_BAD, ids=repr)
def test_malformed_forward_descriptors_are_rejected(lib, kw):
    """-1 with a message naming the entry, before any device call (the stream is NULL and every pointer a dummy)."""
    assert lib.kpgnn_sage_tail_fwd(ctypes.byref(_desc(**kw)), None) == EINVAL, kw
    assert FWD.encode() in lib.kpgnn_last_error(), lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", BWD_BAD, ids=repr)
def test_malformed_backward_descriptors_are_rejected(lib, kw):
    kw = dict(kw)
    if kw.get("workspace_bytes") == "one short":
        kw["workspace_bytes"] = int(lib.kpgnn_sage_tail_workspace_bytes(100, 3, 11, 11, 33)) - 1
    assert lib.kpgnn_sage_tail_bwd(ctypes.byref(_desc(**kw)), None) == EINVAL, kw
    assert BWD.encode() in lib.kpgnn_last_error(), lib.kpgnn_last_error()


def test_beyond_the_limits_is_elimit_and_no_rows_is_ok(lib):
    for kw in (dict(DI=33), dict(DO=33), dict(H=1025), dict(K=33), dict(K=9, DI=17)):
        assert lib.kpgnn_sage_tail_fwd(ctypes.byref(_desc(**kw)), None) == ELIMIT, kw
        assert b"sage_tail" in lib.kpgnn_last_error()
        assert lib.kpgnn_sage_tail_bwd(ctypes.byref(_desc(**kw)), None) == ELIMIT, kw
    # N == 0 launches nothing; what the forward does not use may be NULL (the evaluation form saves nothing)
    assert lib.kpgnn_sage_tail_fwd(ctypes.byref(_desc(N=0)), None) == OK
    d = _desc(N=0, y=None, rinv=None, gout=None, gx=None, gxn=None, gflat=None, workspace=None, workspace_bytes=0, bc=None)
    assert lib.kpgnn_sage_tail_fwd(ctypes.byref(d), None) == OK
    assert lib.kpgnn_sage_tail_fwd(ctypes.byref(_desc(N=0, H=0, theta=None, out=None)), None) == OK     # the plain mode


def test_the_size_function(lib):
    f = lib.kpgnn_sage_tail_workspace_bytes
    for N, K, DI, DO, H, _ in SHAPES + [NARROW]:
        nbytes = int(f(N, K, DI, DO, H))
        row = 4 * _slab_floats(K, DI, DO, H)
        assert nbytes > 0 and nbytes % row == 0 and 1 <= nbytes // row <= (N + 31) // 32, (N, K, DI, DO, H)
    assert f(1, 3, 11, 11, 33) == 4 * _slab_floats(3, 11, 11, 33)
    for bad in ((100, 3, 33, 11, 0), (100, 3, 11, 33, 0), (100, 3, 11, 11, 1025), (0, 3, 11, 11, 0), (100, 0, 11, 11, 0),
                (100, 3, 0, 11, 0), (100, 3, 11, 0, 0), (100, 3, 11, 11, -1), (100, 33, 4, 4, 0)):
        assert f(*bad) == 0, bad
    # K * ceil(D / 16)^2 <= 32 weight-gradient tiles: 32 one-tile hops and 8 four-tile hops fit, 9 four-tile hops do not
    assert f(100, 32, 4, 4, 0) > 0 and f(100, 8, 20, 20, 0) > 0 and f(100, 9, 32, 32, 0) == 0


def test_the_entries_are_bound_as_the_header_declares(lib):
    from kp_gnn_amd import _lib
    header = (ROOT / "include" / "kpgnn.h").read_text()
    body = re.search(r"typedef struct kpgnn_sage_tail_desc \{(.*?)\} kpgnn_sage_tail_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, ctype = [], {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ptr = "*" in decl
        base = decl.replace("const", "").replace("*", " ").split()
        for name in "".join(base[1:]).split(","):
            fields.append((name, ctypes.c_void_p if ptr else ctype[base[0]]))
    assert [(n, t) for n, t in _lib.SageTailDesc._fields_] == fields
    assert [n for n, _ in fields] == ["N", "K", "DI", "DO", "H", "x", "xn", "w", "b", "theta", "wc", "bc", "y", "rinv", "out",
                                      "gout", "gx", "gxn", "gflat", "workspace", "workspace_bytes"]
    for name in (FWD, BWD):
        assert re.search(r"int %s\(const kpgnn_sage_tail_desc\* d, kpgnn_stream_t stream\);" % name, header)
        fn = getattr(lib, name)
        assert fn.argtypes == [ctypes.POINTER(_lib.SageTailDesc), ctypes.c_void_p] and fn.restype == ctypes.c_int
    assert re.search(r"size_t %s\(int64_t N, int32_t K, int32_t DI, int32_t DO, int32_t H\);" % SIZE, header)
    fn = getattr(lib, SIZE)
    assert fn.restype == ctypes.c_size_t
    assert fn.argtypes == [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]


def _layer_expression(layer, x, x_n):
    """The tail of KPGraphSAGEConv.forward as it stood before kpgnn_sage_tail_* (layers/KPGraphSAGE.py)."""
    h = torch.cat([x, x_n], dim=-1).transpose(0, 1)
    h = torch.baddbmm(layer.hop_bias.unsqueeze(1), h, layer.hop_proj).transpose(0, 1)
    h = F.normalize(F.relu(h), p=2, dim=-1)
    return layer.combine_proj(layer.combine(h))


def test_the_switch_is_on_by_default_and_cpu_tensors_keep_the_framework_expression(lib, monkeypatch):
    """on by default.  A CPU layer never reaches the native route (sage_tail itself refuses CPU tensors):
    output and gradients are bitwise the framework expression on the aggregation the layer computed."""
    from kp_gnn_amd import _lib, ops_dense
    from kp_gnn_amd.layers import KPGraphSAGE as mod
    assert ops_dense.native_sage_tail() is True
    prev = ops_dense.set_native_sage_tail(False)
    try:
        assert prev is True and ops_dense.native_sage_tail() is False
    finally:
        ops_dense.set_native_sage_tail(True)
    assert ops_dense.native_sage_tail() is True
    assert ops_dense.sage_tail_supported(8, 13, 5, 40) and ops_dense.sage_tail_supported(3, 11, 11)
    assert not ops_dense.sage_tail_supported(3, 40, 40, 120) and not ops_dense.sage_tail_supported(3, 11, 11, 1025)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(9, 3, 4, generator=g)
    with pytest.raises(_lib.KpgnnError):
        ops_dense.sage_tail(x, x, torch.randn(3, 8, 4, generator=g), torch.randn(3, 4, generator=g))
    with pytest.raises(_lib.KpgnnError):
        ops_dense.sage_tail(x, x, torch.randn(3, 8, 4), torch.randn(3, 4), wc=torch.randn(12, 4))
    # the layer on the CPU: the aggregation is replaced by a recorded stand-in (it has no CPU path), the tail is the layer's own
    torch.manual_seed(4)
    layer = mod.KPGraphSAGEConv(12, 12, 3, aggr="add", combine="geometric")
    x_n = torch.randn(9, 3, 4, generator=g)
    monkeypatch.setattr(mod, "khop_aggregate", lambda *a, **k: x_n)
    monkeypatch.setattr(mod.KPGraphSAGEConv, "_csr", lambda self, ei, ea, n: (None, 3))
    monkeypatch.setattr(mod, "sage_tail", lambda *a, **k: pytest.fail("the native route was taken on CPU tensors"))
    xin = x.reshape(9, 12).clone().requires_grad_(True)
    out = layer(xin, None, None)
    gout = torch.randn(9, 12, generator=g)
    used = list(layer.parameters())              # (the edge-code tables feed the stand-in only: their gradient is None)
    got = torch.autograd.grad(out, [xin] + used, gout, allow_unused=True)
    x2 = x.reshape(9, 12).clone().requires_grad_(True)
    want_out = _layer_expression(layer, x2.reshape(9, 3, 4), x_n)
    want = torch.autograd.grad(want_out, [x2] + used, gout, allow_unused=True)
    assert torch.equal(out, want_out)
    for a, b in zip(got, want):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    assert layer._fused_tail is None                 # (no route was decided: the device decides at its first forward)


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(N, K, DI, DO, H, theta, seed=None, cap=None):
    """CPU fp32 inputs; with cap, `cap` rows are drawn and the first N of them are a prefix of the larger problem."""
    g = torch.Generator().manual_seed(1000 * K + 10 * DI + DO if seed is None else seed)
    R = cap or N
    t = dict(x=torch.randn(R, K, DI, generator=g), xn=2.0 * torch.randn(R, K, DI, generator=g),
             w=torch.randn(K, 2 * DI, DO, generator=g) / (2 * DI) ** 0.5, b=0.1 * torch.randn(K, DO, generator=g))
    if theta:
        t["theta"] = torch.softmax(torch.randn(K, DO, generator=g), dim=0)
    if H:
        t["wc"] = torch.randn(H, DO, generator=g) / DO ** 0.5
        t["bc"] = torch.randn(H, generator=g)
    t["gout"] = torch.randn((R, H) if H else ((R, DO) if theta else (R, K, DO)), generator=g)
    return t


def _reference(t, dtype, threads=None):
    """The framework expression (layers/KPGraphSAGE.py, combine.py) and its autograd in `dtype` on the CPU."""
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        v = {k: q.detach().to(dtype).clone().requires_grad_(k != "gout") for k, q in t.items()}
        h = torch.cat([v["x"], v["xn"]], dim=-1).transpose(0, 1)
        h = torch.baddbmm(v["b"].unsqueeze(1), h, v["w"]).transpose(0, 1)
        y = F.normalize(F.relu(h), p=2, dim=-1)
        res = y
        if "theta" in v:
            res = torch.sum(y * v["theta"].unsqueeze(0), dim=-2)
        if "wc" in v:
            res = F.linear(res, v["wc"], v["bc"])
        names = [k for k in v if k != "gout"]
        grads = torch.autograd.grad(res, [v[k] for k in names], v["gout"])
    finally:
        torch.set_num_threads(before)
    out = {"y": y.detach()}
    if "theta" in v:
        out["out"] = res.detach()
    out.update({"d" + k: gk for k, gk in zip(names, grads)})
    return out


def _launch(t, N, K, DI, DO, H, save=True, backward=True, fill=-7.0):
    """Forward (+ backward) on the device through the C ABI, every output pre-filled with a sentinel.  Returns the results
    under the keys of _reference (+ rinv)."""
    from kp_gnn_amd import _lib
    dev = _dev()
    lib = _lib.load()
    v = {k: q.to(dev).contiguous() for k, q in t.items()}
    theta = "theta" in v
    o = {}
    if save:
        o["y"] = torch.full((N, K, DO), fill, device=dev)
        o["rinv"] = torch.full((N, K), fill, device=dev)
    if theta:
        o["out"] = torch.full((N, H if H else DO), fill, device=dev)
    d = _lib.SageTailDesc()
    d.N, d.K, d.DI, d.DO, d.H = N, K, DI, DO, H
    for k in ("x", "xn", "w", "b", "theta", "wc", "bc"):
        if k in v:
            setattr(d, k, v[k].data_ptr())
    for k in ("y", "rinv", "out"):
        if k in o:
            setattr(d, k, o[k].data_ptr())
    _lib.launch(FWD, dev, ctypes.byref(d))
    if backward:
        sizes = [("dw", (K, 2 * DI, DO)), ("db", (K, DO))] + ([("dtheta", (K, DO))] if theta else []) \
            + ([("dwc", (H, DO)), ("dbc", (H,))] if H else [])
        total = sum(torch.Size(s).numel() for _, s in sizes)
        gflat = torch.full((total,), fill, device=dev)
        o["dx"], o["dxn"] = torch.full((N, K, DI), fill, device=dev), torch.full((N, K, DI), fill, device=dev)
        nbytes = int(lib.kpgnn_sage_tail_workspace_bytes(max(N, 1), K, DI, DO, H))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d.gout, d.gx, d.gxn, d.gflat = v["gout"].data_ptr(), o["dx"].data_ptr(), o["dxn"].data_ptr(), gflat.data_ptr()
        d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
        _lib.launch(BWD, dev, ctypes.byref(d))
        off = 0
        for k, s in sizes:
            n = torch.Size(s).numel()
            o[k] = gflat[off:off + n].view(s)
            off += n
    torch.cuda.synchronize()
    return o


def _compare(name, t, N, K, DI, DO, H):
    ref64 = _reference(t, torch.float64)
    ref32 = [_reference(t, torch.float32, threads=n) for n in PF.THREADS]
    got = _launch(t, N, K, DI, DO, H)
    rinv = got.pop("rinv")
    PF.print_ratios(name, PF.close_to_f64(got, ref64, ref32, name, M_F64))
    # rinv: 1 / rinv is the row norm to 1e-5 of the largest |z| (a norm is a sum of z's that may cancel); 1 / eps where clamped
    z = torch.baddbmm(t["b"].double().unsqueeze(1), torch.cat([t["x"], t["xn"]], -1).double().transpose(0, 1),
                      t["w"].double()).transpose(0, 1)
    nrm = F.relu(z).norm(dim=-1)
    live = nrm > 1e-12
    assert bool(((1.0 / rinv.cpu().double()[live] - nrm[live]).abs() <= 1e-5 * float(z.abs().max())).all()), name + ": rinv"
    assert bool((rinv.cpu()[~live] == torch.tensor(1.0) / torch.tensor(1e-12)).all()), name + ": rinv where clamped"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("N,K,DI,DO,H,theta", SHAPES)
def test_forward_and_backward_vs_float64(N, K, DI, DO, H, theta):
    """x = randn, xn = 2 randn, W = randn / sqrt(2 DI), b = 0.1 randn, theta = softmax(randn), Wc = randn / sqrt(DO), gout = randn.
    y, out and the gradients into x, xn, W, b, theta, Wc, bc through close_to_f64 with M = 3: ref64 is the framework expression
    cat -> baddbmm -> relu -> F.normalize -> theta-sum -> F.linear and its autograd in float64 on the CPU, the yardstick the
    same in fp32 on the CPU at 4, 8 and 16 threads."""
    name = f"sage_tail N{N} K{K} DI{DI} DO{DO} H{H}" + ("" if theta else " plain")
    _compare(name, _inputs(N, K, DI, DO, H, theta), N, K, DI, DO, H)


@pytest.mark.gpu
def test_a_block_that_walks_several_tiles():
    """K = 1, DI = DO = 4, 70,001 rows: ceil(N / 32) = 2188 tiles against a backward grid of (workspace bytes / slab row bytes)
    blocks, so blocks walk at least two tiles (asserted) - the prefetch across the tile loop and the accumulation of the
    weight-gradient tiles over a block's tiles."""
    from kp_gnn_amd import _lib
    N, K, DI, DO, H, theta = NARROW
    grid = int(_lib.load().kpgnn_sage_tail_workspace_bytes(N, K, DI, DO, H)) // (4 * _slab_floats(K, DI, DO, H))
    assert grid >= 1 and (N + 31) // 32 > grid, grid
    _compare(f"sage_tail narrow N{N}", _inputs(N, K, DI, DO, H, theta), N, K, DI, DO, H)


@pytest.mark.gpu
@pytest.mark.parametrize("H,theta", [(33, True), (0, True), (0, False)])
def test_a_dead_slot_gives_exact_zeros(H, theta):
    """Hop 1's bias at -100: relu(z) is all zero in that slot of every node.  y is exactly 0 there (the clamp keeps 0 / 0 out),
    and so are the slot's dW, db, dtheta, gx and gxn; every output is finite, and the live slots still match float64."""
    N, K, DI, DO = 45, 3, 11, 11
    t = _inputs(N, K, DI, DO, H, theta, seed=77)
    t["b"][1] = -100.0
    got = _compare(f"sage_tail dead slot H{H} theta{theta}", t, N, K, DI, DO, H)
    for k, q in got.items():
        assert bool(torch.isfinite(q).all()), k
    assert bool((got["y"][:, 1] == 0).all())
    for k in ("dx", "dxn"):
        assert bool((got[k][:, 1] == 0).all()), k
    for k in ("dw", "db") + (("dtheta",) if theta else ()):
        assert bool((got[k][1] == 0).all()), k
        assert bool((got[k][0] != 0).any()), k
    r = _launch(t, N, K, DI, DO, H, backward=False)["rinv"]
    assert bool((r[:, 1].cpu() == torch.tensor(1.0) / torch.tensor(1e-12)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("H,theta", [(40, True), (0, True), (0, False)])
def test_bitwise_reproducible_and_independent_of_the_row_count(H, theta):
    """Two runs on the same inputs are bitwise equal in every output.  The first 257 rows of the same data embedded in N = 300
    (another grid, another tail tile) give bitwise the same y / out / gx / gxn (the parameter gradients sum over other rows).
    With theta the evaluation form (y = rinv = NULL) gives bitwise the out of the saving form."""
    N, CAP, K, DI, DO = 257, 300, 8, 13, 5
    big = _inputs(CAP, K, DI, DO, H, theta, seed=5)
    small = {k: (q[:N].contiguous() if k in ("x", "xn", "gout") else q) for k, q in big.items()}
    a, b = _launch(small, N, K, DI, DO, H), _launch(small, N, K, DI, DO, H)
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
        assert not bool((a[k] == -7.0).all()), k
    wide = _launch(big, CAP, K, DI, DO, H)
    for k in ("y", "rinv", "dx", "dxn") + (("out",) if theta else ()):
        assert torch.equal(_bits(wide[k][:N]), _bits(a[k])), k
    if theta:
        ev = _launch(small, N, K, DI, DO, H, save=False, backward=False)
        assert sorted(ev) == ["out"] and torch.equal(_bits(ev["out"]), _bits(a["out"]))


@pytest.mark.gpu
def test_no_rows_zero_fills_the_parameter_gradients():
    from kp_gnn_amd import _lib
    dev = _dev()
    K, DI, DO, H = 3, 11, 11, 33
    t = {k: q.to(dev) for k, q in _inputs(1, K, DI, DO, H, True).items()}
    total = K * 2 * DI * DO + 2 * K * DO + H * DO + H
    gflat = torch.full((total + 8,), -7.0, device=dev)
    d = _lib.SageTailDesc()
    d.N, d.K, d.DI, d.DO, d.H = 0, K, DI, DO, H
    for k in ("x", "xn", "w", "b", "theta", "wc", "bc", "gout"):
        setattr(d, k, t[k].data_ptr())
    d.y = d.rinv = d.gx = d.gxn = d.out = t["x"].data_ptr()     # (not touched with N == 0)
    d.gflat = gflat.data_ptr()
    _lib.launch(FWD, dev, ctypes.byref(d))
    _lib.launch(BWD, dev, ctypes.byref(d))
    torch.cuda.synchronize()
    assert bool((gflat[:total] == 0).all()) and bool((gflat[total:] == -7.0).all())


@pytest.mark.gpu
def test_the_autograd_function_matches_the_c_abi_and_saves_nothing_under_no_grad():
    """ops_dense.sage_tail: gradients bitwise those of the direct launches; under no_grad with theta no [N,K,DO] tensor is
    allocated (peak memory stays below the saved y's size on top of the inputs and out)."""
    from kp_gnn_amd import ops_dense
    dev = _dev()
    N, K, DI, DO, H = 257, 8, 13, 5, 40
    t = _inputs(N, K, DI, DO, H, True)
    raw = _launch(t, N, K, DI, DO, H)
    v = {k: q.to(dev).requires_grad_(k != "gout") for k, q in t.items()}
    out = ops_dense.sage_tail(v["x"], v["xn"], v["w"], v["b"], theta=v["theta"], wc=v["wc"], bc=v["bc"])
    names = ["x", "xn", "w", "b", "theta", "wc", "bc"]
    grads = torch.autograd.grad(out, [v[k] for k in names], v["gout"])
    assert torch.equal(_bits(out), _bits(raw["out"]))
    for k, gk in zip(names, grads):
        assert torch.equal(_bits(gk), _bits(raw["d" + k])), k
    N2 = 20000
    t2 = {k: q.to(dev) for k, q in _inputs(N2, K, DI, DO, H, True).items()}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    with torch.no_grad():
        o2 = ops_dense.sage_tail(t2["x"], t2["xn"], t2["w"], t2["b"], theta=t2["theta"], wc=t2["wc"], bc=t2["bc"])
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(dev) - base
    assert extra < 4 * N2 * H + 4 * N2 * K * DO // 2, extra
    assert bool(torch.isfinite(o2).all())
