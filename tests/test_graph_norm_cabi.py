"""kpgnn_graph_norm_fwd / _bwd (csrc/body_norm_graph.hip) through the C ABI.

CPU: both entries reject malformed descriptors before any device call; N == 0 and G == 0 launch nothing.  GPU: every kind on
every pointer of tests/graph_norm_cases.py against tests/graph_norm_ref.py in float64, graph by graph
(|got - ref| <= ATOL * max|ref| + RTOL * |ref|, the maximum over the graph's OWN block, so a block the reference has as zeros
must be zeros); rows beyond the live count and beyond the pointer keep a NaN sentinel bit for bit while the live rows keep the
bits of the exact-shape run; and the bits of a graph's rows do not depend on G, the graph's position, the other graphs or the
capacity.

Layer on a constant block (one row of one column here): torch.std's gradient at 0 is 0, which is what the kernel does (K = 0),
so the float64 reference is finite there and the same bound applies."""
import ctypes

import pytest
import torch

import graph_norm_cases as GC
import graph_norm_ref as GR
import norm_ref as NR
import parity_f64 as PF

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
OK, EINVAL, ELIMIT = 0, -1, -3
KIND_ID = {"Layer": 0, "Instance": 1, "GraphSize": 2, "Pair": 3}
FWD, BWD = "kpgnn_graph_norm_fwd", "kpgnn_graph_norm_bwd"
RTOL, ATOL = PF.RTOL, PF.ATOL
SENTINEL = 0x7FC12345                             # a quiet NaN with a payload no arithmetic produces


def _T():
    from kp_gnn_amd import _lib
    return _lib.GRAPH_NORM_BLOCK_ROWS


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


# ------------------------------------------------------------------------------------------------ CPU
def _desc(lib, N=100, G=4, C=32, kind=0, **kw):
    """A descriptor that passes every check of both entries (all pointers dummies); kw overrides."""
    from kp_gnn_amd import _lib
    d = _lib.GraphNormDesc()
    d.N, d.G, d.C, d.kind, d.eps = N, G, C, kind, 1e-5
    d.x, d.x_stride, d.weight, d.bias, d.residual, d.res_stride = A, C, A, A, A, C
    d.out, d.out_stride, d.saved, d.graph_ptr = A, C, A, A
    d.gout, d.gout_stride, d.gx, d.gx_stride, d.gweight, d.gbias = A, C, A, C, A, A
    d.workspace = A
    d.workspace_bytes = lib.kpgnn_graph_norm_workspace_bytes(max(N, 0), max(G, 0), C, kind) if 1 <= C <= 256 else 1 << 20
    for k, v in kw.items():
        setattr(d, k, v)
    return d


COMMON_BAD = [dict(C=0), dict(C=-4), dict(C=257), dict(kind=-1), dict(kind=4), dict(N=-1), dict(G=-1), dict(x=None),
              dict(graph_ptr=None), dict(kind=0, weight=None), dict(x_stride=31), dict(eps=-1.0)]
FWD_BAD = COMMON_BAD + [dict(out=None), dict(out_stride=31), dict(res_stride=31)]
BWD_BAD = COMMON_BAD + [dict(gout=None), dict(gx=None), dict(gout_stride=31), dict(gx_stride=31), dict(workspace=None),
                        dict(workspace_bytes=0)]


@pytest.mark.parametrize("name,bad", [(FWD, FWD_BAD), (BWD, BWD_BAD)], ids=["fwd", "bwd"])
def test_malformed_descriptors_are_rejected_before_any_device_call(lib, name, bad):
    """A message naming the entry (the stream is NULL and every pointer a dummy); C > 256 is a limit, the rest invalid."""
    assert getattr(lib, name)(None, None) == EINVAL
    assert name.encode() + b": NULL descriptor" in lib.kpgnn_last_error()
    for kw in bad:
        rc = getattr(lib, name)(ctypes.byref(_desc(lib, **kw)), None)
        assert rc == (ELIMIT if kw.get("C", 0) > 256 else EINVAL), (kw, rc)
        assert name.encode() in lib.kpgnn_last_error(), lib.kpgnn_last_error()


def test_sizes_and_what_launches_nothing(lib):
    need = lib.kpgnn_graph_norm_workspace_bytes(5000, 200, 104, 0)
    assert need >= (200 + 200 // 8) * 2 * 104 * 8 and need % 16 == 0
    assert lib.kpgnn_graph_norm_bwd(ctypes.byref(_desc(lib, N=5000, G=200, C=104, workspace_bytes=need - 1)), None) == EINVAL
    assert b"workspace" in lib.kpgnn_last_error()
    for kind in (1, 2, 3):                              # only Layer's parameter gradients need one
        assert lib.kpgnn_graph_norm_workspace_bytes(5000, 200, 104, kind) == 0
    assert lib.kpgnn_graph_norm_saved_floats(200, 104, 0) == 800
    for G, C, kind in [(-1, 8, 0), (4, 0, 0), (4, 257, 0), (4, 8, 4)]:
        assert lib.kpgnn_graph_norm_saved_floats(G, C, kind) == 0
    assert lib.kpgnn_graph_norm_workspace_bytes(-1, 4, 8, 0) == 0 and lib.kpgnn_graph_norm_workspace_bytes(10, 4, 257, 0) == 0
    for kind in range(4):
        for N, G in [(0, 4), (100, 0), (0, 0)]:         # no rows or no graphs: nothing is launched (the stream is NULL)
            w = A if kind == 0 else None
            d = _desc(lib, N=N, G=G, kind=kind, weight=w, bias=None, residual=None, saved=None, gout=None, gx=None,
                      gweight=None, gbias=None, workspace=None, workspace_bytes=0)
            assert lib.kpgnn_graph_norm_fwd(ctypes.byref(d), None) == OK, (kind, N, G)
            d = _desc(lib, N=N, G=G, kind=kind, weight=w, bias=None, residual=None, saved=None, out=None, gweight=None,
                      gbias=None, workspace=None, workspace_bytes=0)
            assert lib.kpgnn_graph_norm_bwd(ctypes.byref(d), None) == OK, (kind, N, G)
    assert lib.kpgnn_graph_norm_fwd(ctypes.byref(_desc(lib, N=0, C=256)), None) == OK          # the maximal C is accepted


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _sentinel(shape, dev):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)


def _roundtrip(kind, x, gout, res, w, b, ptr, live=None, ws_fill=0xFF, cap=None):
    """{y, dx[, dweight, dbias], saved} of one forward + backward through the C ABI.  x / gout / res: CPU tensors of the live
    rows; cap: the capacity the device buffers get (dead rows of the inputs hold 1e30); ptr: the graph pointer (list); live: the
    device-side row count (n_dyn).  out and gx start as the NaN sentinel everywhere, the workspace as `ws_fill` bytes."""
    from kp_gnn_amd import _lib
    dev = _dev()
    n, C = x.shape
    N = n if cap is None else cap
    pad = lambda t: None if t is None else torch.cat([t, torch.full((N - n, C), 1e30)]).to(dev)
    x, gout, res = pad(x), pad(gout), pad(res)
    G = len(ptr) - 1
    gptr = torch.tensor(ptr, dtype=torch.int32, device=dev)
    out, gx = _sentinel((N, C), dev), _sentinel((N, C), dev)
    saved = torch.full((max(G, 1), 4), -7.0, device=dev)
    gw, gb = torch.full((C,), -7.0, device=dev), torch.full((C,), -7.0, device=dev)
    nbytes = _lib.load().kpgnn_graph_norm_workspace_bytes(N, G, C, KIND_ID[kind])
    ws = torch.full((max(nbytes, 16),), ws_fill, dtype=torch.uint8, device=dev)
    n_dyn = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev)
    d = _lib.GraphNormDesc()
    d.N, d.G, d.C, d.kind, d.eps = N, G, C, KIND_ID[kind], 1e-5
    d.graph_ptr = gptr.data_ptr()
    d.x, d.x_stride, d.out, d.out_stride, d.saved = x.data_ptr(), C, out.data_ptr(), C, saved.data_ptr()
    d.gout, d.gout_stride, d.gx, d.gx_stride = gout.data_ptr(), C, gx.data_ptr(), C
    if kind == "Layer":
        w, b = w.to(dev), b.to(dev)
        d.weight, d.bias, d.gweight, d.gbias = w.data_ptr(), b.data_ptr(), gw.data_ptr(), gb.data_ptr()
    if res is not None:
        d.residual, d.res_stride = res.data_ptr(), C
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    if n_dyn is not None:
        d.n_dyn = n_dyn.data_ptr()
    _lib.launch(FWD, dev, ctypes.byref(d))
    _lib.launch(BWD, dev, ctypes.byref(d))
    torch.cuda.synchronize()
    got = {"y": out.cpu(), "dx": gx.cpu(), "saved": saved.cpu()}
    if kind == "Layer":
        got["dweight"], got["dbias"] = gw.cpu(), gb.cpu()
    return got


def _reference(kind, x, gout, res, w, b, ptr, live=None):
    """{y, dx[, dweight, dbias]} of graph_norm_ref in float64 on the CPU through autograd."""
    dt = torch.float64
    x = x.to(dt).clone().requires_grad_(True)
    params = [t.to(dt).clone().requires_grad_(True) for t in (w, b)] if kind == "Layer" else []
    y = GR.norm(kind, x, ptr, *params, residual=None if res is None else res.to(dt), live=live)
    grads = torch.autograd.grad(y, [x] + params, gout.to(dt))
    out = {"y": y.detach(), "dx": grads[0]}
    if kind == "Layer":
        out["dweight"], out["dbias"] = grads[1], grads[2]
    return out


def _check_blocks(got, ref, ptr, name, live=None):
    """The bound of the module docstring, graph by graph; prints the worst ratio err / bound before it asserts."""
    worst, bad = 0.0, []
    for g, r0, r1 in GR.blocks(ptr, live):
        a, r = got[r0:r1].double(), ref[r0:r1]
        err = (a - r).abs()
        bound = ATOL * float(r.abs().max()) + RTOL * r.abs()
        ratio = float((err / bound.clamp(min=1e-300)).max())
        worst = max(worst, ratio)
        if not bool((err <= bound).all()):
            bad.append((g, r1 - r0, float(err.max()), float(r.abs().max())))
    print(f"[graph-norm] {name}: worst err / bound {worst:.3e}")
    assert not bad, (name, bad[:5])


def _check_vector(got, ref, name):
    err = (got.double() - ref).abs()
    bound = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    print(f"[graph-norm] {name}: worst err / bound {float((err / bound.clamp(min=1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), (name, float(err.max()))


CASE_NAMES = ["sizes", "shuffled", "empty-first-middle-last", "one-graph", "one-small-graph", "200-tiny"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_NAMES)
@pytest.mark.parametrize("kind", NR.KINDS)
def test_every_kind_and_case_against_float64(kind, case):
    """out and gx graph by graph, Layer's gweight / gbias as vectors, at every width, with a residual; and without one the
    exact answers: a one-row graph is zeros in out and gx (Instance, Pair), a one-element block exactly bias (Layer), both of
    which the per-block bound demands anyway wherever the reference is identically zero."""
    sizes = GC.cases(_T())[case]
    ptr = GC.ptr_of(sizes)
    N = ptr[-1]
    for C in GC.WIDTHS:
        x, gout, res, w, b = GC.inputs(N, C, seed=1)
        for r in (res, None):
            ref = _reference(kind, x, gout, r, w, b, ptr)
            got = _roundtrip(kind, x, gout, r, w, b, ptr)
            tag = f"{kind} {case} C={C}{'' if r is None else ' +res'}"
            for k in ("y", "dx"):
                assert not bool((_bits(got[k]) == SENTINEL).any()), tag     # every row belongs to a graph here
                _check_blocks(got[k], ref[k], ptr, f"{tag} {k}")
            for k in ("dweight", "dbias"):
                if k in ref:
                    _check_vector(got[k], ref[k], f"{tag} {k}")
        for g, r0, r1 in GR.blocks(ptr):          # (got: the run without a residual)
            if r1 - r0 == 1 and kind in ("Instance", "Pair"):
                assert not bool(got["y"][r0].any()) and not bool(got["dx"][r0].any()), (kind, case, C, g)
            if (r1 - r0) * C == 1 and kind == "Layer":
                assert torch.equal(got["y"][r0], b) and not bool(got["dx"][r0].any()), (kind, case, C, g)
            assert float(got["saved"][g, 3]) == r1 - r0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NR.KINDS)
def test_constant_columns_are_exactly_zero(kind):
    """Column 0 of every graph is the constant 3.3 with a constant gout: exactly 0 in out and gx for Instance and Pair (the
    reference is identically zero there); a constant block of Layer is exactly bias.  Wave teams and a block team."""
    T = _T()
    sizes = [2, 37, T + 7, 5]
    ptr = GC.ptr_of(sizes)
    x, gout, res, w, b = GC.inputs(ptr[-1], 8, seed=5)
    x[:, 0], gout[:, 0] = 3.3, 0.7
    x[ptr[1]:ptr[2]] = 1.7                          # the 37-row graph is one constant block
    x[ptr[2]:ptr[2] + T + 7, 1] = -0.3              # and the block team has a second constant column
    got = _roundtrip(kind, x, gout, None, w, b, ptr)
    ref = _reference(kind, x, gout, None, w, b, ptr)
    if kind in ("Instance", "Pair"):
        assert not bool(got["y"][:, 0].any()) and not bool(got["dx"][:, 0].any())
        assert not bool(got["y"][ptr[1]:ptr[2]].any())
    if kind == "Layer":
        assert torch.equal(got["y"][ptr[1]:ptr[2]], b.expand(37, 8))
    # (n copies of one fp32 value sum exactly in float64, so the reference's centred constant column is exactly 0 as well and
    #  the per-block bound asks for exact zeros there on its own)
    for k in ("y", "dx"):
        _check_blocks(got[k], ref[k], ptr, f"{kind} constant columns {k}")


def _dead_rows_case(kind, C, sizes, live, cap, ptr_live):
    """ptr (over `sizes`) may run past `live`; ptr_live is the same pointer clamped to live: the exact-shape run."""
    ptr = GC.ptr_of(sizes)
    x, gout, res, w, b = GC.inputs(live, C, seed=cap)
    exact = _roundtrip(kind, x, gout, res, w, b, ptr_live)
    got = _roundtrip(kind, x, gout, res, w, b, ptr, live=live, cap=cap, ws_fill=0x7F)
    for k in ("y", "dx"):
        assert torch.equal(_bits(got[k][:live]), _bits(exact[k])), (kind, C, k)
        assert bool((_bits(got[k][live:]) == SENTINEL).all()), (kind, C, k)
    for k in ("dweight", "dbias"):
        if k in got:
            assert torch.equal(_bits(got[k]), _bits(exact[k])), (kind, C, k)
    ref = _reference(kind, x, gout, res, w, b, ptr, live=live)
    for k in ("y", "dx"):
        _check_blocks(got[k][:live], ref[k], ptr, f"{kind} dead rows C={C} {k}", live=live)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [33, 104])
@pytest.mark.parametrize("kind", NR.KINDS)
def test_dead_rows_keep_the_sentinel_and_live_rows_their_bits(kind, C):
    """A capacity of 1.5 times the live rows with n_dyn given.  First with graph_ptr[G] == live; then with a pointer that runs
    past live: the last live graph is truncated (once inside a wave team, once cutting a block team down to a wave team) and
    the later graphs are wholly dead.  Dead rows of out and gx keep the NaN sentinel bit for bit - the dead rows of the inputs
    hold 1e30 - and live rows, and Layer's parameter gradients, have the bits of the exact-shape run."""
    T = _T()
    sizes = [5, 37, T + 9, 0, 23, 2 * T, 12]
    ptr = GC.ptr_of(sizes)
    live = ptr[-1]
    _dead_rows_case(kind, C, sizes, live, live + live // 2, ptr)
    for cut in (ptr[4] + 7, ptr[5] + 40, ptr[5] + T + 3):      # inside graph 4 (23 rows) / graph 5 (2T rows: to 40, to T + 3)
        clamped = [min(p, cut) for p in ptr]
        _dead_rows_case(kind, C, sizes, cut, cut + cut // 2, clamped)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NR.KINDS)
def test_a_graphs_bits_depend_on_that_graph_alone(kind):
    """40 graphs (wave teams, three block teams, an empty graph): every graph's rows of out and gx are the same bits alone
    (G == 1), in reversed graph order, with other graphs' values changed, at another capacity, and in a second run."""
    T = _T()
    g = torch.Generator().manual_seed(40)
    sizes = torch.randint(1, 41, (40,), generator=g).tolist()
    sizes[3], sizes[11], sizes[20], sizes[33] = T, 0, T + 1, 2 * T + 3
    ptr = GC.ptr_of(sizes)
    N = ptr[-1]
    for C in (33, 104):
        x, gout, res, w, b = GC.inputs(N, C, seed=2)
        base = _roundtrip(kind, x, gout, res, w, b, ptr)
        again = _roundtrip(kind, x, gout, res, w, b, ptr, ws_fill=0x00)
        for k in base:
            assert torch.equal(_bits(base[k]), _bits(again[k])), (kind, C, k, "second run")
        # another capacity
        big = _roundtrip(kind, x, gout, res, w, b, ptr, live=N, cap=2 * N + 5)
        # reversed graph order
        order = list(range(39, -1, -1))
        rows = torch.cat([torch.arange(ptr[i], ptr[i + 1]) for i in order])
        rptr = GC.ptr_of([sizes[i] for i in order])
        rev = _roundtrip(kind, x[rows], gout[rows], res[rows], w, b, rptr)
        # other graphs' values changed: every even graph gets new rows, the odd ones must not notice (and the other way round)
        x2, g2, r2, _, _ = GC.inputs(N, C, seed=77)
        changed = {}
        for parity in (0, 1):
            xa, ga, ra = x.clone(), gout.clone(), res.clone()
            for i in range(parity, 40, 2):
                xa[ptr[i]:ptr[i + 1]], ga[ptr[i]:ptr[i + 1]], ra[ptr[i]:ptr[i + 1]] = (t[ptr[i]:ptr[i + 1]] for t in (x2, g2, r2))
            changed[parity] = _roundtrip(kind, xa, ga, ra, w, b, ptr)
        for i in range(40):
            r0, r1 = ptr[i], ptr[i + 1]
            if r1 == r0:
                continue
            alone = _roundtrip(kind, x[r0:r1], gout[r0:r1], res[r0:r1], w, b, [0, r1 - r0])
            q0 = rptr[order.index(i)]
            for k in ("y", "dx"):
                want = _bits(base[k][r0:r1])
                assert torch.equal(_bits(alone[k]), want), (kind, C, i, sizes[i], k, "alone")
                assert torch.equal(_bits(big[k][r0:r1]), want), (kind, C, i, sizes[i], k, "capacity")
                assert torch.equal(_bits(rev[k][q0:q0 + r1 - r0]), want), (kind, C, i, sizes[i], k, "reversed")
                assert torch.equal(_bits(changed[1 - i % 2][k][r0:r1]), want), (kind, C, i, sizes[i], k, "others changed")
