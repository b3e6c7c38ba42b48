"""GPU (-m gpu): the bf16-split matrix kernels (csrc/bf3.h: lin3f_kernel, lin3_kernel modes 0 and 1, wgrad3_kernel) and the fp32
kernels they replace, held PER ELEMENT to float64 with the measure of tests/bf3_cases.py:

    rho(y) = max_ij |y_ij - y64_ij| / (u (sum_k |a_ik| |b_jk| + |bias_j|)),        rho(kernel) <= M * max(rho32, 1) + D

rho32: the fp32 CPU yardstick (bf3_cases.fp32_samples); D = 8 under set_dense_math("auto") (the worst sum of the three dropped
piece products, 7.83 u |a b|) and 0 under "f32"; M = bf3_cases.M.  tests/test_bf16_split_host.py proves on the CPU that at
every family and shape used here a kernel that loses ONE of the six products lands at least 4 times outside the bound.

Every case runs under "auto" AND under "f32", and under "auto" asserts that the split route ran: the scratch for the split copy
of W (0xFF bytes when handed out) was written, and under "f32" it was not; the weight gradient has no scratch, there the two
modes' results must differ in some bit on `ones`.  The `exact` family must come back bit for bit equal to float64 on every
route.  Every case prints its rho, rho32 and (rho - D) / max(rho32, 1)."""
import ctypes
import functools

import pytest
import torch

import bf3_cases as C
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

N, NW = C.N_FWD, C.N_WGRAD
MODES = ("auto", "f32")
SEED = 0            # the seed of tests/test_bf16_split_host.py: the same tensors


# ------------------------------------------------------------------------------------------------------------ harness
def _in_both_modes(run):
    """{mode: run(mode)} with "auto" restored whatever happens."""
    from kp_gnn_amd import ops_dense
    out = {}
    try:
        for mode in MODES:
            ops_dense.set_dense_math(mode)
            out[mode] = run(mode)
            torch.cuda.synchronize()
    finally:
        ops_dense.set_dense_math("auto")
    return out


@pytest.fixture
def scratch(monkeypatch):
    """Records what ops_dense._split_workspace hands out, filled with 0xFF (as tests/test_dynamic_rows_training.py does)."""
    from kp_gnn_amd import ops_dense
    rec, real = [], ops_dense._split_workspace

    def recording(*a):
        ws = real(*a)
        if ws is not None:
            ws.fill_(0xFF)
        rec.append(ws)
        return ws
    monkeypatch.setattr(ops_dense, "_split_workspace", recording)
    return rec


def _route(rec, mode, name, launches=1):
    """The bf16-split kernels write the split copy of W into the scratch first; the fp32 kernels never touch it."""
    torch.cuda.synchronize()
    assert len(rec) == launches and all(ws is not None for ws in rec), (name, mode, "no scratch was asked for")
    written = [bool((ws != 0xFF).any()) for ws in rec]
    assert all(written) if mode == "auto" else not any(written), (name, mode, written, "the other kernel family ran")
    del rec[:]


def _hold(name, mode, y, y64, den, r32, D=None):
    """rho(y) <= M max(rho32, 1) + D, printed first."""
    D = (C.D_SPLIT if mode == "auto" else 0) if D is None else D
    r = C.rho(y, y64, den)
    print(f"[bf3] {name} {mode}: rho {r:.3f}  rho32 {r32:.3f}  (rho - D) / max(rho32, 1) {max(r - D, 0.0) / max(r32, 1.0):.3f}")
    assert r <= C.bound(r32, C.M, D), (name, mode, r, r32, C.bound(r32, C.M, D))
    return r


def _exact(name, mode, y, y64):
    assert torch.equal(y.detach().cpu().double().reshape(y64.shape), y64), (name, mode, "the exact family is not exact")


# ------------------------------------------------------------------------------------------- kpgnn_linear_bn (lin3f_kernel)
def _lin_bn(x, w, bias, wt, epi, prepared=False):
    """y = x w^T + bias through ops_dense._lin_bn, pro 0; w [O, I] on the host, handed over as [I, O] when wt.  prepared: the
    split copy comes from kpgnn_linear_split_many (w_split_ready = 1) as ops_dense.prepare_mlp_splits registers it.
    Returns (y, the slot's column sums [2, O] or None)."""
    from kp_gnn_amd import _lib, ops_dense
    lib, dev = _lib.load(), _dev()
    n, I = x.shape
    O = w.shape[0]
    xd, bd = x.to(dev), bias.to(dev)
    wd = (w.t().contiguous() if wt else w.contiguous()).to(dev)
    y = torch.full((n, O), float("nan"), device=dev)
    kw = dict(N=n, O=O, I=I, x=xd, w=wd, bias=bd, y=y, pro=0, epi=epi, w_transposed=wt)
    slot = None
    if epi:
        slot = kw["out_slot"] = ops_dense.take_stat_slot(O, dev)
    try:
        if prepared:
            nb = int(lib.kpgnn_linear_split_workspace_bytes(O, I, 1))
            frag = torch.full((nb,), 0xFF, dtype=torch.uint8, device=dev)
            job = _lib.SplitJob()
            job.w, job.O, job.I, job.frag = wd.data_ptr(), O, I, frag.data_ptr()
            job.wn, job.wk = (1, O) if wt else (I, 1)
            _lib.launch("kpgnn_linear_split_many", dev, (_lib.SplitJob * 1)(job), 1)
            ops_dense._split_cache[(wd.data_ptr(), wt)] = (wd._version, O, I, frag)
        ops_dense._lin_bn(lib, dev, **kw)
        torch.cuda.synchronize()
    finally:
        ops_dense.invalidate_splits()
    sums = slot.cpu()[:ops_dense.STAT_REPLICAS * 2 * O].view(ops_dense.STAT_REPLICAS, 2, O).sum(0) if epi else None
    return y.cpu(), sums


def _hold_column_sums(name, mode, sums, y64, den, r32):
    """The slot of epi 1 against float64 sums of y64 and y64^2.  Every y_ij is within e_ij = B u den_ij of y64_ij (B = the bound
    above); the kernels add a tile's 16 values in fp32 before they join the float64 sums (16 roundings of u each, 17 with the
    square's), everything else is float64:
        |s0_j - sum_i y64|   <= sum_i e + 16 u sum_i (|y64| + e)
        |s1_j - sum_i y64^2| <= sum_i (2 |y64| e + e^2) + 17 u sum_i (|y64| + e)^2"""
    B = C.bound(r32, C.M, C.D_SPLIT if mode == "auto" else 0)
    e, a = B * C.U * den, y64.abs()
    b0 = e.sum(0) + 16 * C.U * (a + e).sum(0)
    b1 = (2 * a * e + e * e).sum(0) + 17 * C.U * ((a + e) ** 2).sum(0)
    e0, e1 = (sums[0] - y64.sum(0)).abs(), (sums[1] - (y64 * y64).sum(0)).abs()
    print(f"[bf3] {name} {mode}: column sums at {float((e0 / b0).max()):.3f} / {float((e1 / b1).max()):.3f} of their bounds")
    assert bool((e0 <= b0).all()) and bool((e1 <= b1).all()), (name, mode, float((e0 / b0).max()), float((e1 / b1).max()))


@pytest.mark.parametrize("epi", [0, 1])
@pytest.mark.parametrize("wt", [0, 1])
@pytest.mark.parametrize("I,O", C.LIN_BN_SHAPES)
@pytest.mark.parametrize("family", C.FWD_FAMILIES + ("exact",))
def test_linear_bn(family, I, O, wt, epi, scratch):
    """lin3f_kernel<KS, 0, EPI> (KS = 7, 2, 6) and lin_fused_kernel on 4129 rows (129 tiles of 32 and one row)."""
    x, _, w, bias, y64, den, r32 = C.reference(family, N, O, I, SEED, True, None)
    name = f"linear_bn {family} I{I} O{O} wt{wt} epi{epi}"

    def run(mode):
        y, sums = _lin_bn(x, w, bias, wt, epi)
        _route(scratch, mode, name)
        if family == "exact":
            _exact(name, mode, y, y64)
        else:
            _hold(name, mode, y, y64, den, r32)
        if epi:
            _hold_column_sums(name, mode, sums.double(), y64, den, r32)
        return y

    got = _in_both_modes(run)
    # the split made by kpgnn_linear_split_many instead of per call: the same bits
    y2, sums2 = _lin_bn(x, w, bias, wt, epi, prepared=True)
    assert not scratch, "a prepared split needs no scratch"
    assert torch.equal(y2, got["auto"]), (name, "prepared split != per-call split")
    if family == "ones":
        assert not torch.equal(got["auto"], got["f32"]), (name, "the two modes ran the same arithmetic")


# ------------------------------------------------------------------------- kpgnn_linear_group_fwd (lin3_kernel, mode 0)
def _group_fwd(a, b, bias, S, H):
    """relu(sum_l a[:, lH:(l+1)H] b[:, lH:(l+1)H]^T + bias) through ops_dense._jk_group_fwd."""
    from kp_gnn_amd import ops_dense
    dev = _dev()
    states = [a[:, l * H:(l + 1) * H].contiguous().to(dev) for l in range(S)]
    y = ops_dense._jk_group_fwd(b.contiguous().to(dev), bias.to(dev), states)
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("S,H,O", C.GROUP_SHAPES)
@pytest.mark.parametrize("family", C.FWD_FAMILIES + ("exact",))
def test_linear_group_fwd(family, S, H, O, scratch):
    """Against relu(y64): ReLU is 1-Lipschitz, the bound of the product applies."""
    family = C.group_fwd_family(family, (S, H, O))
    a, _, b, bias, y64, den, r32 = C.reference(family, N, O, S * H, SEED, True, None)
    name = f"group_fwd {family} S{S} H{H} O{O}"
    want = torch.relu(y64)

    def run(mode):
        y = _group_fwd(a, b, bias, S, H)
        _route(scratch, mode, name)
        if family == "exact":
            _exact(name, mode, y, want)
        else:
            _hold(name, mode, y, want, den, r32)
        return y

    got = _in_both_modes(run)
    if family not in C.POSITIVE:
        assert bool((got["auto"] > 0).any()) and bool((got["auto"] == 0).any()), "both sides of the ReLU"
    else:
        assert not torch.equal(got["auto"], got["f32"]), (name, "the two modes ran the same arithmetic")


# --------------------------------------------------------------- kpgnn_linear_fwd with blocked output (lin3_kernel, mode 1)
def _blocked(dy, mask, bt, S, H):
    """dx_l = (dy [mask > 0]) W_l as ops_dense.JKConcatLinear.backward fills the descriptor: W = bt^T [O, S H], the result S
    contiguous [N, H] blocks, returned as [N, S H]."""
    from kp_gnn_amd import _lib, ops_dense
    lib, dev = _lib.load(), _dev()
    n, O = dy.shape
    dyd, md, wd = dy.contiguous().to(dev), mask.contiguous().to(dev), bt.t().contiguous().to(dev)
    G = torch.full((S, n, H), float("nan"), device=dev)
    d = _lib.LinearDesc()
    d.N, d.O, d.I = n, S * H, O
    d.n_dyn = ops_dense.dyn_ptr(n)
    d.x, d.x_stride, d.w, d.y, d.y_stride = dyd.data_ptr(), O, wd.data_ptr(), G.data_ptr(), H
    d.w_transposed, d.y_block_cols, d.y_block_stride = 1, H, n * H
    d.x_mask = md.data_ptr()
    ws = ops_dense._split_workspace(lib, H, O, S, dev)
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    _lib.launch("kpgnn_linear_fwd", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    return G.cpu().permute(1, 0, 2).reshape(n, S * H)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("S,H,O", C.BLOCKED_SHAPES)
@pytest.mark.parametrize("family", C.FWD_FAMILIES + ("exact",))
def test_linear_fwd_blocked_output(family, S, H, O, masked, scratch):
    """An all-positive mask, and one that zeroes a third of dy's entries."""
    dy, mask, bt, _, y64, den, r32 = C.reference(family, N, S * H, O, SEED, False, None, masked)
    name = f"blocked {family} S{S} H{H} O{O}{' masked' if masked else ''}"
    assert bool((mask <= 0).any()) == masked

    def run(mode):
        y = _blocked(dy, mask, bt, S, H)
        _route(scratch, mode, name)
        if family == "exact":
            _exact(name, mode, y, y64)
        else:
            _hold(name, mode, y, y64, den, r32)
        return y

    got = _in_both_modes(run)
    if family == "ones":
        assert not torch.equal(got["auto"], got["f32"]), (name, "the two modes ran the same arithmetic")


def test_linear_fwd_refuses_a_blocked_output_of_128_columns_or_fewer():
    """(S, H, O) = (2, 32, 32): 64 columns in two blocks.  The entry point refuses it in both modes (ops_dense._jk_native_ok keeps
    such a projection on the framework path) - neither kernel family may be reached with it."""
    from kp_gnn_amd import _lib
    S, H, O = C.BLOCKED_REFUSED
    dy, mask, bt, _, _, _, _ = C.reference("randn", N, S * H, O, SEED, False, None, False)

    def run(mode):
        with pytest.raises(_lib.KpgnnError, match="blocked output needs O > 128"):
            _blocked(dy, mask, bt, S, H)
    _in_both_modes(run)


# --------------------------------------------------------------------------- the weight gradients (wgrad3_kernel / wgrad2)
def _wgrad_desc(dy, x, dw, db, ws, mask=None):
    from kp_gnn_amd import _lib, ops_dense
    d = _lib.WgradDesc()
    d.N, d.O, d.I = dy.shape[0], dy.shape[1], x.shape[1]
    d.n_dyn = ops_dense.dyn_ptr(dy.shape[0])
    d.dy, d.dy_stride, d.x, d.x_stride = dy.data_ptr(), dy.shape[1], x.data_ptr(), x.shape[1]
    d.dw, d.db = dw.data_ptr(), db.data_ptr()
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if mask is not None:
        d.dy_mask = mask.data_ptr()
    return d


@functools.lru_cache(maxsize=4)
def _wgrad_reference(family, O, I, seed, masked=False):
    """dW = dy^T x as the product a b^T with a = dy^T [O, N], b = x^T [I, N]; the yardstick leaves the sequential sample out.
    db = the column sums of dy, measured the same way against float64 with torch's fp32 sums as the yardstick.  `exact`: dy is
    the narrow side (its column sums are small integers)."""
    a, mask, b, _, y64, den, r32 = C.reference(family, O, I, NW, seed, False, False, masked, "b")
    dy = (a * (mask > 0)).t().contiguous()
    db64, dbden = dy.double().sum(0), dy.double().abs().sum(0)
    dbr32 = 0.0 if family == "exact" else _db_rho32(dy, db64, dbden)
    return a.t().contiguous(), mask.t().contiguous(), b.t().contiguous(), y64, den, r32, db64, dbden, dbr32


def _db_rho32(dy, db64, dbden):
    before = torch.get_num_threads()
    try:
        out = []
        for t in C.THREADS:
            torch.set_num_threads(t)
            out.append(C.rho(dy.sum(0), db64, dbden))
    finally:
        torch.set_num_threads(before)
    return max(out)


def _hold_wgrad(name, mode, family, dw, db, ref):
    _, _, _, y64, den, r32, db64, dbden, dbr32 = ref
    if family == "exact":
        _exact(name + " dW", mode, dw, y64)
        _exact(name + " db", mode, db, db64)
    else:
        _hold(name + " dW", mode, dw, y64, den, r32)
        _hold(name + " db", mode, db, db64, dbden, dbr32, D=0)        # (plain fp32 column sums in both modes: nothing is dropped)


@pytest.mark.parametrize("O,I", C.WGRAD_SHAPES)
@pytest.mark.parametrize("family", C.WGRAD_FAMILIES + ("exact",))
def test_linear_wgrad_and_pair(family, O, I):
    """kpgnn_linear_wgrad on one problem and kpgnn_linear_wgrad_pair on two of the same shape, 2081 rows (65 chunks and a row)."""
    from kp_gnn_amd import _lib
    lib, dev = _lib.load(), _dev()
    refs = [_wgrad_reference(family, O, I, s) for s in (SEED, SEED + 1)]
    dev_in = [(r[0].to(dev), r[2].to(dev)) for r in refs]
    nb = int(lib.kpgnn_wgrad_workspace_bytes(O, I))

    def run(mode):
        out = []
        dw, db = torch.full((O, I), float("nan"), device=dev), torch.full((O,), float("nan"), device=dev)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        _lib.launch("kpgnn_linear_wgrad", dev, ctypes.byref(_wgrad_desc(*dev_in[0], dw, db, ws)))
        torch.cuda.synchronize()
        _hold_wgrad(f"wgrad {family} O{O} I{I}", mode, family, dw, db, refs[0])
        out.append(dw.cpu())
        dws = [torch.full((O, I), float("nan"), device=dev) for _ in range(2)]
        dbs = [torch.full((O,), float("nan"), device=dev) for _ in range(2)]
        ws2 = torch.empty(2 * nb, dtype=torch.uint8, device=dev)
        qa = _wgrad_desc(*dev_in[0], dws[0], dbs[0], ws2)
        qb = _wgrad_desc(*dev_in[1], dws[1], dbs[1], None)
        _lib.launch("kpgnn_linear_wgrad_pair", dev, ctypes.byref(qa), ctypes.byref(qb))
        torch.cuda.synchronize()
        for q in range(2):
            _hold_wgrad(f"wgrad_pair[{q}] {family} O{O} I{I}", mode, family, dws[q], dbs[q], refs[q])
            out.append(dws[q].cpu())
        return out

    got = _in_both_modes(run)
    if family == "ones":        # no scratch to look at: the bf16-split route's bits differ from the fp32 instruction's
        for a, f in zip(got["auto"], got["f32"]):
            assert not torch.equal(a, f), "the two modes ran the same arithmetic"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("O,I", C.WGRAD_SHAPES)
@pytest.mark.parametrize("family", C.WGRAD_FAMILIES + ("exact",))
def test_linear_wgrad_group(family, O, I, masked):
    """kpgnn_linear_wgrad_group: three x blocks side by side against one dy, without and with the ReLU mask read on load."""
    from kp_gnn_amd import _lib
    lib, dev, S = _lib.load(), _dev(), C.WGRAD_GROUP
    ref = _wgrad_reference(family, O, S * I, SEED, masked)
    dy, mask, x = ref[0].to(dev), ref[1].to(dev), ref[2]
    xs = [x[:, l * I:(l + 1) * I].contiguous().to(dev) for l in range(S)]
    nb = int(lib.kpgnn_wgrad_group_workspace_bytes(O, I, S))
    name = f"wgrad_group {family} O{O} I{I}{' masked' if masked else ''}"

    def run(mode):
        dw, db = torch.full((O, S * I), float("nan"), device=dev), torch.full((O,), float("nan"), device=dev)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        q = _wgrad_desc(dy, xs[0], dw, db, ws, mask if masked else None)
        ptrs = (ctypes.c_void_p * S)(*[t.data_ptr() for t in xs])
        _lib.launch("kpgnn_linear_wgrad_group", dev, ctypes.byref(q), ptrs, S)
        torch.cuda.synchronize()
        _hold_wgrad(name, mode, family, dw, db, ref)
        return dw.cpu()

    got = _in_both_modes(run)
    if family == "ones":
        assert not torch.equal(got["auto"], got["f32"]), "the two modes ran the same arithmetic"


# ---------------------------------------------------------------------------------------------------------------- edges
EDGE_LIN = (104, 104)          # (I, O)
EDGE_GROUP = (3, 104, 104)     # (S, H, O)


@functools.lru_cache(maxsize=None)
def _edge_reference(kind):
    K, O = (EDGE_LIN[0], EDGE_LIN[1]) if kind == "linear_bn" else (EDGE_GROUP[0] * EDGE_GROUP[1], EDGE_GROUP[2])
    a, b, bias = C.edge_operands(N, O, K, seed=len(kind))
    y64, den = C.ref64(a, b, bias), C.denominator(a, b, bias)
    r32 = max(C.rho(y, y64, den) for y in C.fp32_samples(a, b, bias))
    return a, b, bias, y64, den, r32


def _edge_run(kind, a, b, bias):
    if kind == "linear_bn":
        return _lin_bn(a, b, bias, 0, 0)[0]
    return _group_fwd(a, b, bias, EDGE_GROUP[0], EDGE_GROUP[1])


def _edge_want(kind, y64):
    return y64 if kind == "linear_bn" else torch.relu(y64)


@pytest.mark.parametrize("pa,pb", [(-40, 40), (-20, -20), (30, 20)])
@pytest.mark.parametrize("kind", ["linear_bn", "group_fwd"])
def test_power_of_two_scaling_is_exact(kind, pa, pb, scratch):
    """(2^a x, 2^b W, 2^(a+b) bias) gives 2^(a+b) times the unscaled result, bit for bit: the split commutes with exact scaling
    while no piece is subnormal, and so does fp32 accumulation."""
    a, b, bias, _, _, _ = _edge_reference(kind)

    def run(mode):
        y0 = _edge_run(kind, a, b, bias)
        ys = _edge_run(kind, C.scaled(a, pa), C.scaled(b, pb), C.scaled(bias, pa + pb))
        _route(scratch, mode, kind, launches=2)
        assert torch.equal(ys, C.scaled(y0, pa + pb)), (kind, mode, pa, pb)
    _in_both_modes(run)


@pytest.mark.parametrize("kind", ["linear_bn", "group_fwd"])
def test_subnormal_pieces_keep_the_bound(kind, scratch):
    """x * 2^-110, W * 2^110: every value of x is still a normal fp32 number, its m and l pieces are subnormal bf16 numbers (or
    zero).  The product is the unscaled one; the bound is asserted as for any other input."""
    a, b, bias, y64, den, r32 = _edge_reference(kind)
    sa = C.scaled(a, -110)
    assert bool((sa.abs() >= 2.0 ** -126).all()) and torch.equal(C.scaled(sa, 110), a)
    p = C.split3(sa)
    assert bool(((p["l"] != 0) & (p["l"].abs() < 2.0 ** -126)).any()) and bool(((p["m"] != 0) & (p["m"].abs() < 2.0 ** -126)).any())

    def run(mode):
        y = _edge_run(kind, sa, C.scaled(b, 110), bias)
        _route(scratch, mode, kind)
        _hold(f"{kind} subnormal pieces", mode, y, _edge_want(kind, y64), den, r32)
    _in_both_modes(run)


@pytest.mark.parametrize("kind", ["linear_bn", "group_fwd"])
def test_large_finite_values(kind, scratch):
    """|x| up to 2^126 with |W| <= 2^-20: finite and inside the bound."""
    a, b, bias, y64, den, r32 = _edge_reference(kind)
    la, lb, lbias = C.scaled(a, 124), C.scaled(b, -22), C.scaled(bias, 102)
    assert float(la.abs().max()) == 2.0 ** 126 and float(lb.abs().max()) <= 2.0 ** -20
    s = 2.0 ** 102

    def run(mode):
        y = _edge_run(kind, la, lb, lbias)
        _route(scratch, mode, kind)
        assert bool(torch.isfinite(y).all()), (kind, mode)
        _hold(f"{kind} large finite", mode, y, _edge_want(kind, y64) * s, den * s, r32)
    _in_both_modes(run)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", ["linear_bn", "group_fwd"])
def test_one_bad_row_stays_in_its_row(kind, bad, scratch):
    """Row 40 of x holds +inf / NaN: its outputs are non-finite wherever the float64 reference's are (which non-finite value is
    not asserted), and every other row is bit-identical to the run with row 40 zeroed."""
    a, b, bias, _, _, _ = _edge_reference(kind)
    ab, az = a.clone(), a.clone()
    ab[40] = bad
    az[40] = 0.0
    want = _edge_want(kind, C.ref64(ab[40:41], b, bias))[0]
    assert bool((~torch.isfinite(want)).any())
    others = torch.arange(N) != 40

    def run(mode):
        yb, yz = _edge_run(kind, ab, b, bias), _edge_run(kind, az, b, bias)
        _route(scratch, mode, kind, launches=2)
        assert bool((~torch.isfinite(yb[40]))[~torch.isfinite(want)].all()), (kind, mode, "a non-finite input row came out finite")
        assert torch.equal(yb[others], yz[others]), (kind, mode, "a bad row leaked into another row")
        assert bool(torch.isfinite(yz).all())
    _in_both_modes(run)
