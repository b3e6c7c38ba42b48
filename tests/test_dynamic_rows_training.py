"""GPU (-m gpu): the kernels of the KP-GIN+ training step under a dynamic row count (ops.dynamic_rows(count, capacity)), one
operator at a time, through the wrappers of kp_gnn_amd/ops.py and kp_gnn_amd/ops_dense.py.

Every case builds its inputs for CAP rows and runs forward AND backward inside dynamic_rows(cnt, CAP) with LIVE <= CAP rows live:
  * the floating-point payload of rows >= LIVE of everything handed in (inputs, residuals, upstream gradients, saved state) is
    NaN in one run and 1e30 in a second one; integer inputs of dead rows hold valid, in-range values;
  * torch.empty / torch.empty_like are patched for the duration of the call: float tensors come back NaN-filled, uint8
    workspaces 0xFF-filled - the dead rows of every intermediate and every slab row a block without live rows might skip are
    poisoned as well (statistic slots come from a zeroed arena by contract and are left alone);
  * (a) live rows and reduced outputs are held to a FLOAT64 CPU evaluation of the operator on [:LIVE], with the numbers of the
    operator's exact-shape test (test_gpu_parity.TOL); (b) dead rows of every row-shaped output still hold their poison, bit for
    bit; (c) the two runs agree - bit for bit where the kernels are documented as bitwise repeatable, else within (a)'s bound.

Live counts.  Dense group: {2, 31, 32, 33, 65, CAP - 1, CAP} (32 rows: the tile of lin_fused, lin3f and wgrad2).  For the fused
MLP the smallest count is 5, not 2: two BatchNorms over 2 rows in a row leave the fp32 torch evaluation of the same expression
up to 5.6x the bound away from float64 (the reference alone does not fit: dx 4.3x, weight gradients 4.4x, biases 5.6x); at 5 rows
it is within 1.0x.  One BatchNorm over 2 rows fits (0.7x), so batch_norm_act keeps 2.  Gather group: {33, 257, 261, CAP - 1, CAP}
at CAP = 300 (257 leaves one live node in a tile of 8, 261 five).
Live count 0 is not supported (a StaticBatch cannot produce it) and not tested."""
import contextlib
import functools

import pytest
import torch

import test_gpu_parity as P
from test_fwd_gather_epilogue import N0, NK, _graph, _theta_ref
from test_gpu_parity import TOL, _dev
from test_gpu_parity import _close as _parity_close

pytestmark = pytest.mark.gpu

NAN, BIG = float("nan"), 1e30


def _dense_live(cap, smallest=2):
    return [smallest, 31, 32, 33, 65, cap - 1, cap]


GATHER_CAP = 300
GATHER_LIVE = [33, 257, 261, GATHER_CAP - 1, GATHER_CAP]


# ------------------------------------------------------------------------------------------------------------ harness
def _poisoned(t):
    if t.is_floating_point():
        return t.fill_(NAN)
    if t.dtype == torch.uint8:
        return t.fill_(0xFF)
    return t


@contextlib.contextmanager
def _dynamic(live, cap):
    """dynamic_rows(cnt, cap) with every torch.empty / torch.empty_like of the wrappers poisoned (neither ops.py nor ops_dense.py
    calls Tensor.new_empty)."""
    from kp_gnn_amd import ops
    cnt = torch.tensor([live], dtype=torch.int32, device=_dev())
    real_empty, real_empty_like = torch.empty, torch.empty_like
    mp = pytest.MonkeyPatch()
    with ops.dynamic_rows(cnt, cap):
        mp.setattr(torch, "empty", lambda *a, **kw: _poisoned(real_empty(*a, **kw)))
        mp.setattr(torch, "empty_like", lambda *a, **kw: _poisoned(real_empty_like(*a, **kw)))
        try:
            yield
            torch.cuda.synchronize()
        finally:
            mp.undo()


def _close(op, a, b, name, key=None, tol=None):
    """test_gpu_parity._close with the bound TOL[op][key or name]; prints the largest error over its bound (the room it has)."""
    print(f"RATIO {op} {name} {_parity_close(a, b, name, **(TOL[op][key or name] if tol is None else tol)):.4f}")


def _dead(t, live, value, name):
    """(b): rows >= live of a row-shaped output hold `value`, bit for bit."""
    got = t.detach()[live:].contiguous().cpu().view(torch.int32)
    want = torch.full((1,), value, dtype=torch.float32).view(torch.int32)
    assert bool((got == want).all()), f"{name}: a dead row was written"


def _two_poisons(op, run, bitwise=False):
    """(c): run(poison) -> {name: reduced output or live rows} for both poisons; the two agree."""
    a, b = run(NAN), run(BIG)
    assert sorted(a) == sorted(b)
    for k in a:
        if bitwise:
            assert torch.equal(a[k], b[k]), f"{op} {k}: the result depends on what the dead rows hold"
        else:
            _close(op, a[k], b[k].cpu(), k + " (NaN run vs 1e30 run)", key=k)


# ------------------------------------------------------------------------------------------------ dense: batch_norm_act
@functools.lru_cache(maxsize=None)
def _bn_reference(C, relu, res, live, cap):
    g = torch.Generator().manual_seed(cap + C)
    x, r, w = (torch.randn(cap, C, generator=g) * s + m for s, m in ((2.0, 5.0), (1.0, 0.0), (1.0, 0.0)))
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    bn = torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta)
    xr, rr = x[:live].double().requires_grad_(True), r[:live].double().requires_grad_(True)
    out = bn(xr)
    out = torch.relu(out) if relu else out
    out = out + rr if res else out
    (out * w[:live].double()).sum().backward()
    ref = {"out": out.detach(), "dx": xr.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
           "running_mean": bn.running_mean, "running_var": bn.running_var}
    if res:
        ref["dres"] = rr.grad
    return (x, r, w, gamma, beta), ref


@pytest.mark.parametrize("live", _dense_live(1100))
@pytest.mark.parametrize("slot", [False, True])
@pytest.mark.parametrize("C", [104, 33])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
def test_batch_norm_act(relu, res, C, slot, live):
    """bn.hip: stats (or a slot the producer filled), apply, backward reduce, backward apply."""
    from kp_gnn_amd import ops_dense
    dev, CAP, op = _dev(), 1100, "batch_norm_act"
    (x, r, w, gamma, beta), ref = _bn_reference(C, relu, res, live, CAP)

    def run(poison):
        xs, rs, ws = (t.clone() for t in (x, r, w))
        for t in (xs, rs, ws):
            t[live:] = poison
        bn = torch.nn.BatchNorm1d(C)
        with torch.no_grad():
            bn.weight.copy_(gamma), bn.bias.copy_(beta)
        bn = bn.to(dev).train()
        xd = xs.to(dev).requires_grad_(True)
        rd = rs.to(dev).requires_grad_(True) if res else None
        with _dynamic(live, CAP):
            if slot:      # the producer's column sums of the live rows, spread over the replicas
                s = ops_dense.take_stat_slot(C, dev)
                x64 = x[:live].double()
                sums = torch.stack([torch.stack([x64[q::ops_dense.STAT_REPLICAS].sum(0), (x64[q::ops_dense.STAT_REPLICAS] ** 2).sum(0)])
                                    for q in range(ops_dense.STAT_REPLICAS)])
                s[:sums.numel()].copy_(sums.reshape(-1).to(dev))
                ops_dense.attach_column_stats(xd, s)
                assert ops_dense._column_stats_of(xd) is s
            out = ops_dense.batch_norm_act(xd, bn, relu=relu, residual=rd)
            (out * ws.to(dev)).sum().backward()
        got = {"out": out[:live], "dx": xd.grad[:live], "dgamma": bn.weight.grad, "dbeta": bn.bias.grad,
               "running_mean": bn.running_mean, "running_var": bn.running_var}
        _dead(out, live, NAN, "out")
        _dead(xd.grad, live, NAN, "dx")
        if res:
            got["dres"] = rd.grad[:live]
            _dead(rd.grad, live, poison, "dres")
        for k, v in ref.items():
            _close(op, got[k], v, k)
        assert int(bn.num_batches_tracked) == 1
        return got

    _two_poisons(op, run)


# -------------------------------------------------------------------------------------------------------- dense: linear
@pytest.mark.parametrize("live", _dense_live(1100))
@pytest.mark.parametrize("O,I", [(104, 104), (64, 104)])
def test_linear(O, I, live):
    """ops_dense.linear (LinearWgrad): kpgnn_linear_fwd both ways and kpgnn_linear_wgrad (wgrad2) with its slab finisher."""
    from kp_gnn_amd import ops_dense
    dev, CAP, op = _dev(), 1100, "linear"
    g = torch.Generator().manual_seed(CAP + O)
    x = torch.randn(CAP, I, generator=g)
    wt, b = torch.randn(O, I, generator=g) * 0.1, torch.randn(O, generator=g)
    gy = torch.randn(CAP, O, generator=g) * (1 + torch.arange(O) * 0.01)
    xr, wr, br = x[:live].double().requires_grad_(True), wt.double().requires_grad_(True), b.double().requires_grad_(True)
    yr = torch.nn.functional.linear(xr, wr, br)
    (yr * gy[:live].double()).sum().backward()
    ref = {"y": yr.detach(), "dx": xr.grad, "dW": wr.grad, "db": br.grad}

    def run(poison):
        xs, gs = x.clone(), gy.clone()
        xs[live:] = poison
        gs[live:] = poison
        lin = torch.nn.Linear(I, O)
        with torch.no_grad():
            lin.weight.copy_(wt), lin.bias.copy_(b)
        lin = lin.to(dev)
        xd = xs.to(dev).requires_grad_(True)
        with _dynamic(live, CAP):
            y = ops_dense.linear(xd, lin)
            assert isinstance(y.grad_fn, ops_dense.LinearWgrad._backward_cls)
            (y * gs.to(dev)).sum().backward()
        got = {"y": y[:live], "dx": xd.grad[:live], "dW": lin.weight.grad, "db": lin.bias.grad}
        _dead(y, live, NAN, "y")
        _dead(xd.grad, live, NAN, "dx")
        for k, v in ref.items():
            _close(op, got[k], v, k)
        return got

    _two_poisons(op, run)


# ----------------------------------------------------------------------------------------------------- dense: fused MLP
def _fused_mlp(cap, I, O, follow_norm, live, monkeypatch, bf16_split):
    """test_gpu_parity._fused_mlp_case(live=): the exact-shape test's code, reference and numbers on the live rows.
    bf16_split: which kernels must have run.  kpgnn_linear_bn chooses without a trace and falls back to the fp32 kernels quietly;
    the bf16-split ones first write the split copy of W into the scratch the wrapper hands them, the fp32 ones never touch it -
    and under _dynamic that scratch starts as 0xFF bytes."""
    from kp_gnn_amd import ops_dense
    op = "fused_mlp"
    monkeypatch.setattr(P, "_close", lambda a, b, name, **tol: _close(op, a, b, name, tol=tol))
    scratch, real_split_workspace = [], ops_dense._split_workspace

    def recording_split_workspace(*a):
        ws = real_split_workspace(*a)
        scratch.append(ws)
        return ws
    monkeypatch.setattr(ops_dense, "_split_workspace", recording_split_workspace)

    def run(poison):
        del scratch[:]
        got = P._fused_mlp_case(cap, I, O, follow_norm, live=live, poison=poison, scope=lambda: _dynamic(live, cap))
        assert len(scratch) == 4 and all(ws is not None for ws in scratch), "two Linear+BatchNorm launches per direction"
        written = [bool((ws != 0xFF).any()) for ws in scratch]
        assert all(written) if bf16_split else not any(written), (written, "the other kernel family ran")
        _dead(got["out"], live, NAN, "out")
        _dead(got["dx"], live, NAN, "dx")
        if "dres_rows" in got:     # dz itself, or the parked share the kernel added dz's live rows to
            _dead(got["dres_rows"], live, poison, "dres")
        return got

    a, b = run(NAN), run(BIG)
    T = TOL[op]
    for k in ("out", "dx", "dres"):
        if k in a:
            _close(op, a[k][:live], b[k][:live].cpu(), k + " (NaN run vs 1e30 run)", key=k)
    for k, v in a["reduced"].items():
        if "num_batches" in k:
            assert int(v) == int(b["reduced"][k]) == (1 if (follow_norm or not k.startswith("norm.")) else 0), k
        elif "running" in k:
            _close(op, v, b["reduced"][k].cpu(), k + " (NaN run vs 1e30 run)", key="running")
    # the parameter gradients of the two runs, each held to the float64 reference above, against each other by the same rule
    grads = {k: v for k, v in a["reduced"].items() if k.startswith("grad ") and k in a["ref_grads"]}

    class _G:
        def __init__(self, g):
            self.grad = g
    P._close_param_grads({k: _G(v) for k, v in grads.items()}, {k: b["reduced"][k] for k in grads}, "NaN run vs 1e30 run",
                         *T["param_grads"])


@pytest.mark.parametrize("live", _dense_live(1100, smallest=5))
@pytest.mark.parametrize("I,O", [(104, 104), (64, 104), (32, 32)])
@pytest.mark.parametrize("follow_norm", [False, True, "fused", "fused_cell"])
def test_fused_mlp_fp32_kernels(follow_norm, I, O, live, monkeypatch):
    """lin_fused_*, lin_fused_bwd*, the paired wgrad: a capacity below 4096 keeps the fp32 kernels."""
    _fused_mlp(1100, I, O, follow_norm, live, monkeypatch, bf16_split=False)


@pytest.mark.parametrize("live", _dense_live(4200, smallest=5) + [4095, 4096, 4097])
@pytest.mark.parametrize("I,O", [(104, 104), (64, 104), (32, 32)])
@pytest.mark.parametrize("follow_norm", [False, True, "fused", "fused_cell"])
def test_fused_mlp_bf16_split_kernels(follow_norm, I, O, live, monkeypatch):
    """linear_bf3_fused (lin3f_kernel: grid sized for the capacity): the CAPACITY of 4200 picks the bf16-split kernels, however
    few rows are live."""
    _fused_mlp(4200, I, O, follow_norm, live, monkeypatch, bf16_split=True)


@pytest.mark.parametrize("live", [33, 16385])
@pytest.mark.parametrize("follow_norm", [False, True, "fused", "fused_cell"])
def test_fused_mlp_tile_height_2_from_the_capacity(follow_norm, live, monkeypatch):
    """set_dense_math("f32") at a capacity of 16500: lin_fused_kernel's tile height m = 2 is chosen from the capacity."""
    from kp_gnn_amd import ops_dense
    ops_dense.set_dense_math("f32")
    try:
        _fused_mlp(16500, 64, 104, follow_norm, live, monkeypatch, bf16_split=False)
    finally:
        ops_dense.set_dense_math("auto")


# ---------------------------------------------------------------------------------------------- dense: JK concat projection
@pytest.mark.parametrize("live_of", range(7))
@pytest.mark.parametrize("H,S,O", [(104, 9, 104), (32, 5, 64)])
@pytest.mark.parametrize("CAP", [1100, 4200])
def test_jk_concat_projection(CAP, H, S, O, live_of):
    """ops_dense.JKConcatLinear: linear_group (CAP = 1100) / linear_bf3 (CAP = 4200), kpgnn_linear_fwd with the ReLU mask read
    on load, the grouped wgrad.  As in the exact-shape test the reference applies the mask the GPU forward produced."""
    from kp_gnn_amd.ops_dense import JKConcatLinear, _jk_native_ok
    dev, op = _dev(), "jk_projection"
    live = _dense_live(CAP)[live_of]
    g = torch.Generator().manual_seed(CAP + S)
    states = [torch.randn(CAP, H, generator=g) * (1 + 0.1 * l) for l in range(S)]
    w = torch.randn(O, S * H, generator=g) * 0.05
    b = torch.randn(O, generator=g) * 0.1
    gy = torch.randn(CAP, O, generator=g) * (1 + torch.arange(O) * 0.01)
    sr = [t[:live].double().requires_grad_(True) for t in states]
    wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = torch.nn.functional.linear(torch.cat(sr, dim=1), wr, br)

    def run(poison):
        ss, gs = [t.clone() for t in states], gy.clone()
        for t in ss + [gs]:
            t[live:] = poison
        sd = [t.to(dev).requires_grad_(True) for t in ss]
        wd, bd = w.clone().to(dev).requires_grad_(True), b.clone().to(dev).requires_grad_(True)
        assert _jk_native_ok(wd, bd, sd)
        with _dynamic(live, CAP):
            y = JKConcatLinear.apply(wd, bd, *sd)
            (y * gs.to(dev)).sum().backward()
        _dead(y, live, NAN, "y")
        _close(op, y[:live], torch.relu(pre.detach()), "y")
        for t in [wr, br] + sr:
            t.grad = None
        mask = (y.detach()[:live].cpu() > 0).double()
        ((pre * mask) * gy[:live].double()).sum().backward(retain_graph=True)
        got = {"y": y[:live], "dW": wd.grad, "db": bd.grad}
        _close(op, wd.grad, wr.grad, "dW")
        _close(op, bd.grad, br.grad, "db")
        for l in range(S):
            _dead(sd[l].grad, live, NAN, f"dstate{l}")
            _close(op, sd[l].grad[:live], sr[l].grad, f"dstate{l}", key="dstate")
            got[f"dstate {l}"] = sd[l].grad[:live]
        return got

    a, b2 = run(NAN), run(BIG)
    for k in a:
        _close(op, a[k], b2[k].cpu(), k + " (NaN run vs 1e30 run)", key=k.split(" ")[0])


# --------------------------------------------------------------------------------------------------- dense: segment_pool
@pytest.mark.parametrize("live,ptr_end", [pytest.param(n, e, id=str(n) if e == "live" else f"{n}-{e}")
                                          for e in ("live", "capacity") for n in _dense_live(1100)])
@pytest.mark.parametrize("D", [104, 13])
@pytest.mark.parametrize("mean", [False, True])
def test_segment_pool(mean, D, live, ptr_end):
    """pool.hip, forward + backward; the dead rows of `batch` repeat a valid graph id.  graph_ptr ends at the live count (as
    dataset.StaticBatch attaches it) or at the capacity (what ops.graph_ptr_of makes of this `batch`): the kernels clamp it to
    the live count themselves, so neither the last graph's sum nor its mean divisor may see a dead row."""
    from kp_gnn_amd import ops
    dev, CAP, G, op = _dev(), 1100, 40, "segment_pool"
    g = torch.Generator().manual_seed(D + live)
    cut = torch.sort(torch.randint(0, live + 1, (G - 1,), generator=g)).values          # (empty graphs where cuts coincide)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long), cut, torch.tensor([live])])
    sizes = ptr[1:] - ptr[:-1]
    batch_live = torch.repeat_interleave(torch.arange(G), sizes)
    batch = torch.cat([batch_live, torch.full((CAP - live,), G - 1, dtype=torch.long)])
    x = torch.randn(CAP, D, generator=g)
    w = torch.randn(G, D, generator=g)
    xr = x[:live].double().requires_grad_(True)
    pr = torch.zeros(G, D, dtype=torch.float64).index_add_(0, batch_live, xr)
    if mean:
        pr = pr / sizes.clamp(min=1).unsqueeze(-1)
    (pr * w.double()).sum().backward()
    ptr_dev = ptr.to(torch.int32).to(dev)
    if ptr_end == "capacity":
        ptr_dev[G] = CAP
        assert torch.equal(ops.graph_ptr_of(batch.to(dev), G), ptr_dev)

    def run(poison):
        xs = x.clone()
        xs[live:] = poison
        xd, bd = xs.to(dev).requires_grad_(True), batch.to(dev)
        setattr(bd, ops._GPTR, ((bd._version, G), ptr_dev))
        with _dynamic(live, CAP):
            out = ops.segment_pool(xd, bd, G, mean=mean)
            (out * w.to(dev)).sum().backward()
        _dead(xd.grad, live, NAN, "pool grad")
        got = {"pool": out.detach(), "pool grad": xd.grad[:live]}
        _close(op, got["pool"], pr.detach(), "pool")
        _close(op, got["pool grad"], xr.grad, "pool grad")
        return got

    _two_poisons(op, run, bitwise=True)


# ----------------------------------------------------------------------------------- dense: table_gather_sum / embedding_rows
@pytest.mark.parametrize("live", _dense_live(777))
@pytest.mark.parametrize("D", [104, 13])
@pytest.mark.parametrize("entry", ["table_gather_sum", "embedding_rows"])
def test_table_gather(entry, D, live):
    """table_gather.hip, forward + table gradient, no bias (its gradient is refused): M = CAP = 777 index rows; the dead rows
    hold other valid indices."""
    from kp_gnn_amd import ops
    dev, CAP, op = _dev(), 777, "table_gather_sum"
    g = torch.Generator().manual_seed(D)
    R_sizes = [5, 51] + [51] * 7
    if entry == "table_gather_sum":
        tab_of_col = [0, 1] + list(range(len(R_sizes)))
        starts = torch.tensor([0] + R_sizes).cumsum(0)
        idx = torch.stack([torch.randint(0, R_sizes[t], (CAP,), generator=g) for t in tab_of_col], 1)
        off = torch.stack([starts[t] for t in tab_of_col])
        table = torch.randn(int(starts[-1]), D, generator=g)
    else:
        idx = torch.randint(0, 51, (CAP,), generator=g)
        off = torch.zeros(1, dtype=torch.long)
        table = torch.randn(51, D, generator=g)
    w = torch.randn(CAP, D, generator=g)
    tr = table.double().requires_grad_(True)
    flat = (idx.view(CAP, -1) + off)[:live]
    ref_out = tr[flat.reshape(-1)].view(live, -1, D).sum(1)
    (ref_out * w[:live].double()).sum().backward()

    def run(poison):
        ws = w.clone()
        ws[live:] = poison
        td = table.clone().to(dev).requires_grad_(True)
        with _dynamic(live, CAP):
            if entry == "table_gather_sum":
                out = ops.table_gather_sum(td, None, idx.to(torch.int16).to(dev), off.to(torch.int32).to(dev))
            else:
                out = ops.embedding_rows(td, idx.to(dev))
            (out * ws.to(dev)).sum().backward()
        _dead(out, live, NAN, "out")
        got = {"out": out[:live], "gtable": td.grad}
        _close(op, got["out"], ref_out.detach(), "out")
        _close(op, got["gtable"], tr.grad, "gtable")
        return got

    _two_poisons(op, run, bitwise=True)


# ----------------------------------------------------------------------------------------------------------- gather side
@functools.lru_cache(maxsize=None)
def _capacity_csr(live, K=8):
    """The CSR of GATHER_CAP nodes whose pairs all lie among the first `live` (what a refilled StaticBatch holds), and the
    (node, hop, other end, code) of every pair read back from it, by destination and by source."""
    from kp_gnn_amd.khop_csr import KHopCSR
    ei, ea = _graph(GATHER_CAP, K, seed=1000 + live, n_live=live)
    csr = KHopCSR.build(ei.to(_dev()), ea.to(_dev()), GATHER_CAP)
    assert any(l % csr.nodes_per_tile for l in GATHER_LIVE), "no tile mixes live and dead nodes"

    def pairs(rowptr, col, code):
        rp, col, code = rowptr.cpu().long().view(-1), col.cpu().long(), code.cpu().long() & 0xFFFF
        n_seg = live * csr.K
        assert int(rp[n_seg]) == int(rp[-1]) == csr.A, "a dead node has pairs"
        seg = torch.repeat_interleave(torch.arange(n_seg), rp[1:n_seg + 1] - rp[:n_seg])
        p = torch.arange(int(rp[0]), int(rp[n_seg]))
        assert int(col[p].max()) < live
        return seg // csr.K, seg % csr.K, col[p], code[p]

    return csr, pairs(csr.rowptr_dst, csr.col_dst, csr.code_dst), pairs(csr.rowptr_src, csr.col_src, csr.code_src)


def _table_ref(pairs, g64, k_act):
    """float64 edge-code table gradients: index_add_ of dL/dS[dst, hop] over the live nodes' pairs"""
    node, hop, _, code = pairs
    keep = hop < k_act
    node, hop, code = node[keep], hop[keep], code[keep]
    rows = g64[node, hop]
    D = g64.shape[2]
    return (torch.zeros(N0, D, dtype=torch.float64).index_add_(0, code[hop == 0], rows[hop == 0]),
            torch.zeros(NK, D, dtype=torch.float64).index_add_(0, code[hop > 0], rows[hop > 0]))


def _uid_matrix(gen, live, U, K=8):
    """[GATHER_CAP, K] ids: skewed over [0, U) in the live rows, other valid ids in the dead ones"""
    uid = ((torch.rand(GATHER_CAP, K, generator=gen) ** 3) * U).to(torch.int32)
    uid[live:] = (U - 1 - uid[live:])
    return uid


@pytest.mark.parametrize("live", GATHER_LIVE)
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("mode", ["gin", "ginplus"])
def test_aggregate_bwd(mode, accum, live):
    """ops.aggregate_bwd_raw (agg_bwd_kernel, K = 8, D = 104): a fresh gx and gx added into a state's gradient cell; gin with a
    fresh gx also takes the code-table gradients in the gather (the kernel has no accumulating form with table gradients)."""
    from kp_gnn_amd import ops
    dev, CAP, K, D, op = _dev(), GATHER_CAP, 8, 104, "aggregate"
    csr, _, (src, hop, dst, code) = _capacity_csr(live)
    gen = torch.Generator().manual_seed(live + len(mode))
    g = torch.randn(CAP, K, D, generator=gen)
    old = torch.randn(CAP, K * D, generator=gen)
    eps = torch.tensor([0.3])
    g64 = g[:live].double()
    ref = torch.zeros(live * K, D, dtype=torch.float64).index_add_(0, src * K + hop, g64[dst, hop]).view(live, K, D)
    tables = mode == "gin" and not accum
    if mode == "gin":
        ref = ref + (1.0 + eps.double()) * g64
        ref0, refk = _table_ref((dst, hop, src, code), g64, K)
    if accum:
        ref = ref + old[:live].double().view(live, K, D)

    def run(poison):
        gs, olds = g.clone(), old.clone()
        gs[live:] = poison
        olds[live:] = poison
        cell = olds.to(dev) if accum else None
        with _dynamic(live, CAP):
            gx, gt0, gtk = ops.aggregate_bwd_raw(csr, K, ops.MODE_GIN if mode == "gin" else ops.MODE_GINPLUS, gs.to(dev),
                                                 eps.to(dev) if mode == "gin" else None, N0, NK, tables, gx_accum=cell)
        _dead(gx, live, poison if accum else NAN, "gx")
        got = {"grad_x": gx[:live]}
        _close(op, got["grad_x"], ref, "grad_x")
        if tables:
            got.update(grad_table0=gt0, grad_tablek=gtk)
            _close(op, gt0, ref0, "grad_table0")
            _close(op, gtk, refk, "grad_tablek")
        return got

    _two_poisons(op, run)


@pytest.mark.parametrize("live", GATHER_LIVE)
@pytest.mark.parametrize("D", [104, 13])
@pytest.mark.parametrize("dict_mode", ["theta_gh", "rows", "none"])
@pytest.mark.parametrize("kernel", ["walk", "mfma"])
def test_table_grad(kernel, dict_mode, D, live):
    """ops.table_grad_raw, both kernels: edge-code tables and both dictionary sources.  The walk takes every entry of the uid-sorted
    list of ops.dict_tile_pack and loads only the live rows of a tile: with the list built over the capacity, "rows" added what an
    earlier tile had left in LDS for the dead nodes of the tile that mixes live and dead ones."""
    from kp_gnn_amd import ops
    dev, CAP, K, U, op = _dev(), GATHER_CAP, 8, 19, "table_grad"
    csr, by_dst, _ = _capacity_csr(live)
    gen = torch.Generator().manual_seed(D * 7 + live)
    g = torch.randn(CAP, K, D, generator=gen)
    gh = torch.randn(CAP, D, generator=gen)
    theta = torch.rand(K, D, generator=gen)
    uid = _uid_matrix(gen, live, U)
    g64 = g[:live].double()
    ref0, refk = _table_ref(by_dst, g64, K)
    if dict_mode != "none":
        srcd = (theta.double().unsqueeze(0) * gh[:live].double().unsqueeze(1)) if dict_mode == "theta_gh" else g64
        refd = torch.zeros(U, D, dtype=torch.float64).index_add_(0, uid[:live].reshape(-1).long(), srcd.reshape(-1, D))

    def run(poison):
        gs, ghs = g.clone(), gh.clone()
        gs[live:] = poison
        ghs[live:] = poison
        kw = {}
        if dict_mode == "theta_gh":
            kw = dict(uid=uid.to(dev), n_dict=U, theta=theta.to(dev), gh=ghs.to(dev))
        elif dict_mode == "rows":
            kw = dict(uid=uid.to(dev), n_dict=U)
        with _dynamic(live, CAP):
            res = ops.table_grad_raw(csr, gs.to(dev), N0, NK, edges=True, kernel={"walk": 1, "mfma": 2}[kernel], **kw)
        assert res is not None
        got = {"gtable0": res[0], "gtablek": res[1]}
        _close(op, res[0], ref0, "gtable0")
        _close(op, res[1], refk, "gtablek")
        if dict_mode != "none":
            got["gdict"] = res[2]
            _close(op, res[2], refd, "gdict")
        return got

    _two_poisons(op, run, bitwise=True)


def test_dictionary_list_of_a_dynamic_launch_is_not_walked_by_a_static_one():
    """The uid-sorted list built under dynamic_rows holds live nodes only and is kept on the csr: a later launch over ALL rows of
    the same csr and uid (no dynamic_rows) builds and walks its own, complete list."""
    from kp_gnn_amd import ops
    dev, CAP, live, K, D, U = _dev(), GATHER_CAP, 257, 8, 104, 19
    csr, by_dst, _ = _capacity_csr(live)
    gen = torch.Generator().manual_seed(11)
    g = torch.randn(CAP, K, D, generator=gen)
    uid = _uid_matrix(gen, live, U).to(dev)
    gd = g.to(dev)
    with _dynamic(live, CAP):
        first = ops.table_grad_raw(csr, gd, N0, NK, edges=True, kernel=1, uid=uid, n_dict=U)
    res = ops.table_grad_raw(csr, gd, N0, NK, edges=True, kernel=1, uid=uid, n_dict=U)
    refd = lambda n: torch.zeros(U, D, dtype=torch.float64).index_add_(0, uid[:n].cpu().reshape(-1).long(), g[:n].double().reshape(-1, D))
    _close("table_grad", first[2], refd(live), "gdict")
    _close("table_grad", res[2], refd(CAP), "gdict")


@pytest.mark.parametrize("live", GATHER_LIVE)
@pytest.mark.parametrize("k_act,D,U", [(8, 104, 11), (1, 64, 3)])
@pytest.mark.parametrize("form", ["plain", "designated", "multi"])
def test_dict_grad(form, k_act, D, U, live):
    """ops.dict_grad_raw without and with a designated id per hop (_kp_dom), and ops.dict_grad_multi_raw over three layers that
    read hop prefixes of one id matrix."""
    from kp_gnn_amd import ops
    dev, CAP, op = _dev(), GATHER_CAP, "dict_grad"
    gen = torch.Generator().manual_seed(live + k_act)
    uid_full = _uid_matrix(gen, live, U)
    ks = [k_act, max(1, k_act - 3), max(1, k_act - 5)] if form == "multi" else [k_act]
    thetas = [torch.rand(k, D, generator=gen) for k in ks]
    ghs = [torch.randn(CAP, D, generator=gen) for _ in ks]
    ref = torch.zeros(U, D, dtype=torch.float64)
    for k, th, gh in zip(ks, thetas, ghs):
        ref.index_add_(0, uid_full[:live, :k].reshape(-1).long(),
                       (th.double().unsqueeze(0) * gh[:live].double().unsqueeze(1)).reshape(-1, D))

    def run(poison):
        ud = uid_full.to(dev)
        gd = []
        for gh in ghs:
            t = gh.clone()
            t[live:] = poison
            gd.append(t.to(dev))
        views = [ud[:, :k] for k in ks]
        if form != "plain":
            views[0]._kp_dom = torch.mode(uid_full[:live, :k_act], dim=0).values.to(torch.int32).to(dev).contiguous()
        with _dynamic(live, CAP):
            if form == "multi":
                assert all(ops.dict_multi_ok(v, U, th.to(dev), t) for v, th, t in zip(views[:1], thetas, gd))
                out = ops.dict_grad_multi_raw([(v, th.to(dev), t) for v, th, t in zip(views, thetas, gd)], U)
            else:
                out = ops.dict_grad_raw(views[0], U, thetas[0].to(dev), gd[0])
        assert out is not None
        _close(op, out, ref, "gdict")
        return {"gdict": out}

    _two_poisons(op, run, bitwise=True)


@pytest.mark.parametrize("live", GATHER_LIVE)
@pytest.mark.parametrize("k_act,in_walk", [(8, False), (8, True), (3, False), (1, False)])
def test_combine_table_grad(k_act, in_walk, live):
    """ops.combine_table_grad_raw (kpgnn_table_grad with the combine backward fused in), want_gtheta with alphas: the
    matrix-core kernel (8, no dictionary rows), dictionary rows in the walk (the dict_tile_pack path: the walk does not compare an
    entry's node with the live count, the list has to hold live nodes only) and super-tiles (k = 3, 1).
    float64: g = theta[k] gh[i] gelu'(S[i,k]); gtheta[k] = sum_i gh[i] (gelu(S[i,k]) + P[uid[i,k]]); d/dalphas through
    theta = softmax_k(a (1 - a)^k); tables and dictionary rows by index_add_ over the live nodes."""
    from kp_gnn_amd import ops
    dev, CAP, D, U, op = _dev(), GATHER_CAP, 104, 13, "combine_table_grad"
    csr, by_dst, _ = _capacity_csr(live)
    gen = torch.Generator().manual_seed(live + 7 * k_act)
    pre = torch.randn(CAP, k_act, D, generator=gen)
    gh = torch.randn(CAP, D, generator=gen)
    alphas = torch.randn(D, generator=gen)
    ptab = torch.randn(U, D, generator=gen)
    uid_full = _uid_matrix(gen, live, U)
    uid = uid_full[:, :k_act]
    theta = _theta_ref(alphas, k_act).float()
    S = pre[:live].double().requires_grad_(True)
    th64 = theta.double().requires_grad_(True)
    hout = ((torch.nn.functional.gelu(S) + ptab.double()[uid[:live].long()]) * th64.unsqueeze(0)).sum(1)
    (hout * gh[:live].double()).sum().backward()
    al = alphas.double().requires_grad_(True)
    (_theta_ref(al, k_act) * th64.grad).sum().backward()
    ref0, refk = _table_ref(by_dst, S.grad, k_act)
    ref = {"g": S.grad, "gtheta": th64.grad, "galphas": al.grad, "gtable0": ref0}
    if k_act > 1:
        ref["gtablek"] = refk
    if in_walk:
        ref["gdict"] = torch.zeros(U, D, dtype=torch.float64).index_add_(
            0, uid[:live].reshape(-1).long(), (theta.double().unsqueeze(0) * gh[:live].double().unsqueeze(1)).reshape(-1, D))

    def run(poison):
        ps, ghs = pre.clone(), gh.clone()
        ps[live:] = poison
        ghs[live:] = poison
        ud = uid_full.to(dev)[:, :k_act]           # (a hop-prefix view of the [N,8] id matrix, as the layers pass it)
        with _dynamic(live, CAP):
            r = ops.combine_table_grad_raw(csr, ps.to(dev), ghs.to(dev), theta.to(dev), ptab.to(dev), ud, N0, NK, want_gtheta=True,
                                           alphas=alphas.to(dev), dict_rows=U if in_walk else 0)
        assert r is not None
        if not in_walk:
            assert 1 <= csr.max_multiplicity() < 64
        _dead(r[0], live, NAN, "g")
        got = {"g": r[0][:live], "gtheta": r[1][0], "galphas": r[1][1], "gtable0": r[2]}
        if k_act > 1:
            got["gtablek"] = r[3]
        if in_walk:
            got["gdict"] = r[4]
        for k, v in ref.items():
            _close(op, got[k], v, k)
        return got

    _two_poisons(op, run, bitwise=True)


# -------------------------------------------------------------------------------------------------------------- refusals
def _refusal_sites():
    """name -> (rows, call): `call()` runs one operator that has no n_dyn on `rows` rows (forward and, where the refusal sits
    there, backward)."""
    from kp_gnn_amd import ops, ops_dense
    from kp_gnn_amd.khop_csr import KHopCSR
    dev = _dev()
    gen = torch.Generator().manual_seed(3)
    R = lambda *s: torch.randn(*s, generator=gen).to(dev)

    def combine_bwd():
        N, K, D = 64, 3, 24
        ops.combine_bwd_raw(ops.MODE_GINPLUS, R(N, K, D), R(N, D), torch.rand(K, D, generator=gen).to(dev), None, None, None,
                            want_gtheta=False, want_gv=False)

    def eps_gradient():
        N, K, D = 61, 5, 16
        ei, ea = P._random_khop(N, 700, K, seed=5)
        csr = KHopCSR.build(ei.to(dev), ea.to(dev), N)
        eps = torch.tensor([0.3], device=dev, requires_grad=True)
        out = ops.khop_aggregate(R(N, K, D).requires_grad_(True), csr, K, ops.MODE_GIN, table0=R(5, D), tablek=R(12, D),
                                 periph=R(N, K, D), eps=eps)
        out.sum().backward()

    def gather_bias():
        table, bias = R(56, 16).requires_grad_(True), R(16).requires_grad_(True)
        idx = torch.randint(0, 5, (40, 2), generator=gen).to(torch.int16).to(dev)
        ops.table_gather_sum(table, bias, idx, torch.tensor([0, 5], dtype=torch.int32, device=dev)).sum().backward()

    def wide_pool():
        ops.segment_pool(R(50, 300), torch.arange(50, device=dev) // 10, 5)

    def linear_few_rows():
        ops_dense.linear(R(500, 104), torch.nn.Linear(104, 104).to(dev))

    def linear_width():
        ops_dense.linear(R(1100, 40), torch.nn.Linear(40, 40).to(dev))

    def linear_wgrad_unaligned():      # (forward on kpgnn_linear_fwd; O = 132 > 128 is outside wgrad2: kpgnn_linear_wgrad's own check)
        ops_dense.linear(R(1100, 32), torch.nn.Linear(32, 132).to(dev)).sum().backward()

    def batch_norm_wide():
        ops_dense.batch_norm_act(R(40, 300), torch.nn.BatchNorm1d(300).to(dev).train())

    def jk_width():
        w = R(64, 3 * 40).requires_grad_(True)
        ops_dense.JKConcatLinear.apply(w, None, *[R(70, 40) for _ in range(3)])

    def hop_mlp():
        N, K, DI = 77, 6, 20
        ops_dense.hop_mlp(R(N, K, DI), R(K, DI, DI), R(K, DI), R(K, DI, DI), R(K, DI))

    # (rows, call, the words of the site's own message)
    return {"combine_bwd_raw": (64, combine_bwd, "kpgnn_combine_bwd has no dynamic row count"),
            "eps gradient": (61, eps_gradient, "the eps gradient"),
            "table_gather_sum bias": (40, gather_bias, "the bias gradient of a table gather-sum"),
            "segment_pool wider than 256": (50, wide_pool, "graph readout of rows wider than 256"),
            "linear below 1024 rows": (500, linear_few_rows, "nn.Linear on the framework path"),
            "linear width": (1100, linear_width, "nn.Linear outside the MFMA kernels' shapes"),
            "kpgnn_linear_wgrad unaligned": (1100, linear_wgrad_unaligned, "linear_wgrad: dy_mask / n_dyn need"),
            "batch_norm_act wider than 256": (40, batch_norm_wide, "BatchNorm on the framework path"),
            "JK projection width": (70, jk_width, "the jumping-knowledge projection outside the grouped-K kernels' shapes"),
            "hop_mlp": (77, hop_mlp, "kpgnn_hop_mlp has no dynamic row count")}


@pytest.mark.parametrize("site", ["combine_bwd_raw", "eps gradient", "table_gather_sum bias", "segment_pool wider than 256",
                                  "linear below 1024 rows", "linear width", "kpgnn_linear_wgrad unaligned",
                                  "batch_norm_act wider than 256", "JK projection width", "hop_mlp"])
def test_operators_without_n_dyn_refuse_the_capacity(site):
    """Each operator without a dynamic row count raises under dynamic_rows when its row count IS the capacity - with the message
    of the site the case names, not another check's on the way there - and the same call runs when the capacity is another
    number: the refusal keys on the capacity and on nothing else."""
    import re
    from kp_gnn_amd import _lib, ops
    rows, call, words = _refusal_sites()[site]
    cnt = torch.tensor([rows - 1], dtype=torch.int32, device=_dev())
    with ops.dynamic_rows(cnt, rows):
        with pytest.raises(_lib.KpgnnError, match=re.escape(words)):
            call()
    with ops.dynamic_rows(cnt, rows + 1):
        call()
    torch.cuda.synchronize()
