"""GPU: kpgnn_khop_pull_gather (the pull form of the backward gather as an entry of its own) on hand-built CSR tensors.

Every case holds the new entry (a) bit for bit to kpgnn_aggregate_fwd called the way ops.khop_pull_gather called it before
(mode SUM, no tables, per-hop slabs, theta = ones) and (b) to a float64 index_add_ reference, per element within
2 * n * 2^-24 * sum|addends|, n = that element's addend count (pairs + hinit terms): the bound of sequential fp32 summation."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _csr(N, K_csr, seed=0):
    """(source, hop)-keyed CSR by hand: segment lengths 0..5; node 5 has no pairs at all; node 11 has 70 pairs, 40 of them in
    ONE segment (hop 2 where there is one, else hop 0) - the segment crosses the refill of the 32-pair chunk and the node needs
    three chunks.  Returns (rowptr int32 [N*K_csr+1], col int32 [A], seg int64 [A]: the (node * K_csr + hop) of every pair)."""
    g = torch.Generator().manual_seed(1234 + seed)
    lens = torch.randint(0, 6, (N, K_csr), generator=g)
    lens[5] = 0
    big = [3, 5, 40, 5, 5, 4, 4, 4]
    if K_csr >= 8:
        lens[11] = 0
        lens[11, :8] = torch.tensor(big)
    else:
        lens[11] = 0
        lens[11, 0] = 40
        lens[11, K_csr - 1] += 30
    assert int(lens[11].sum()) == 70 and int(lens[5].sum()) == 0
    flat = lens.reshape(-1)
    rowptr = torch.zeros(N * K_csr + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(flat, 0)
    A = int(rowptr[-1])
    col = torch.randint(0, N, (A,), generator=g)
    seg = torch.repeat_interleave(torch.arange(N * K_csr), flat)
    return rowptr.to(torch.int32), col.to(torch.int32), seg


def _inputs(N, K, D, seed, offset=0):
    """K slabs [N,D] (optionally each starting `offset` floats into its allocation) and two addends, on the host."""
    g = torch.Generator().manual_seed(99 + seed)
    slabs = [torch.randn(N, D, generator=g) for _ in range(K)]
    return slabs, torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)


def _place(t, dev, offset):
    """`t` on the device, its first element `offset` floats behind a 256-byte aligned allocation."""
    if not offset:
        return t.to(dev).contiguous()
    buf = torch.empty(t.numel() + offset, dtype=torch.float32, device=dev)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def _reference(rowptr, col, seg, slabs, K, K_csr, N, D, hinit, hinit2, live):
    """float64 sums and, per element, the addend count and the sum of the addends' magnitudes."""
    ref = torch.zeros(N, D, dtype=torch.float64)
    mag = torch.zeros(N, D, dtype=torch.float64)
    cnt = torch.zeros(N, dtype=torch.float64)
    for h in (hinit, hinit2):
        if h is not None:
            ref += h.double()
            mag += h.double().abs()
            cnt += 1
    node, hop = seg // K_csr, seg % K_csr
    for k in range(K):
        m = hop == k
        rows = slabs[k].double()[col[m].long()]
        ref.index_add_(0, node[m], rows)
        mag.index_add_(0, node[m], rows.abs())
        cnt.index_add_(0, node[m], torch.ones(int(m.sum()), dtype=torch.float64))
    return ref[:live], 2.0 * cnt[:live, None] * U * mag[:live]


def _run_both(N, K, K_csr, D, seed=0, addends="both", alias=False, offset=0, live=None):
    """Launches both entries on the same inputs; returns (new, old, reference, bound, sentinel rows of new / old)."""
    from kp_gnn_amd import _lib
    dev = _dev()
    rowptr, col, seg = _csr(N, K_csr)
    slabs, h1, h2 = _inputs(N, K, D, seed)
    hinit = h1 if addends in ("one", "both") else None
    hinit2 = h2 if addends == "both" else None
    live = N if live is None else live
    ref, bound = _reference(rowptr, col, seg, slabs, K, K_csr, N, D, hinit, hinit2, live)
    rp_d, col_d = rowptr.to(dev), col.to(dev)
    code_d = torch.zeros(col.numel(), dtype=torch.int16, device=dev)
    sl_d = [_place(t, dev, offset) for t in slabs]
    n_dyn = torch.tensor([live], dtype=torch.int32, device=dev) if live != N else None
    ones = torch.ones(16, D, dtype=torch.float32, device=dev)
    SENT = -12345.0
    outs = []
    for which in ("new", "old"):
        hi = hinit.to(dev) if hinit is not None else None
        hi2 = hinit2.to(dev) if hinit2 is not None else None
        if alias:
            assert hi is not None and live == N
            out = hi
        else:
            out = torch.full((N, D), SENT, dtype=torch.float32, device=dev)
        if which == "new":
            d = _lib.PullGatherDesc()
            d.N, d.K, d.D, d.K_csr = N, K, D, K_csr
            d.rowptr, d.col, d.slab_sn = rp_d.data_ptr(), col_d.data_ptr(), D
            for k, t in enumerate(sl_d):
                d.slab[k] = t.data_ptr()
            name = "kpgnn_khop_pull_gather"
        else:
            d = _lib.AggFwdDesc()
            d.N, d.K, d.D, d.K_csr, d.mode, d.use_tables = N, K, D, K_csr, _lib.MODE_SUM, 0
            d.rowptr, d.col, d.code, d.x_sn = rp_d.data_ptr(), col_d.data_ptr(), code_d.data_ptr(), D
            for k, t in enumerate(sl_d):
                d.x_slot[k] = t.data_ptr()
            d.theta = ones.data_ptr()
            name = "kpgnn_aggregate_fwd"
        d.n_dyn = n_dyn.data_ptr() if n_dyn is not None else None
        d.hout = out.data_ptr()
        d.hinit = hi.data_ptr() if hi is not None else None
        d.hinit2 = hi2.data_ptr() if hi2 is not None else None
        _lib.launch(name, dev, ctypes.byref(d))
        torch.cuda.synchronize()
        outs.append(out.cpu())
    new, old = outs
    return new, old, ref, bound, SENT


def _check(new, old, ref, bound, live):
    assert torch.equal(new.view(torch.int32), old.view(torch.int32)), \
        f"not bit-identical to kpgnn_aggregate_fwd: max |diff| {float((new - old).abs().max()):.3e}"
    err = (new[:live].double() - ref).abs()
    worst = float((err - bound).max())
    print(f"max err {float(err.max()):.3e}, smallest slack to the bound {-worst:.3e}")
    assert bool((err <= bound).all()), f"float64 reference missed by {worst:.3e} beyond the bound"


def test_odd_node_count_long_node_and_empty_node():
    """N = 37 (no multiple of the 8 nodes of a tile), K = K_csr = 8, D = 104: empty node, 70-pair node with a 40-pair segment."""
    new, old, ref, bound, _ = _run_both(37, 8, 8, 104)
    _check(new, old, ref, bound, 37)
    assert float(bound[5].max()) > 0.0      # node 5 has no pairs: its row is hinit + hinit2 alone
    new0, old0, ref0, bound0, _ = _run_both(37, 8, 8, 104, addends="none")
    _check(new0, old0, ref0, bound0, 37)
    assert float(bound0[5].max()) == 0.0 and bool((new0[5] == 0).all())


@pytest.mark.parametrize("K,K_csr", [(3, 8), (1, 1)])
def test_hop_prefix_and_single_hop(K, K_csr):
    """K = 3 of K_csr = 8 (a layer that reads a prefix of the hops: row-pointer stride K_csr) and K = 1."""
    new, old, ref, bound, _ = _run_both(37, K, K_csr, 104, seed=K)
    _check(new, old, ref, bound, 37)


@pytest.mark.parametrize("D,K,offset", [(96, 8, 0), (128, 8, 0), (64, 8, 0), (100, 8, 2), (64, 16, 0)])
def test_row_widths_and_fallback(D, K, offset):
    """24 of 32 lanes, all 32 lanes, 16-lane sub-groups; D = 100 with the slabs 8 bytes off a 16-byte boundary (8-byte lanes)
    and K = 16 on 16 lanes (row pointers do not fit the sub-group) leave the specialisation for the generic kernel."""
    new, old, ref, bound, _ = _run_both(37, K, K, D, seed=D + K, offset=offset)
    _check(new, old, ref, bound, 37)


@pytest.mark.parametrize("addends,alias", [("none", False), ("one", True), ("both", False), ("both", True)])
def test_addends(addends, alias):
    """No hinit; hinit aliasing hout (what ops.khop_pull_gather does); hinit + hinit2."""
    new, old, ref, bound, _ = _run_both(37, 8, 8, 104, seed=7, addends=addends, alias=alias)
    _check(new, old, ref, bound, 37)


def test_dynamic_rows_leave_dead_rows_alone():
    """Capacity N = 64, live count 37 through n_dyn: rows >= 37 of hout keep the sentinel written before the launch."""
    new, old, ref, bound, sent = _run_both(64, 8, 8, 104, seed=3, live=37)
    _check(new, old, ref, bound, 37)
    assert bool((new[37:] == sent).all()) and bool((old[37:] == sent).all())


def test_malformed_descriptors_are_refused():
    from kp_gnn_amd import _lib
    lib = _lib.load()
    assert lib.kpgnn_khop_pull_gather(None, None) == -1
    d = _lib.PullGatherDesc()
    d.N, d.K, d.D, d.K_csr = 4, 3, 8, 2            # K > K_csr
    assert lib.kpgnn_khop_pull_gather(ctypes.byref(d), None) == -1
    assert b"bad N=" in lib.kpgnn_last_error()
    d.K_csr = 3                                    # NULL rowptr
    assert lib.kpgnn_khop_pull_gather(ctypes.byref(d), None) == -1
