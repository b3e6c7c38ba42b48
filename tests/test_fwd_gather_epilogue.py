"""GPU (-m gpu): the forward K-hop gather's KP-GIN+ training epilogue (agg_fwd_kernel, FAST instantiations) through
ops.aggregate_fwd_raw: per-hop inputs, code tables, dictionary P, S saved, geometric combine from alphas or a given theta.

The kernel requests a hop's dictionary row one hop ahead, parks it in LDS and stores a hop's S row one hop late, so the cases
are the ones where that bookkeeping can go wrong: a node with more pairs in one hop than two chunks of its sub-group, empty
middle hops, an isolated node, a node whose pairs all lie in the last hop, K = 1, K >= G (the generic instantiation), dead
rows of a static-shape launch, bf16 rows.  N = 4100 is the smallest exact-shape batch the library does not hand to
agg_fwd_small_kernel (N <= 4096) and leaves a ragged last tile.

Reference: S, gelu(S) + P[uid] and the theta-weighted hop sum in float64 on the CPU from the same CSR (index_add_ in
edge-list order), compared with test_gpu_parity._close - the bound that file holds fp32 aggregates to."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_parity import BF16_RTOL, _close, _dev, _rel_close

pytestmark = pytest.mark.gpu

N_BIG = 4100
N0, NK = 5, 52          # rows of the two code tables (the ZINC line: 3 + 2 and 50 + 2)
HEAVY, GAPPY, ALONE, LATE = 1, 2, 3, 5     # the special nodes of every graph


def _graph(N, K, seed, n_live=None):
    """edge_index [2,E], edge_attr [E,K] (0 = pair absent): random pairs among the live nodes plus
    HEAVY: 70 pairs in ONE hop (more than two chunks of G = 32); GAPPY: pairs in the first and the last hop only;
    ALONE: no pair at all; LATE: pairs in the last hop only."""
    n_live = N if n_live is None else n_live
    rng = np.random.default_rng(seed)
    E = 6 * n_live
    special = np.array([HEAVY, GAPPY, ALONE, LATE])
    dst = rng.integers(0, n_live, size=E)
    dst = np.where(np.isin(dst, special), (dst + 7) % n_live, dst)      # (1, 2, 3, 5 -> 8, 9, 10, 12: none of them special)
    src = rng.integers(0, n_live, size=E)
    ea = np.zeros((E, K), dtype=np.int64)
    act = rng.random((E, K)) < 0.3
    ea[:, 0] = rng.integers(2, N0, size=E) * act[:, 0]
    if K > 1:
        ea[:, 1:] = rng.integers(2, NK, size=(E, K - 1)) * act[:, 1:]
    last, mid = K - 1, min(2, K - 1)

    def extra(node, n, hops):
        e = np.zeros((n, K), dtype=np.int64)
        for h in hops:
            e[:, h] = rng.integers(2, N0 if h == 0 else NK, size=n)
        return rng.integers(0, n_live, size=n), np.full(n, node), e

    parts = [extra(HEAVY, 70, [mid]), extra(GAPPY, 9, sorted({0, last})), extra(LATE, 6, [last])]
    src = np.concatenate([src] + [p[0] for p in parts])
    dst = np.concatenate([dst] + [p[1] for p in parts])
    ea = np.concatenate([ea] + [p[2] for p in parts])
    return torch.from_numpy(np.stack([src, dst])), torch.from_numpy(ea)


def _uid(N, K, n_dict):
    """even nodes: one id at every hop; odd nodes: another id at every hop (all K distinct when n_dict >= K)"""
    i = torch.arange(N).unsqueeze(1)
    k = torch.arange(K).unsqueeze(0)
    return torch.where(i % 2 == 0, (i % n_dict).expand(N, K), (i + k) % n_dict).to(torch.int32).contiguous()


def _theta_ref(alphas, K):
    """softmax_k(a (1 - a)^k), a = sigmoid(alphas) (the geometric combine), float64"""
    a = torch.sigmoid(alphas.double())
    return torch.softmax(torch.stack([a * (1 - a) ** k for k in range(K)]), 0)


def _reference(csr, K, xs, t0, tk, ptab, uid, theta, n_rows):
    """float64: S [n_rows,K,D] and hout [n_rows,D] from the CSR the kernel reads"""
    D = xs[0].shape[1]
    rp = csr.rowptr_dst.cpu().long()
    col = csr.col_dst.cpu().long()
    code = csr.code_dst.cpu().long()
    n_seg = n_rows * csr.K                                      # segments (node, hop) of the rows asked for, in CSR order
    seg = torch.repeat_interleave(torch.arange(n_seg), rp[1:n_seg + 1] - rp[:n_seg])
    pairs = torch.arange(int(rp[0]), int(rp[n_seg]))
    node, hop = seg // csr.K, seg % csr.K
    keep = hop < K
    node, hop, pairs = node[keep], hop[keep], pairs[keep]
    tabs = torch.cat([t0, tk]).double()                         # hop 0 reads table0, later hops tablek
    vals = torch.stack(xs).double()[hop, col[pairs]] + tabs[code[pairs] + (hop > 0) * t0.shape[0]]
    S = torch.zeros(n_rows * K, D, dtype=torch.float64).index_add_(0, node * K + hop, vals).view(n_rows, K, D)
    v = torch.nn.functional.gelu(S) + ptab.double()[uid[:n_rows].long()]
    return S, (v * theta.double().unsqueeze(0)).sum(1)


@functools.lru_cache(maxsize=None)
def _case(D, K, n_dict, N=N_BIG):
    """inputs (CPU), the device CSR and the float64 reference, shared by the tests of one shape and left unchanged"""
    from kp_gnn_amd.khop_csr import KHopCSR
    ei, ea = _graph(N, K, seed=D * 100 + K)
    g = torch.Generator().manual_seed(D * 1000 + K * 10 + n_dict)
    c = dict(xs=[torch.randn(N, D, generator=g) for _ in range(K)], t0=torch.randn(N0, D, generator=g) * 0.3,
             tk=torch.randn(NK, D, generator=g) * 0.3, ptab=torch.randn(n_dict, D, generator=g),
             alphas=torch.randn(D, generator=g), uid=_uid(N, K, n_dict))
    c["theta"] = _theta_ref(c["alphas"], K).float()
    c["csr"] = KHopCSR.build(ei.to(_dev()), ea.to(_dev()), N)
    c["S_ref"], c["h_ref"] = _reference(c["csr"], K, c["xs"], c["t0"], c["tk"], c["ptab"], c["uid"],
                                        _theta_ref(c["alphas"], K), N)
    c["h_ref_theta"] = _reference(c["csr"], K, c["xs"], c["t0"], c["tk"], c["ptab"], c["uid"], c["theta"], N)[1]
    return c


def _launch(c, K, theta_mode, csr=None, bf16=False, n_rows=None):
    """(hout, pre, theta buffer) of one kpgnn_aggregate_fwd launch on fresh device copies of the case's inputs"""
    from kp_gnn_amd import ops
    dev = _dev()
    xs = [x[:n_rows].to(dev) for x in c["xs"]]
    if bf16:
        xs = [x.to(torch.bfloat16).contiguous() for x in xs]
    if theta_mode == "alphas":
        alphas = c["alphas"].to(dev)
        theta = torch.empty(K, alphas.numel(), dtype=torch.float32, device=dev)
    else:
        alphas, theta = None, c["theta"].to(dev)
    hout, pre = ops.aggregate_fwd_raw(csr if csr is not None else c["csr"], K, ops.MODE_GINPLUS, None, c["t0"].to(dev),
                                      c["tk"].to(dev), None, None, theta, None, True, ptab=c["ptab"].to(dev),
                                      uid=c["uid"][:n_rows].to(dev).contiguous(), xs=xs, alphas=alphas, bf16=bf16)
    return hout, pre, theta


# (D, K): G = 32 the bench row shape; K = 1 the theta = 1 layer; G = 16; G = 4 <= K, which the host must route to the generic
# instantiation.  n_dict = 3 is staged in LDS wherever a cap allows, 40 never under the present cap.
SHAPES = [(104, 8, 3), (104, 8, 40), (104, 1, 3), (64, 8, 3), (16, 8, 3)]


@pytest.mark.parametrize("theta_mode", ["alphas", "theta"])
@pytest.mark.parametrize("D,K,n_dict", SHAPES)
def test_epilogue_vs_float64(D, K, n_dict, theta_mode):
    c = _case(D, K, n_dict)
    rp = c["csr"].rowptr_dst.cpu().view(-1)
    seg = (rp[1:] - rp[:-1])[:N_BIG * K].view(N_BIG, K)
    assert int(seg[HEAVY].max()) >= 70 and int(seg[ALONE].sum()) == 0 and int(seg[LATE, :K - 1].sum()) == 0
    assert int(seg[LATE, K - 1]) > 0 and (K < 3 or int(seg[GAPPY, 1:K - 1].sum()) == 0)
    hout, pre, theta = _launch(c, K, theta_mode)
    _close(theta, _theta_ref(c["alphas"], K), "theta_out" if theta_mode == "alphas" else "theta")
    _close(pre, c["S_ref"], "S")
    _close(hout, c["h_ref"] if theta_mode == "alphas" else c["h_ref_theta"], "hout")


@pytest.mark.parametrize("D,K,n_dict", [(104, 8, 40), (16, 8, 3)])
def test_two_launches_are_bit_identical(D, K, n_dict):
    c = _case(D, K, n_dict)
    h1, p1, _ = _launch(c, K, "alphas")
    h2, p2, _ = _launch(c, K, "alphas")
    assert torch.equal(h1, h2) and torch.equal(p1, p2)


def test_dynamic_rows_flush_the_last_live_node_only(monkeypatch):
    """Capacity 300, 257 live rows, dead input rows NaN, outputs pre-filled with a sentinel: the live rows are the exact-shape
    launch on 257 rows bit for bit, the dead rows of hout and S still hold the sentinel.
    The exact-shape launch runs under dynamic_rows(257, 257): a plain launch on 257 rows is handed to agg_fwd_small_kernel,
    whose hout differs from this kernel's in the last bit (it did before the epilogue change as well), so that one is
    held to the float64 reference instead."""
    from kp_gnn_amd import ops
    from kp_gnn_amd.khop_csr import KHopCSR
    dev = _dev()
    CAP, LIVE, D, K, U = 300, 257, 104, 8, 40
    SENT = -12345.0
    ei, ea = _graph(CAP, K, seed=77, n_live=LIVE)
    g = torch.Generator().manual_seed(5)
    c = dict(xs=[torch.randn(CAP, D, generator=g) for _ in range(K)], t0=torch.randn(N0, D, generator=g) * 0.3,
             tk=torch.randn(NK, D, generator=g) * 0.3, ptab=torch.randn(U, D, generator=g),
             alphas=torch.randn(D, generator=g), uid=_uid(CAP, K, U))
    csr_live = KHopCSR.build(ei.to(dev), ea.to(dev), LIVE)
    small = _launch(c, K, "alphas", csr=csr_live, n_rows=LIVE)          # (N <= 4096: agg_fwd_small_kernel, another kernel)
    with ops.dynamic_rows(torch.tensor([LIVE], dtype=torch.int32, device=dev), LIVE):
        exact = _launch(c, K, "alphas", csr=csr_live, n_rows=LIVE)      # the kernel under test on exactly the 257 rows
    for x in c["xs"]:
        x[LIVE:] = float("nan")
    csr = KHopCSR.build(ei.to(dev), ea.to(dev), CAP)
    cnt = torch.tensor([LIVE], dtype=torch.int32, device=dev)
    real_empty = torch.empty

    def sentinel_empty(*a, **kw):          # (aggregate_fwd_raw allocates hout and S itself)
        t = real_empty(*a, **kw)
        return t.fill_(SENT) if t.is_floating_point() else t

    with ops.dynamic_rows(cnt, CAP):
        monkeypatch.setattr(torch, "empty", sentinel_empty)
        try:
            hout, pre, _ = _launch(c, K, "alphas", csr=csr)
        finally:
            monkeypatch.setattr(torch, "empty", real_empty)
    assert torch.equal(hout[:LIVE], exact[0]) and torch.equal(pre[:LIVE], exact[1])
    assert bool((hout[LIVE:] == SENT).all()) and bool((pre[LIVE:] == SENT).all())
    S_ref, h_ref = _reference(csr, K, c["xs"], c["t0"], c["tk"], c["ptab"], c["uid"], _theta_ref(c["alphas"], K), LIVE)
    _close(pre[:LIVE], S_ref, "S (live rows)")
    _close(hout[:LIVE], h_ref, "hout (live rows)")
    _close(small[1], S_ref, "S (small-batch kernel)")
    _close(small[0], h_ref, "hout (small-batch kernel)")


@pytest.mark.parametrize("D,K,n_dict", [(104, 8, 40), (16, 8, 3)])
def test_bf16_rows_vs_fp32_launch(D, K, n_dict):
    """bf16 hop slots and S against the fp32 launch: the bound of test_bf16_storage_aggregate_vs_fp32 (2e-2 of the scale).
    (104, 8): the FAST instantiation with bf16 rows; (16, 8): G = 4 <= K, the generic instantiation with bf16 rows."""
    c = _case(D, K, n_dict)
    h32, p32, _ = _launch(c, K, "alphas")
    h16, p16, _ = _launch(c, K, "alphas", bf16=True)
    assert p16.dtype == torch.bfloat16 and p32.dtype == torch.float32
    _rel_close(h16, h32, "hout", BF16_RTOL)
    _rel_close(p16, p32, "S", BF16_RTOL)
    _close(h32, c["h_ref"], "hout fp32")
