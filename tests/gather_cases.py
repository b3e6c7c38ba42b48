"""Hand-built hard K-hop CSRs and float64 references for the K-hop gather kernels (helper, not a test module).

hard_csr builds a (node, hop)-keyed CSR in the layout of include/kpgnn.h whose special nodes sit on the bookkeeping of the
sub-group kernels of csrc/aggregate.hip: the pair list of a node is fetched in chunks of G pairs, the first PF rows of a hop are
requested one hop ahead (clipped at the chunk end), a hop's result is stored one hop late.  G and PF are those of the
instantiation under test (prefetch_depth).  fwd_reference / bwd_reference restate the contract of kpgnn_aggregate_fwd /
kpgnn_aggregate_bwd in float64 with index_add_ over the pair list; tests/test_gather_cases_host.py checks both on the CPU."""
import torch

U = 2.0 ** -24                      # unit roundoff of fp32

# the special nodes (every batch has at least MIN_NODES nodes; the LAST node is a copy of EDGE)
GAPPY, ALONE, LATE, ONES, EXACT, AFTER_EXACT, EDGE, EVERY, DUP = 2, 3, 5, 7, 9, 10, 12, 14, 16
MIN_NODES = 18
EVERY_MAX_PAIRS = 300               # EVERY gets its G + 1 pairs per hop only where K_csr * (G + 1) stays below this

MODE_GIN, MODE_GINPLUS, MODE_GCN, MODE_SUM = 0, 1, 2, 3      # include/kpgnn.h KPGNN_MODE_*


def prefetch_depth(G):
    """rows requested one hop ahead by agg_fwd_kernel / agg_bwd_kernel<.., G, ..> (`constexpr int PF` in aggregate.hip)"""
    return 2 if G < 32 else 4


def case_nodes(G):
    """the smallest batch that places every special node and spans two full tiles of 256 / G nodes plus a ragged one:
    max(40, 2 * 256 / G + 3), one more where that is a multiple of the tile (G = 32, 64: 41)"""
    n = max(40, 2 * (256 // G) + 3)
    return n + 1 if n % (256 // G) == 0 else n


def special_lens(K_csr, G, PF):
    """name -> the K_csr segment lengths of a special node (None: the node keeps its random lengths)"""
    K = K_csr
    late = [0] * K
    late[K - 1] = 4
    gappy = [0] * K
    gappy[0] = gappy[K - 1] = 3
    exact = [G // K + (1 if h < G % K else 0) for h in range(K)]
    edge = [2 * G + PF + 1] if K == 1 else [G - 1, 2 * G + PF + 1] + [1] * (K - 2)
    return {
        "ALONE": [0] * K,
        "LATE": late,
        "GAPPY": gappy,
        "ONES": [1] * K,
        "EXACT": exact,
        "AFTER_EXACT": [G] + [2] * (K - 1),
        "EDGE": edge,
        "EVERY": [G + 1] * K if K * (G + 1) <= EVERY_MAX_PAIRS else None,
        "DUP": [5] + [2] * (K - 1),
    }


SPECIAL_NODE = {"ALONE": ALONE, "LATE": LATE, "GAPPY": GAPPY, "ONES": ONES, "EXACT": EXACT, "AFTER_EXACT": AFTER_EXACT,
                "EDGE": EDGE, "EVERY": EVERY, "DUP": DUP}


class HardCSR:
    """rowptr int32 [N*K_csr+1], col int32 [A], code int16 [A] (the 16-bit tensor the descriptors take), seg int64 [A] (the
    node * K_csr + hop of every pair), lens int64 [N, K_csr]"""

    def __init__(self, N, K_csr, G, PF, rowptr, col, code, seg, lens):
        self.N, self.K_csr, self.G, self.PF = N, K_csr, G, PF
        self.rowptr, self.col, self.code, self.seg, self.lens = rowptr, col, code, seg, lens


def hard_csr(N, K_csr, G, PF, seed, n_code0=5, n_codek=7, graph_ptr=None):
    """Base segment lengths random in 0..5, then the special nodes (module docstring); the last node copies EDGE.
    Every col is a node of the batch - of the pair's own graph where graph_ptr (node offsets, [num_graphs + 1]) is given -
    and every code is >= 1 and below its table's row count (hop 0: n_code0, later hops: n_codek)."""
    assert N >= MIN_NODES and K_csr >= 1 and n_code0 >= 2 and n_codek >= 2
    g = torch.Generator().manual_seed(4321 + 1000 * seed + 10 * G + K_csr)
    lens = torch.randint(0, 6, (N, K_csr), generator=g)
    for name, want in special_lens(K_csr, G, PF).items():
        if want is not None:
            lens[SPECIAL_NODE[name]] = torch.tensor(want)
    lens[N - 1] = lens[EDGE]
    flat = lens.reshape(-1)
    rowptr = torch.zeros(N * K_csr + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(flat, 0)
    A = int(rowptr[-1])
    seg = torch.repeat_interleave(torch.arange(N * K_csr), flat)
    node, hop = seg // K_csr, seg % K_csr
    if graph_ptr is None:
        lo, hi = torch.zeros(A, dtype=torch.int64), torch.full((A,), N, dtype=torch.int64)
    else:
        gp = torch.as_tensor(graph_ptr, dtype=torch.int64)
        assert int(gp[0]) == 0 and int(gp[-1]) == N and bool((gp[1:] > gp[:-1]).all())
        gid = torch.searchsorted(gp, node, right=True) - 1
        lo, hi = gp[gid], gp[gid + 1]
    col = lo + (torch.rand(A, generator=g, dtype=torch.float64) * (hi - lo).double()).long().clamp_(max=N - 1)
    col = torch.minimum(col, hi - 1)
    # DUP: self pairs and repeated pairs - hop 0 = [self, self, j, j, j], later hops = [self, j]
    for h in range(K_csr):
        b = int(rowptr[DUP * K_csr + h])
        j = col[b + int(lens[DUP, h]) - 1].clone()
        if h == 0:
            col[b:b + 2] = DUP
            col[b + 2:b + 5] = j
        else:
            col[b] = DUP
    code = torch.where(hop == 0, torch.randint(1, n_code0, (A,), generator=g), torch.randint(1, n_codek, (A,), generator=g))
    assert bool((col >= lo).all()) and bool((col < hi).all()) and bool((code >= 1).all())
    return HardCSR(N, K_csr, G, PF, rowptr.to(torch.int32), col.to(torch.int32), code.to(torch.int16), seg, lens)


def chunk_walk(lens, G, PF):
    """The index bookkeeping of the chunked pair walk (agg_fwd_kernel's non-GCN loop, agg_bwd_kernel's CHUNKED loop) for ONE
    node with the hop lengths `lens`, restated on the host to show which branches a node reaches.  Per hop k a dict:
      prefetched   rows of hop k requested one hop ahead (prn: min(PF, pairs of the hop left in the current chunk), >= 0)
      refill_first the chunk was refilled at the hop's FIRST pair (nothing of the hop had been prefetched)
      chunks       chunks of G pairs the hop's pairs lie in
      tail         the hop's walk ended on the one-pair tail (t < lim) at least once"""
    K = len(lens)
    rp = [0]
    for n in lens:
        rp.append(rp[-1] + int(n))
    cbase, beg, hops = 0, 0, []
    prn = max(0, min(PF, min(rp[1], cbase + G) - beg))
    for k in range(K):
        end, cn = rp[k + 1], prn
        ev = dict(prefetched=cn, refill_first=False, chunks={cbase // G} if cn else set(), tail=False)
        if k + 1 < K:
            prn = max(0, min(PF, min(rp[k + 2], cbase + G) - end))
        pos, summed = beg + cn, cn
        while pos < end:
            if pos >= cbase + G:
                cbase += G
                ev["refill_first"] |= pos == beg
            lim = min(end, cbase + G) - cbase
            t = pos - cbase
            assert 0 <= t < lim <= G                            # every broadcast stays inside the sub-group's G lanes
            ev["chunks"].add(cbase // G)
            ev["tail"] |= (lim - t) % 2 == 1
            summed += lim - t
            pos = cbase + lim
        assert summed == int(lens[k]) and (cn == 0 or beg + cn <= min(end, (beg // G + 1) * G))
        ev["chunks"] = len(ev["chunks"])
        hops.append(ev)
        beg = end
    return hops


def edge_list(c, K):
    """The equivalent K-hop edge list of the first K hops: one edge per pair, edge_index [2, E] = (col, owner node),
    edge_attr [E, K] = the pair's code in its own hop and 0 (inactive) in the others; pairs in list order."""
    node, hop = c.seg // c.K_csr, c.seg % c.K_csr
    keep = hop < K
    node, hop = node[keep], hop[keep]
    ei = torch.stack([c.col.long()[keep], node])
    ea = torch.zeros(node.numel(), K, dtype=torch.int64)
    ea[torch.arange(node.numel()), hop] = c.code.long()[keep]
    return ei, ea


def degree_dis(c):
    """dis [N, K_csr] float64 = (segment length + 1)^-1/2 (KPGCN.py:11-25, 106-109: the self loop counts)"""
    return (c.lens.double() + 1.0).pow(-0.5)


def theta_ref(alphas, K):
    """softmax_k(a (1 - a)^k), a = sigmoid(alphas) (the geometric combine, combine.py:43-50), float64"""
    a = torch.sigmoid(alphas.double())
    return torch.softmax(torch.stack([a * (1 - a) ** k for k in range(K)]), 0)


def _pairs(c, K):
    node, hop = c.seg // c.K_csr, c.seg % c.K_csr
    keep = hop < K
    return node[keep], hop[keep], c.col.long()[keep], c.code.long()[keep]


def _tab_rows(t0, tk, code, hop):
    tabs = torch.cat([t0.double(), tk.double()]) if tk is not None else t0.double()
    return tabs[code + (hop > 0) * t0.shape[0]]


def fwd_reference(c, K, mode, x, t0=None, tk=None, xbias=None, dis=None, periph=None, ptab=None, uid=None, eps=None,
                  theta=None):
    """kpgnn_aggregate_fwd in float64.  x [N, K, D] (any strides); t0 / tk the code tables or None (tk None where K == 1);
    dis [N, K_csr] for GCN; periph [N, K, D] or the dictionary (ptab [U, D], uid [N, >= K]); eps a float; theta [K, D].
    Returns S (what `pre` receives), out [N, K, D], hout [N, D] (None without theta) and sum_bound: per element
    2 n 2^-24 sum|addends| of S, n the segment length - the bound of sequential fp32 summation."""
    N, Kc = c.N, c.K_csr
    x = x.double()
    D = x.shape[2]
    node, hop, col, code = _pairs(c, K)
    gcn = mode == MODE_GCN
    vals = x[col, hop]
    if t0 is not None:
        vals = vals + _tab_rows(t0, tk, code, hop)
    xb = torch.zeros(K, D, dtype=torch.float64)
    if xbias is not None:
        xb[1:] = xbias.double()
    lens = c.lens[:, :K].double()
    slot = node * K + hop
    if gcn:
        d2 = dis.double().view(N, Kc)
        w = d2[col, hop]
        S = torch.zeros(N * K, D, dtype=torch.float64).index_add_(0, slot, vals * w[:, None]).view(N, K, D)
        wacc = torch.zeros(N * K, dtype=torch.float64).index_add_(0, slot, w).view(N, K)
        S = S + wacc[:, :, None] * xb[None]
        self_ = x + xb[None]
        if t0 is not None:
            self_ = self_ + torch.stack([t0[1].double()] + [tk[1].double()] * (K - 1))[None]    # self-loop code 1
        di = d2[:, :K]
        S = (S + di[:, :, None] * self_) * di[:, :, None]
    else:
        S = torch.zeros(N * K, D, dtype=torch.float64).index_add_(0, slot, vals).view(N, K, D)
        S = S + lens[:, :, None] * xb[None]                     # the constant row, once per gathered pair of hops >= 1
    mag = torch.zeros(N * K, D, dtype=torch.float64).index_add_(0, slot, vals.abs()).view(N, K, D)
    v = S
    if mode == MODE_GINPLUS:
        v = torch.nn.functional.gelu(S)
    if gcn:
        v = torch.relu(S)
    if periph is not None:
        v = v + periph.double()
    elif uid is not None:
        v = v + ptab.double()[uid.long()[:, :K]]
    if mode == MODE_GIN:
        v = v + (1.0 + (eps or 0.0)) * (x + xb[None])
    hout = (v * theta.double()[None]).sum(1) if theta is not None else None
    return dict(S=S, out=v, hout=hout, sum_bound=2.0 * lens[:, :, None] * U * mag)


def bwd_reference(c, K, mode, g, dis=None, eps=None, old=None, acc_mask=0, n_code0=0, n_codek=0):
    """kpgnn_aggregate_bwd in float64 with c read as the by-source CSR.  g [N, K, D] = dL/dS; old [N, K, D]: what the
    accumulating hops (bits of acc_mask) held before; n_code0 > 0 asks for the table gradients.
    Returns gx [N, K, D], gtable0 / gtablek (None when not asked for; gtablek None where K == 1) and sum_bound as in
    fwd_reference for the plain sum."""
    N, Kc = c.N, c.K_csr
    g = g.double()
    D = g.shape[2]
    node, hop, col, code = _pairs(c, K)
    slot = node * K + hop
    vals = g[col, hop]
    self_ = None
    if mode == MODE_GCN:
        d2 = dis.double().view(N, Kc)
        vals = vals * (d2[node, hop] * d2[col, hop])[:, None]
        self_ = g * (d2[:, :K] ** 2)[:, :, None]
    elif mode == MODE_GIN:
        self_ = (1.0 + (eps or 0.0)) * g
    gx = torch.zeros(N * K, D, dtype=torch.float64).index_add_(0, slot, vals).view(N, K, D)
    mag = torch.zeros(N * K, D, dtype=torch.float64).index_add_(0, slot, vals.abs()).view(N, K, D)
    if self_ is not None:
        gx = gx + self_
    for k in range(K):
        if (acc_mask >> k) & 1:
            gx[:, k] += old[:, k].double()
    gt0 = gtk = None
    if n_code0:
        gt0 = torch.zeros(n_code0, D, dtype=torch.float64).index_add_(0, code[hop == 0], vals[hop == 0])
        if K > 1:
            gtk = torch.zeros(n_codek, D, dtype=torch.float64).index_add_(0, code[hop > 0], vals[hop > 0])
        if mode == MODE_GCN:                                    # the self loop's code row 1
            gt0[1] += self_[:, 0].sum(0)
            if K > 1:
                gtk[1] += self_[:, 1:].sum((0, 1))
    return dict(gx=gx, gtable0=gt0, gtablek=gtk, sum_bound=2.0 * c.lens[:, :K].double()[:, :, None] * U * mag)
