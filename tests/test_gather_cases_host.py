"""CPU: the hard K-hop CSRs and float64 references of tests/gather_cases.py, which tests/test_gather_row_shapes.py holds the
gather kernels to.  The special nodes have the segment lengths their names claim for every chunk size G, the CSR stays inside
the contract of include/kpgnn.h, and the references equal the oracle's materialised message passing (LO.propagate_sum /
LO.masked_message / LO.khop_degree) evaluated in float64 on the equivalent edge list."""
import pytest
import torch

import gather_cases as GC
from oracle import kp_layers_oracle as LO


@pytest.mark.parametrize("K_csr", [1, 2, 3, 8, 16])
@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_special_nodes_have_the_claimed_segments(G, K_csr):
    PF = GC.prefetch_depth(G)
    assert PF == (2 if G < 32 else 4)
    N = GC.case_nodes(G)
    assert N >= 40 and N % (256 // G) != 0 and N > 2 * (256 // G)
    c = GC.hard_csr(N, K_csr, G, PF, seed=1)
    rp = c.rowptr.long()
    lens = (rp[1:] - rp[:-1]).view(N, K_csr)
    assert torch.equal(lens, c.lens) and int(rp[0]) == 0 and int(rp[-1]) == c.col.numel() == c.code.numel() == c.seg.numel()
    last = K_csr - 1
    assert int(lens[GC.ALONE].sum()) == 0
    assert int(lens[GC.LATE, :last].sum()) == 0 and int(lens[GC.LATE, last]) > 0
    assert int(lens[GC.GAPPY, 0]) > 0 and int(lens[GC.GAPPY, last]) > 0 and int(lens[GC.GAPPY, 1:last].sum()) == 0
    assert bool((lens[GC.ONES] == 1).all())
    assert int(lens[GC.EXACT].sum()) == G
    # the node after EXACT: hop 0 ends exactly one chunk behind the node's first pair, more hops follow
    b = int(rp[GC.AFTER_EXACT * K_csr])
    assert int(rp[GC.AFTER_EXACT * K_csr + 1]) == b + G
    assert K_csr == 1 or bool((lens[GC.AFTER_EXACT, 1:] > 0).all())
    if K_csr > 1:
        assert int(lens[GC.EDGE, 0]) == G - 1 and int(lens[GC.EDGE, 1]) == 2 * G + PF + 1
    else:
        assert int(lens[GC.EDGE, 0]) == 2 * G + PF + 1
    if K_csr * (G + 1) <= GC.EVERY_MAX_PAIRS:
        assert bool((lens[GC.EVERY] == G + 1).all())
    assert torch.equal(lens[N - 1], lens[GC.EDGE])
    # DUP: self pairs and repeated pairs
    b = int(rp[GC.DUP * K_csr])
    dup0 = c.col[b:b + int(lens[GC.DUP, 0])].tolist()
    assert dup0[:2] == [GC.DUP, GC.DUP] and dup0[2] == dup0[3] == dup0[4]
    # inside the contract
    assert c.col.dtype == torch.int32 and c.rowptr.dtype == torch.int32 and c.code.dtype == torch.int16
    assert int(c.col.min()) >= 0 and int(c.col.max()) < N
    hop = c.seg % K_csr
    assert int(c.code.min()) >= 1 and int(c.code[hop == 0].max()) < 5 and (K_csr == 1 or int(c.code[hop > 0].max()) < 7)
    assert torch.equal(c.seg, torch.repeat_interleave(torch.arange(N * K_csr), lens.reshape(-1)))


@pytest.mark.parametrize("K_csr", [2, 3, 8, 16])
@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_special_nodes_reach_the_branches_of_the_chunked_walk(G, K_csr):
    """the bookkeeping of the kernels' chunked pair walk, restated in gather_cases.chunk_walk, on the special nodes"""
    PF = GC.prefetch_depth(G)
    c = GC.hard_csr(GC.case_nodes(G), K_csr, G, PF, seed=1)
    walk = lambda node: GC.chunk_walk(c.lens[node].tolist(), G, PF)
    after = walk(GC.AFTER_EXACT)            # hop 0 fills the chunk: nothing of hop 1 can be prefetched, hop 1 opens with a refill
    assert after[0]["chunks"] == 1 and after[1]["prefetched"] == 0 and after[1]["refill_first"]
    edge = walk(GC.EDGE)                    # one pair of the long hop is left in the chunk: prefetch clipped to 1, 3+ chunks
    assert edge[1]["prefetched"] == 1 < PF and edge[1]["chunks"] >= 3 and not edge[1]["refill_first"]
    assert edge[0]["tail"]                  # G - 1 - PF pairs behind the prefetched ones: odd
    assert walk(c.N - 1) == edge
    exact = walk(GC.EXACT)                  # the node's pairs end with its only chunk
    assert sum(h["chunks"] > 1 for h in exact) == 0 and not any(h["refill_first"] for h in exact)
    assert all(h["prefetched"] == 1 and h["chunks"] == 1 for h in walk(GC.ONES)[:G])
    assert all(h["prefetched"] == 0 and h["chunks"] == 0 for h in walk(GC.ALONE))
    if K_csr * (G + 1) <= GC.EVERY_MAX_PAIRS:                   # every hop crosses a chunk end, at a different lane each time
        every = walk(GC.EVERY)
        assert all(h["chunks"] == 2 for h in every[:G])
        assert len({h["prefetched"] for h in every}) > 1 or K_csr < 3
    for node in range(c.N):                                     # (chunk_walk asserts that every pair is summed once)
        walk(node)


def test_pairs_stay_inside_their_graph():
    gp = [0, 1, 4, 13, 40]
    c = GC.hard_csr(40, 3, 8, 2, seed=2, graph_ptr=gp)
    node = c.seg // 3
    gpt = torch.tensor(gp)
    gid = torch.searchsorted(gpt, node, right=True) - 1
    col = c.col.long()
    assert bool((col >= gpt[gid]).all()) and bool((col < gpt[gid + 1]).all())
    assert bool((col[node == 0] == 0).all())                    # the one-node graph: self pairs only


def _inputs(N, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    t0, tk = r(5, D), r(7, D)
    return dict(x=r(N, K, D), t0=t0, tk=tk, P=r(N, K, D), xbias=r(D), g=r(N, K, D), old=r(N, K, D), theta=r(K, D))


def _oracle_S(c, K, x, t0, tk, xbias):
    """S of the non-GCN modes by the oracle's materialised sequence, float64"""
    ei, ea = GC.edge_list(c, K)
    x = torch.cat([x[:, :1], x[:, 1:] + xbias], 1)              # x[:, 1:] += hopk_node_path_emb(0) (KPGIN.py:92-94)
    emb = LO.edge_code_embedding({"hop1_edge_emb.weight": t0, "hopk_edge_emb.weight": tk}, ea, K)
    return LO.propagate_sum(c.N, ei, LO.masked_message(x.index_select(0, ei[0]), emb, ea)), x


def test_gin_references_equal_the_oracle():
    N, K_csr, K, D, G = 40, 4, 3, 6, 8
    c = GC.hard_csr(N, K_csr, G, 2, seed=3)
    i = _inputs(N, K, D, 11)
    xo = i["x"].clone().requires_grad_(True)
    t0o, tko = i["t0"].clone().requires_grad_(True), i["tk"].clone().requires_grad_(True)
    S, xb = _oracle_S(c, K, xo, t0o, tko, i["xbias"])
    out = S + i["P"] + (1 + 0.3) * xb
    ref = GC.fwd_reference(c, K, GC.MODE_GIN, i["x"], t0=i["t0"], tk=i["tk"], xbias=i["xbias"], periph=i["P"], eps=0.3,
                           theta=i["theta"])
    assert torch.allclose(ref["S"], S.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["out"], out.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["hout"], (out.detach() * i["theta"][None]).sum(1), rtol=1e-12, atol=1e-12)
    # GELU / SUM epilogues and the dictionary form of P on the same S
    uid = (torch.arange(N)[:, None] + torch.arange(K)[None]) % 3
    rp = GC.fwd_reference(c, K, GC.MODE_GINPLUS, i["x"], t0=i["t0"], tk=i["tk"], xbias=i["xbias"], ptab=i["P"][0], uid=uid)
    assert torch.allclose(rp["out"], torch.nn.functional.gelu(S.detach()) + i["P"][0][uid], rtol=1e-12, atol=1e-12)
    rs = GC.fwd_reference(c, K, GC.MODE_SUM, i["x"])
    S0, _ = _oracle_S(c, K, i["x"], torch.zeros(5, D, dtype=torch.float64), torch.zeros(7, D, dtype=torch.float64),
                      torch.zeros(D, dtype=torch.float64))
    assert torch.allclose(rs["out"], S0, rtol=1e-12, atol=1e-12) and torch.equal(rs["out"], rs["S"])
    assert bool((rs["sum_bound"][GC.ALONE] == 0).all()) and bool((rs["S"][GC.ALONE] == 0).all())
    # backward: the same CSR read as the by-source one is the forward of the transposed edge list; autograd of the oracle
    # with respect to x and the tables against bwd_reference
    ei, ea = GC.edge_list(c, K)
    ei_t = torch.stack([ei[1], ei[0]])                          # pairs of segment (j, k): j is the SOURCE, col the destination
    emb = LO.edge_code_embedding({"hop1_edge_emb.weight": t0o, "hopk_edge_emb.weight": tko}, ea, K)
    St = LO.propagate_sum(N, ei_t, LO.masked_message(xo.index_select(0, ei_t[0]), emb, ea)) + (1 + 0.3) * xo
    (St * i["g"]).sum().backward()
    rb = GC.bwd_reference(c, K, GC.MODE_GIN, i["g"], eps=0.3, old=i["old"], acc_mask=0b101, n_code0=5, n_codek=7)
    want = xo.grad.clone()
    want[:, 0] += i["old"][:, 0]
    want[:, 2] += i["old"][:, 2]
    assert torch.allclose(rb["gx"], want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rb["gtable0"], t0o.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rb["gtablek"], tko.grad, rtol=1e-12, atol=1e-12)


def test_gcn_references_equal_the_oracle():
    N, K_csr, K, D, G = 40, 3, 3, 5, 4
    c = GC.hard_csr(N, K_csr, G, 2, seed=4)
    i = _inputs(N, K, D, 12)
    ei, ea = GC.edge_list(c, K)
    loop = torch.arange(N)
    ei2 = torch.cat([ei, loop.unsqueeze(0).repeat(2, 1)], 1)    # add_self_loops, code 1 (KPGCN.py:85-89)
    ea2 = torch.cat([ea, torch.ones(N, K, dtype=torch.long)], 0)
    deg = LO.khop_degree(ei2[1], N, ea2, dtype=torch.float64)
    dis = deg.pow(-0.5)
    assert torch.allclose(GC.degree_dis(c), dis, rtol=1e-15, atol=0)
    xo = i["x"].clone().requires_grad_(True)
    t0o, tko = i["t0"].clone().requires_grad_(True), i["tk"].clone().requires_grad_(True)
    xb = torch.cat([xo[:, :1], xo[:, 1:] + i["xbias"]], 1)
    emb = LO.edge_code_embedding({"hop1_edge_emb.weight": t0o, "hopk_edge_emb.weight": tko}, ea2, K)
    norm = dis[ei2[0]] * dis[ei2[1]]
    msg = (norm.unsqueeze(-1) * (xb.index_select(0, ei2[0]) + emb)).masked_fill(ea2.unsqueeze(-1) == 0, 0.)
    S = LO.propagate_sum(N, ei2, msg)
    out = torch.relu(S) + i["P"]
    ref = GC.fwd_reference(c, K, GC.MODE_GCN, i["x"], t0=i["t0"], tk=i["tk"], xbias=i["xbias"], dis=dis, periph=i["P"])
    assert torch.allclose(ref["S"], S.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["out"], out.detach(), rtol=1e-12, atol=1e-12)
    # backward with the CSR read as the by-source one and a dis of its own (an array to the kernel, no degree)
    dis_b = torch.rand(N, K_csr, dtype=torch.float64) + 0.5
    ei_t = torch.stack([ei2[1], ei2[0]])
    norm_t = dis_b[ei_t[0]] * dis_b[ei_t[1]]
    xo.grad = t0o.grad = tko.grad = None
    emb = LO.edge_code_embedding({"hop1_edge_emb.weight": t0o, "hopk_edge_emb.weight": tko}, ea2, K)
    msg = (norm_t.unsqueeze(-1) * (xo.index_select(0, ei_t[0]) + emb)).masked_fill(ea2.unsqueeze(-1) == 0, 0.)
    (LO.propagate_sum(N, ei_t, msg) * i["g"]).sum().backward()
    rb = GC.bwd_reference(c, K, GC.MODE_GCN, i["g"], dis=dis_b, n_code0=5, n_codek=7)
    assert torch.allclose(rb["gx"], xo.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rb["gtable0"], t0o.grad, rtol=1e-12, atol=1e-12)
    assert torch.allclose(rb["gtablek"], tko.grad, rtol=1e-12, atol=1e-12)
