"""CPU: the host route of the property-graph generator (kp_gnn_amd/property_graphs.py: the definition of include/kpgnn.h in
numpy) and the front end as far as it needs no device.  The generator keeps the reference's LAWS on another stream, so the
yardsticks are laws: the five fixed structures and the tree construction equal the networkx constructors the reference calls;
the degree law, Barabasi-Albert's degrees and the tree's leaf counts match networkx's by chi-square; Erdos-Renyi, the
attachments, the mixture, the relabelling, `randomize` and the acceptance rate match their closed forms.  Every statistical
bound is the 0.999 quantile (or 4.5 binomial sigma) on a fixed-seed, deterministic run; the statistic is printed.  Against the
definition written a second time in plain integers (tests/property_graph_cases.py) the numpy route gives the same graphs."""
import math

import networkx as nx
import numpy as np
import pytest

import property_graph_cases as PC

# the 0.999 quantile of chi-square at 1 .. 40 degrees of freedom
Q999 = (10.83, 13.82, 16.27, 18.47, 20.52, 22.46, 24.32, 26.12, 27.88, 29.59, 31.26, 32.91, 34.53, 36.12, 37.70, 39.25, 40.79,
        42.31, 43.82, 45.31, 46.80, 48.27, 49.73, 51.18, 52.62, 54.05, 55.48, 56.89, 58.30, 59.70, 61.10, 62.49, 63.87, 65.25,
        66.62, 67.99, 69.35, 70.70, 72.05, 73.40)


def _pg():
    from kp_gnn_amd import property_graphs
    return property_graphs


def _chi2(observed, expected):
    observed, expected = np.asarray(observed, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((observed - expected) ** 2 / expected).sum())


def _nx_fixed(t, n):
    r = PC.divisor(n)
    if t == "GRID":
        return nx.grid_2d_graph(r, n // r)
    if t == "CAVEMAN":
        return nx.caveman_graph(r, n // r)
    if t == "LINE":
        return nx.path_graph(n)
    if t == "STAR":
        return nx.star_graph(n - 1)
    G = nx.ladder_graph(n // 2)
    if n % 2:
        G.add_edge(0, n - 1)
    return G


@pytest.mark.parametrize("t", PC.FIXED)
def test_fixed_structures_are_the_networkx_constructors(t):
    """Primes, squares and odd ladders among the sizes; canonical labels are the positions in list(G)."""
    for n in PC.FIXED_SIZES:
        G = _nx_fixed(t, n)
        want = nx.to_numpy_array(G, nodelist=list(G)).astype(bool)
        assert np.array_equal(_pg().structure(n, t, 0, 0, 0), want), (t, n)


@pytest.mark.parametrize("n", (2, 3, 15, 24, 128))
def test_tree_is_degree_sequence_tree_of_a_tree_sequence(n):
    PG, swaps = _pg(), []
    for seed in range(200):
        deg, s = PG.tree_sequence(n, seed, 0, 0)
        swaps.append(s)
        if deg is None:
            assert s == 5000 and PG.structure(n, "TREE", seed, 0, 0) is None
            continue
        assert sum(deg) == 2 * n - 2 and min(deg) >= 1
        G = nx.degree_sequence_tree(deg)
        assert np.array_equal(PG.structure(n, "TREE", seed, 0, 0), nx.to_numpy_array(G, nodelist=list(G)).astype(bool)), seed
    print(f"n = {n}: swaps at most {max(swaps)}, {sum(s == 5000 for s in swaps)} sequences gave up")
    assert sum(s == 5000 for s in swaps) <= 2


def test_tree_degree_law():
    """100,000 words against P(1) = 5/9, P(k) = 4 / (2k-1)^2 - 4 / (2k+1)^2: k = 1 .. 9 and the tail, 9 degrees of freedom."""
    PG = _pg()
    k = PG.degrees(PG.words("TREE", 0, [0], 0, np.arange(100000))[0][0], 128)
    law = [PC.degree_law(c) for c in range(1, 10)]
    law.append(1 - sum(law))
    assert abs(law[-1] - 4 / 19 ** 2) < 1e-12
    observed = np.bincount(np.minimum(k, 10), minlength=11)[1:]
    chi2 = _chi2(observed, 100000 * np.array(law))
    print(f"degree law: chi-square {chi2:.2f} (bound 27.88)")
    assert chi2 < 27.88
    assert PG.degrees(np.array([0, 2 ** 32 - 1]), 5).tolist() == [1, 5]         # the clamp


def test_tree_leaf_counts_match_networkx():
    """4,000 sequences at n = 15 against 4,000 of nx.random_powerlaw_tree_sequence(15, tries=10000, seed=s): the histograms of
    the number of leaves.  (networkx's seeds 0 .. 3999 against its seeds 4000 .. 7999: 10.42 at 10 degrees of freedom, bound 29.59; this generator: 14.36.)"""
    PG = _pg()
    ours, theirs = np.zeros(16), np.zeros(16)
    for s in range(4000):
        deg, _ = PG.tree_sequence(15, 0, s, 0)
        ours[sum(d == 1 for d in deg)] += 1
        theirs[sum(d == 1 for d in nx.random_powerlaw_tree_sequence(15, tries=10000, seed=s))] += 1
    chi2, df = PC.chi2_two_samples(ours, theirs)
    print(f"leaf counts: chi-square {chi2:.2f} at {df} degrees of freedom (bound {Q999[df - 1]})")
    assert chi2 < Q999[df - 1]


@pytest.mark.parametrize("m", (1, 3, 11))
def test_barabasi_albert_structure(m):
    n = 12
    for gid in range(20):
        C = _pg().structure(n, "BARABASI_ALBERT", 0, gid, 0, param=m)
        assert np.array_equal(C, C.T) and not C.diagonal().any()
        assert C.sum() // 2 == m + m * (n - m - 1)
        low = np.tril(C, -1).sum(axis=1)
        assert low[0] == 0 and (low[1:m + 1] == 1).all() and C[1:m + 1, 0].all() and (low[m + 1:] == m).all()


def test_barabasi_albert_degrees_match_networkx():
    """The degree histogram of 4,000 graphs (n = 12, m = 3) against nx.barabasi_albert_graph(12, 3, seed) for seeds 0 .. 3999.
    (networkx's seeds 0 .. 3999 against its seeds 4000 .. 7999: 8.50 at 10 degrees of freedom, bound 29.59; this generator: 8.26.)"""
    n, m = 12, 3
    C, _ = _pg().structures(n, PC.TYPES["BARABASI_ALBERT"], 0, np.arange(4000), 0, param=m)
    ours = np.bincount(C.sum(axis=2).reshape(-1), minlength=n)
    theirs = np.zeros(n)
    for s in range(4000):
        theirs += np.bincount([d for _, d in nx.barabasi_albert_graph(n, m, seed=s).degree()], minlength=n)
    chi2, df = PC.chi2_two_samples(ours, theirs)
    print(f"BA degrees: chi-square {chi2:.2f} at {df} degrees of freedom (bound {Q999[df - 1]})")
    assert chi2 < Q999[df - 1]


def test_erdos_renyi_law():
    """Forced p = 1/4 at n = 16, 4,000 graphs: every pair within 4.5 binomial sigma of p, and the edge counts against
    Binomial(120, 1/4) with the tails pooled to an expectation of at least 5."""
    G, n, p = 4000, 16, 0.25
    C, _ = _pg().structures(n, PC.TYPES["ERDOS_RENYI"], 0, np.arange(G), 0, param=p)
    assert np.array_equal(C, C.transpose(0, 2, 1)) and not C[:, np.arange(n), np.arange(n)].any()
    iu, ju = np.tril_indices(n, -1)
    freq = C[:, iu, ju].mean(axis=0)
    worst = float(np.abs(freq - p).max() / math.sqrt(p * (1 - p) / G))
    law = np.array([math.comb(120, k) * p ** k * (1 - p) ** (120 - k) for k in range(121)]) * G
    lo = int(np.flatnonzero(np.cumsum(law) >= 5)[0])
    hi = int(120 - np.flatnonzero(np.cumsum(law[::-1]) >= 5)[0])
    counts = np.bincount(C[:, iu, ju].sum(axis=1), minlength=121).astype(np.float64)
    cells = lambda x: np.concatenate([[x[:lo + 1].sum()], x[lo + 1:hi], [x[hi:].sum()]])  # noqa: E731
    chi2, df = _chi2(cells(counts), cells(law)), len(cells(law)) - 1
    print(f"ER: worst pair {worst:.2f} sigma; edge counts chi-square {chi2:.2f} at {df} degrees of freedom (bound {Q999[df - 1]})")
    assert worst < 4.5 and chi2 < Q999[df - 1]


def test_caterpillar_and_lobster_attachments():
    PG, G, n = _pg(), 4000, 20
    # B drawn: a tree, one earlier neighbour per node; the node after a backbone of length 1 can only join node 0
    C, _ = PG.structures(n, PC.TYPES["CATERPILLAR"], 0, np.arange(G), 0)
    assert (np.tril(C, -1).sum(axis=2)[:, 1:] == 1).all() and C[:, 1, 0].all()
    # forced B: the path 0 .. B-1, every later node on a uniform backbone node
    B = 5
    C, _ = PG.structures(n, PC.TYPES["CATERPILLAR"], 1, np.arange(G), 0, param=B)
    par = np.tril(C, -1).argmax(axis=2)
    assert (np.tril(C, -1).sum(axis=2)[:, 1:] == 1).all()
    assert (par[:, 1:B] == np.arange(B - 1)).all() and par[:, B:].max() < B
    chi2 = _chi2(np.bincount(par[:, B:].reshape(-1), minlength=B), np.full(B, G * (n - B) / B))
    print(f"caterpillar targets: chi-square {chi2:.2f} (bound {Q999[B - 2]})")
    assert chi2 < Q999[B - 2]
    # lobster, forced B = 4: F - B is uniform on 1 .. n - B; [B, F) joins the backbone, [F, n) joins [B, F), both uniformly
    B = 4
    C, _ = PG.structures(n, PC.TYPES["LOBSTER"], 2, np.arange(G), 0, param=B)
    par = np.tril(C, -1).argmax(axis=2)
    assert (np.tril(C, -1).sum(axis=2)[:, 1:] == 1).all() and (par[:, 1:B] == np.arange(B - 1)).all()
    assert (par[:, B] < B).all()                                    # F >= B + 1
    F = np.array([next((i for i in range(B, n) if par[g, i] >= B), n) for g in range(G)])
    first, second = [], []
    for g in range(G):
        assert (par[g, B:F[g]] < B).all() and (par[g, F[g]:] >= B).all() and (par[g, F[g]:] < F[g]).all()
        first += par[g, B:F[g]].tolist()
        if F[g] - B == 4:
            second += (par[g, F[g]:] - B).tolist()
    # (F is read exactly: the first node that joins a pendant is F, and every node from F on joins one)
    chi2_f = _chi2(np.bincount(F - B - 1, minlength=n - B), np.full(n - B, G / (n - B)))
    chi2_1 = _chi2(np.bincount(first, minlength=B), np.full(B, len(first) / B))
    chi2_2 = _chi2(np.bincount(second, minlength=4), np.full(4, len(second) / 4))
    print(f"lobster: F chi-square {chi2_f:.2f} (bound {Q999[n - B - 2]}), first level {chi2_1:.2f} (bound {Q999[B - 2]}), "
          f"second level at F - B = 4 over {len(second)} draws {chi2_2:.2f} (bound {Q999[2]})")
    assert chi2_f < Q999[n - B - 2] and chi2_1 < Q999[B - 2] and len(second) > 1000 and chi2_2 < Q999[2]


def _triangular(x):
    """P(u + v < x) for u, v uniform on [0, 1/2)."""
    return 2 * x * x if x <= 0.5 else 1 - 2 * (1 - x) ** 2


def _randomize_law(t, n, param=None):
    """Unconditioned attempts, 4,000 graphs: the kept and the appeared fractions against the triangular law of the
    reference's sum of two uniforms - LINE (e = 19 <= r = 171): 0.98 and 2 (0.1 e / r)^2; CAVEMAN at a prime (complete, e = 78 >
    r = 0): an edge stays with P(value < 1) = 1 and nothing can appear.  Returns (e, r)."""
    PG, G = _pg(), 4000
    before, _ = PG.attempts(n, PC.TYPES[t], 0, np.arange(G), 0, randomize=False, param=param)
    after, _ = PG.attempts(n, PC.TYPES[t], 0, np.arange(G), 0, param=param)
    assert np.array_equal(after, after.transpose(0, 2, 1)) and not after[:, np.arange(n), np.arange(n)].any()
    iu, ju = np.tril_indices(n, -1)
    had, has = before[:, iu, ju], after[:, iu, ju]
    e = int(had[0].sum())
    r = iu.size - e
    assert (had.sum(axis=1) == e).all()
    ep, rp = (0.9, 0.1 * e / r) if e <= r else (0.9 + 0.1 * (e - r) / e, 0.1)
    for name, mask, prob in (("kept", had, _triangular(ep)), ("appeared", ~had, _triangular(rp))):
        trials = int(mask.sum())
        if trials == 0 or prob in (0.0, 1.0):
            assert (has[mask] == (prob == 1.0)).all() if trials else True
            print(f"{t}: {name} {trials} trials, probability {prob}: exact")
            continue
        frac = has[mask].mean()
        sigma = abs(frac - prob) / math.sqrt(prob * (1 - prob) / trials)
        print(f"{t}: {name} {frac:.5f} against {prob:.5f}, {sigma:.2f} sigma over {trials} trials")
        assert sigma < 4.5
    if t == "LINE":
        assert abs(_triangular(ep) - 0.98) < 1e-12
    return e, r


@pytest.mark.parametrize("t,n", (("LINE", 20), ("CAVEMAN", 13)))
def test_randomize_law(t, n):
    _randomize_law(t, n)


def test_randomize_law_with_more_edges_than_gaps():
    """The e > r branch where both of its comparisons decide something: BARABASI_ALBERT at n = 8 with m forced to 4 has
    e = 4 + 4 * 3 = 16 edges against r = 12 missing ones in every graph, so an edge stays with P(value < 0.9 + 0.1 * 4 / 16) =
    1 - 2 * 0.075^2 = 0.98875 and a missing one appears with P(value < 0.1) = 0.02."""
    assert _randomize_law("BARABASI_ALBERT", 8, param=4) == (16, 12)
    assert abs(_triangular(0.925) - 0.98875) < 1e-12 and abs(_triangular(0.1) - 0.02) < 1e-12


def test_mixture():
    counts = np.bincount(_pg().graph_type_of(0, np.arange(10000)), minlength=12)
    chi2 = _chi2([counts[PC.TYPES[t]] for t, _ in PC.MIXTURE], [10000 * share for _, share in PC.MIXTURE])
    print(f"mixture: chi-square {chi2:.2f} (bound 27.88)")
    assert counts[0] == counts[4] == 0 and counts.sum() == 10000 and chi2 < 27.88


def test_relabelling_is_uniform():
    inv = _pg().relabelling(3, 0, np.arange(6000), 0)
    assert (np.sort(inv, axis=1) == np.arange(3)).all()
    counts = np.bincount(inv[:, 0] * 3 + inv[:, 1], minlength=9)
    chi2 = _chi2(counts[counts > 0], np.full(6, 1000.0))
    print(f"relabelling: chi-square {chi2:.2f} (bound 20.52)")
    assert (counts > 0).sum() == 6 and chi2 < 20.52
    # the labels move with it: a LINE's middle node gets the rank of node 1's key
    A, _ = _pg().attempts(3, PC.TYPES["LINE"], 0, np.arange(50), 0, randomize=False)
    assert np.array_equal(A.sum(axis=2).argmax(axis=1), np.argsort(inv[:50], axis=1)[:, 1])


def test_star_acceptance_rate():
    """STAR at n = 24: a leaf keeps its edge with a = 0.98 and two leaves join with q = 2 (0.1 * 23 / 253)^2, so by inclusion
    and exclusion over the sets of isolated leaves P(accept) = sum_k (-1)^k C(23, k) (1 - a)^k (1 - q)^(C(k,2) + k (23 - k))
    (the centre is isolated with 0.02^23).  4,000 first attempts within 4.5 sigma; every graph that comes out has no singleton."""
    PG, G, n, L = _pg(), 4000, 24, 23
    a, q = 0.98, 2 * (0.1 * 23 / 253) ** 2
    law = sum((-1) ** k * math.comb(L, k) * (1 - a) ** k * (1 - q) ** (math.comb(k, 2) + k * (L - k)) for k in range(L + 1))
    A, _ = PG.attempts(n, PC.TYPES["STAR"], 0, np.arange(G), 0)
    rate = A.any(axis=2).all(axis=1).mean()
    sigma = abs(rate - law) / math.sqrt(law * (1 - law) / G)
    print(f"STAR acceptance: {rate:.4f} against {law:.4f}, {sigma:.2f} sigma")
    assert sigma < 4.5
    node_ptr, edge_ptr, ei, feat, source, types, attempts, status = PC.host((n,) * 200, 0, "STAR")
    assert (status == 0).all() and (types == 9).all() and attempts.min() == 1 and attempts.max() > 1
    assert abs(1 / attempts.mean() - law) < 4.5 * math.sqrt(law * (1 - law) / attempts.sum())
    for g in range(200):
        A = PC.adjacency(n, ei[:, edge_ptr[g]:edge_ptr[g + 1]])
        assert A.any(axis=0).all() and np.array_equal(A, A.T) and not A.diagonal().any()
        assert 0 <= source[g] < n
    assert feat.dtype == np.float32 and (feat >= 0).all() and (feat < 1).all()


def test_a_graph_depends_on_its_seed_and_id_alone():
    sizes = tuple(range(15, 25)) * 3
    whole = PC.host(sizes)
    a, b = PC.host(sizes[:11]), PC.host(sizes[11:], first_graph=11)
    assert np.array_equal(whole[2], np.concatenate([a[2], b[2]], axis=1))
    for k in (3, 4, 5, 6, 7):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]]))
    assert np.array_equal(whole[1], np.concatenate([a[1], a[1][-1] + b[1][1:]]))
    other = PC.host(sizes, seed=1)
    assert not np.array_equal(whole[3], other[3]) and (whole[5] != other[5]).any()
    assert sum(np.array_equal(whole[3][whole[0][g]:whole[0][g + 1]], other[3][other[0][g]:other[0][g + 1]]) for g in range(30)) == 0


def test_exhausted_graphs_are_named():
    from kp_gnn_amd import ops
    out = PC.host((4,) * 400, 0, "ERDOS_RENYI", max_attempts=1)
    status, edge_ptr = out[7], out[1]
    assert 0 < (status != 0).sum() < 400 and set(status.tolist()) == {0, 1} and (out[6] == 1).all()
    assert (np.diff(edge_ptr)[status != 0] == 0).all() and (np.diff(edge_ptr)[status == 0] > 0).all()
    want = np.array([PC.one_graph(4, "ERDOS_RENYI", 0, g, max_attempts=1)[5] for g in range(400)])
    assert np.array_equal(status, want)
    r = ops.property_graphs([4] * 400, 0, "cpu", graph_type="ERDOS_RENYI", max_attempts=1)
    assert r.route == "host" and np.array_equal(r.exhausted, np.flatnonzero(status)) and np.array_equal(r.edge_index.numpy(), out[2])


def test_arguments_and_routing():
    from kp_gnn_amd import graph_property as GP, ops
    for nodes in (1, 129, [15, 1], [129, 20], 0, -3):
        with pytest.raises(ValueError):
            _pg().property_graphs_host(nodes, 0, "RANDOM")
        for route in ("auto", "device", "host"):
            with pytest.raises(ValueError):
                ops.property_graphs(nodes, 0, "cpu", route=route)
    for bad in (dict(route="networkx"), dict(graph_type="WHEEL"), dict(graph_type=4), dict(max_attempts=0), dict(first_graph=-1)):
        with pytest.raises(ValueError):
            ops.property_graphs(5, 0, "cpu", **bad)
    with pytest.raises(ops._lib.KpgnnError):
        ops.property_graphs(5, 0, "cpu", route="device")
    r = ops.property_graphs(7, 3, "cpu", graph_type="LINE", randomize=False, shuffle=False)
    assert r.route == "host" and r.node_ptr.tolist() == [0, 7] and r.edge_ptr.tolist() == [0, 12] and r.exhausted.size == 0
    assert r.edge_index.tolist() == [sorted([i for i in range(7) for _ in range((i > 0) + (i < 6))]),
                                     [j for i in range(7) for j in (i - 1, i + 1) if 0 <= j < 7]]
    r = ops.property_graphs([], 0, "cpu")
    assert r.node_ptr.tolist() == [0] and tuple(r.edge_index.shape) == (2, 0)
    assert GP.generate_split([5, 9], 0, "cpu", graph_type="STAR").y.shape == (2, 3)


def test_reference_splits():
    from kp_gnn_amd import graph_property as GP
    s = GP.reference_splits()
    assert list(s) == ["train", "val", "test"] and [v.size for v in s.values()] == [5120, 640, 1280]
    assert s["train"].tolist() == [n for n in range(15, 25) for _ in range(512)] and sorted(set(s["val"].tolist())) == list(range(15, 20))
    x = GP.reference_splits(extrapolation=True)
    assert len(x) == 11 and sum(k.startswith("test-") for k in x) == 9 and all(x[k].size == 1280 for k in x if k.startswith("test-"))
    assert sorted(set(x["test-(95,100)"].tolist())) == [95, 96, 97, 98, 99] and max(v.max() for v in x.values()) == 99


def test_generate_split_on_the_host():
    from kp_gnn_amd import graph_property as GP
    sizes = [15, 16, 24, 17]
    s = GP.generate_split(sizes, 5, "cpu", first_graph=2)
    g = PC.host(tuple(sizes), 5, first_graph=2)
    assert np.array_equal(s.node_ptr, g[0]) and np.array_equal(s.edge_ptr, g[1]) and np.array_equal(s.edge_index.numpy(), g[2])
    assert tuple(s.x.shape) == (72, 2) and tuple(s.pos.shape) == (72, 3) and tuple(s.y.shape) == (4, 3)
    assert np.array_equal(s.x[:, 1].numpy(), g[3]) and s.x[:, 0].sum() == 4 and (s.x[g[0][:-1] + g[4], 0] == 1).all()
    want = GP.graph_property_labels_host(g[0], g[1], g[2], g[3], g[4])
    assert np.array_equal(s.pos.numpy(), want[0].numpy()) and np.array_equal(s.y.numpy(), want[1].numpy())
    assert (s.pos[g[0][:-1] + g[4], 0] == 0).all()                  # the source is at distance 0 from itself


@pytest.mark.parametrize("t", tuple(PC.TYPES))
def test_the_numpy_route_follows_the_definition(t):
    """Graph by graph against the plain-integer definition: adjacency, features, source, type, attempts and status."""
    sizes = PC.DEFINITION_SIZES
    node_ptr, edge_ptr, ei, feat, source, types, attempts, status = PC.host(sizes, 3, t, first_graph=2 ** 33 + 1)
    for g, n in enumerate(sizes):
        A, f, s, ty, a, st = PC.one_graph(n, t, 3, 2 ** 33 + 1 + g)
        assert (types[g], attempts[g], status[g], source[g]) == (ty, a, st, s), (t, n)
        assert np.array_equal(PC.adjacency(n, ei[:, edge_ptr[g]:edge_ptr[g + 1]]), A), (t, n)
        assert np.array_equal(feat[node_ptr[g]:node_ptr[g + 1]], f), (t, n)


@pytest.mark.parametrize("t", ("TREE", "ERDOS_RENYI", "LOBSTER"))
def test_the_flags_follow_the_definition(t):
    for n in (3, 15):
        for randomize, shuffle in ((False, False), (True, False), (False, True)):
            out = PC.host((n,) * 2, -5, t, max_attempts=64, randomize=randomize, shuffle=shuffle)
            for g in range(2):
                A, f, s, ty, a, st = PC.one_graph(n, t, -5 & (2 ** 64 - 1), g, 64, randomize, shuffle)
                assert (out[6][g], out[7][g], out[4][g]) == (a, st, s)
                if st == 0:
                    assert np.array_equal(PC.adjacency(n, out[2][:, out[1][g]:out[1][g + 1]]), A)
