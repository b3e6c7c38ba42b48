"""Shared by the property-graph tests: the shapes; the host route's answers, computed once per case and left read-only; and
the definition of include/kpgnn.h (kpgnn_property_graphs_generate) once more, in plain Python integers - one Philox call at a
time, sets of edges, sorted() - so that the tests own a graph they did not get from the code under test."""
import functools

import numpy as np

from regular_graph_cases import philox4x32_10

TYPES = {"RANDOM": 0, "ERDOS_RENYI": 1, "BARABASI_ALBERT": 2, "GRID": 3, "CAVEMAN": 5, "TREE": 6, "LADDER": 7, "LINE": 8,
         "STAR": 9, "CATERPILLAR": 10, "LOBSTER": 11}
FIXED = ("GRID", "CAVEMAN", "LADDER", "LINE", "STAR")
STREAMS = {"TYPE": 0, "PARAM": 1, "PAIR": 2, "BA": 3, "TREE": 4, "ATTACH": 5, "SHUFFLE": 6, "FEATURE": 7, "SOURCE": 8}
MIXTURE = (("ERDOS_RENYI", .2), ("BARABASI_ALBERT", .2), ("GRID", .05), ("CAVEMAN", .05), ("TREE", .15), ("LADDER", .05),
           ("LINE", .05), ("STAR", .05), ("CATERPILLAR", .1), ("LOBSTER", .1))
TREE_SWAPS = 5000
# the kernel's paths: the smallest graphs, a wavefront's half and whole (32 | 33, 64), the block class (65) and the limit
DEVICE_SIZES = (2, 3, 15, 32, 33, 64, 65, 128)
DEFINITION_SIZES = (2, 3, 15, 64, 65, 128)
FIXED_SIZES = tuple(range(2, 41)) + (49, 64, 97, 99, 100, 127, 128)


@functools.lru_cache(maxsize=None)
def host(nodes, seed=0, graph_type="RANDOM", first_graph=0, max_attempts=4096, randomize=True, shuffle=True):
    """property_graphs_host(...) for a tuple of node counts, every array read-only."""
    from kp_gnn_amd.property_graphs import property_graphs_host
    out = property_graphs_host(list(nodes), seed, graph_type, first_graph, max_attempts, randomize, shuffle)
    for a in out:
        a.setflags(write=False)
    return out


def rows_of(node_ptr, edge_ptr, edge_index):
    """[N, 2] uint64: the adjacency rows of raw graphs, bit v & 63 of word v >> 6."""
    rows = np.zeros((int(node_ptr[-1]), 2), dtype=np.uint64)
    for g in range(len(node_ptr) - 1):
        src, dst = edge_index[:, edge_ptr[g]:edge_ptr[g + 1]]
        np.bitwise_or.at(rows, (node_ptr[g] + src, dst >> 6), np.uint64(1) << (dst & 63).astype(np.uint64))
    return rows


def adjacency(n, edge_index):
    A = np.zeros((n, n), dtype=bool)
    A[edge_index[0], edge_index[1]] = True
    return A


def chi2_two_samples(a, b):
    """Pearson's statistic of two histograms of equal totals over the cells either fills, and its degrees of freedom."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    keep = (a + b) > 0
    return float((((a - b) ** 2)[keep] / (a + b)[keep]).sum()), int(keep.sum()) - 1


# ------------------------------------------------------------------------------------------------ the definition, in integers
def W(stream, seed, gid, a, i):
    return philox4x32_10((i, (a << 4) | STREAMS[stream], gid & 0xFFFFFFFF, gid >> 32), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def below(w, L):
    return (w * L) >> 32


def degree(v, n):
    k = 1
    while k < n and not v * (2 * k + 1) ** 2 < (1 << 32) * ((2 * k + 1) ** 2 - 4):
        k += 1
    return k


def degree_law(k):
    """P(degree = k) without the clamp."""
    return 5 / 9 if k == 1 else 4 / (2 * k - 1) ** 2 - 4 / (2 * k + 1) ** 2


def pick_type(seed, gid):
    x = below(W("TYPE", seed, gid, 0, 0)[0], 20)
    total = 0
    for name, share in MIXTURE:
        total += round(share * 20)
        if x < total:
            return name


def divisor(n):
    return max(i for i in range(1, n + 1) if i * i <= n and n % i == 0)


def canonical(n, t, seed, gid, a):
    """The set of edges (i, j), i > j, of the structure of attempt a on canonical labels; None for a rejected TREE."""
    E = set()
    if t == "ERDOS_RENYI":
        p = W("PARAM", seed, gid, a, 0)[0]
        E = {(i, j) for i in range(n) for j in range(i) if W("PAIR", seed, gid, a, i * (i - 1) // 2 + j)[2] < p}
    elif t == "BARABASI_ALBERT":
        m = 1 + below(W("PARAM", seed, gid, a, 0)[0], n - 1)
        E = {(s, 0) for s in range(1, m + 1)}
        rep, tick = [0] * m + list(range(1, m + 1)), 0
        for s in range(m + 1, n):
            targets = set()
            while len(targets) < m:
                targets.add(rep[below(W("BA", seed, gid, a, tick)[0], len(rep))])
                tick += 1
            E |= {(s, x) for x in targets}
            rep += sorted(targets) + [s] * m
    elif t == "GRID":
        r = divisor(n)
        c = n // r
        E = {(i * c + j + 1, i * c + j) for i in range(r) for j in range(c - 1)} | {((i + 1) * c + j, i * c + j) for i in range(r - 1) for j in range(c)}
    elif t == "CAVEMAN":
        k = n // divisor(n)
        E = {(i, j) for i in range(n) for j in range(i) if i // k == j // k}
    elif t == "LADDER":
        h = n // 2
        E = {(i + 1, i) for i in range(h - 1)} | {(h + i + 1, h + i) for i in range(h - 1)} | {(i + h, i) for i in range(h)}
        if n % 2:
            E.add((n - 1, 0))
    elif t == "LINE":
        E = {(i, i - 1) for i in range(1, n)}
    elif t == "STAR":
        E = {(i, 0) for i in range(1, n)}
    elif t == "TREE":
        deg = [degree(W("TREE", seed, gid, a, i)[0], n) for i in range(n)]
        s = 0
        while sum(deg) != 2 * n - 2:
            if s == TREE_SWAPS:
                return None
            deg[below(W("TREE", seed, gid, a, n + 2 * s)[0], n)] = degree(W("TREE", seed, gid, a, n + 2 * s + 1)[0], n)
            s += 1
        inner = sorted(d for d in deg if d > 1)
        nb = len(inner) + 2
        E, nxt = {(i, i - 1) for i in range(1, nb)}, nb
        for b, d in enumerate(inner, start=1):
            E |= {(leaf, b) for leaf in range(nxt, nxt + d - 2)}
            nxt += d - 2
        assert nxt == n
    else:
        B = 1 + below(W("PARAM", seed, gid, a, 0)[0], n - 1)
        F = B + 1 + below(W("PARAM", seed, gid, a, 1)[0], n - B) if t == "LOBSTER" else n
        E = {(i, i - 1) for i in range(1, B)}
        E |= {(i, below(W("ATTACH", seed, gid, a, i)[0], B)) for i in range(B, F)}
        E |= {(i, B + below(W("ATTACH", seed, gid, a, i)[0], F - B)) for i in range(F, n)}
    return E


def one_attempt(n, t, seed, gid, a, randomize=True, shuffle=True):
    """The adjacency [n, n] bool attempt a ends with; None for a rejected TREE."""
    E = canonical(n, t, seed, gid, a)
    if E is None:
        return None
    label = list(range(n))
    if shuffle:
        keys = []
        for i in range(n):
            w = W("SHUFFLE", seed, gid, a, i)
            keys.append((((w[1] << 32) | w[0]) & ~127) | i)
        for rank, key in enumerate(sorted(keys)):
            label[key & 127] = rank
    E = {(max(label[i], label[j]), min(label[i], label[j])) for i, j in E}
    if randomize:
        e = len(E)
        r = n * (n - 1) // 2 - e
        out = set()
        for u in range(n):
            for v in range(u):
                w = W("PAIR", seed, gid, a, u * (u - 1) // 2 + v)
                t2 = w[0] + w[1]
                if e <= r:
                    keep = 10 * t2 < 9 * 2 ** 33 if (u, v) in E else 10 * t2 * r < e * 2 ** 33
                else:
                    keep = 10 * t2 * e < (10 * e - r) * 2 ** 33 if (u, v) in E else 10 * t2 < 2 ** 33
                if keep:
                    out.add((u, v))
        E = out
    A = np.zeros((n, n), dtype=bool)
    for u, v in E:
        A[u, v] = A[v, u] = True
    return A


def one_graph(n, graph_type, seed, gid, max_attempts=4096, randomize=True, shuffle=True):
    """(adjacency or None, features, source, type id, attempts, status) of graph gid."""
    t = pick_type(seed, gid) if graph_type == "RANDOM" else graph_type
    for a in range(max_attempts):
        A = one_attempt(n, t, seed, gid, a, randomize, shuffle)
        if A is not None and A.any(axis=0).all():
            feat = np.array([(W("FEATURE", seed, gid, a, i)[0] >> 8) / 2 ** 24 for i in range(n)], dtype=np.float32)
            return A, feat, below(W("SOURCE", seed, gid, a, 0)[0], n), TYPES[t], a + 1, 0
    return None, np.zeros(n, dtype=np.float32), 0, TYPES[t], max_attempts, 1
