"""Graphs of the graph-property label tests (test_graph_property*.py, golden/make_graph_property_golden.py): the 53 cases the
device kernel serves, three above its cap for the host route, the edge sizes, and the helpers both test files share."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_property.npz")
EDGE_SIZES = (1, 2, 3, 31, 32, 33, 63, 64)


def sym(n, pairs):
    """(n, edge_index [2,2e] int64): both directions of the undirected pairs, sorted by (source, target)."""
    p = np.asarray(sorted(set((int(a), int(b)) for a, b in pairs) | set((int(b), int(a)) for a, b in pairs)), dtype=np.int64)
    return n, (p.T.copy() if p.size else np.zeros((2, 0), dtype=np.int64))


def path(n, off=0):
    return [(off + i, off + i + 1) for i in range(n - 1)]


def cycle(n, off=0):
    return path(n, off) + ([(off + n - 1, off)] if n > 2 else [])


def complete(n, off=0):
    return [(off + i, off + j) for i in range(n) for j in range(i + 1, n)]


def gnp(n, p, rng):
    return [(i, j) for i in range(n) for j in range(i + 1, n) if rng.random() < p]


def served_cases():
    """name -> (n, edge_index): the 53 graphs of at most 64 nodes."""
    c = {}
    c["path2"], c["path64"] = sym(2, path(2)), sym(64, path(64))
    c["cycle63"], c["cycle64"] = sym(63, cycle(63)), sym(64, cycle(64))
    c["star64"] = sym(64, [(0, i) for i in range(1, 64)])
    c["k64"] = sym(64, complete(64))
    c["k32_32"] = sym(64, [(i, 32 + j) for i in range(32) for j in range(32)])
    c["c5_p7"] = sym(12, cycle(5) + path(7, 5))
    c["grid8x8"] = sym(64, [(r * 8 + q, r * 8 + q + 1) for r in range(8) for q in range(7)]
                       + [(r * 8 + q, r * 8 + q + 8) for r in range(7) for q in range(8)])
    c["k3_iso2"] = sym(5, complete(3))
    c["petersen"] = sym(10, cycle(5) + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)])
    c["ladder32"] = sym(32, path(16) + path(16, 16) + [(i, i + 16) for i in range(16)])
    c["iso5"] = sym(5, [])
    rng = np.random.default_rng(20240607)
    ns = [3, 4, 64] + [int(v) for v in rng.integers(5, 64, size=7)]
    for p in (0.05, 0.1, 0.2, 0.5):
        for n in ns:
            c[f"gnp{n}_{p}"] = sym(n, gnp(n, p, rng))
    assert len(c) == 53
    return c


def host_cases():
    """Three graphs above the kernel's cap: K60 + P5 (the float64 squaring overflows next to exact zeros), a sparse G(80, p)
    and a dense G(100, p) (it overflows everywhere)."""
    rng = np.random.default_rng(977)
    return {"k60_p5": sym(65, complete(60) + path(5, 60)), "gnp80": sym(80, gnp(80, 0.05, rng)), "gnp100": sym(100, gnp(100, 0.9, rng))}


def inputs(cases, seed=11):
    """name -> (n, edge_index, F [n] float64, source): the features and the source node of each case, drawn once per name."""
    rng = np.random.default_rng(seed)
    return {k: (n, ei, rng.random(n), int(rng.integers(0, n))) for k, (n, ei) in cases.items()}


def edge_size_cases():
    """Each edge size as a path, a complete graph and a graph with one isolated node (a cycle or path on the others)."""
    c = {}
    for n in EDGE_SIZES:
        c[f"path{n}"] = sym(n, path(n))
        c[f"complete{n}"] = sym(n, complete(n))
        c[f"isolated{n}"] = sym(n, cycle(n - 1))
    return c


def pack(items):
    """[(n, edge_index, F, source)] -> (node_ptr, edge_ptr, edge_index [2,E], features [N], source [G]) of one call."""
    node_ptr = np.concatenate([[0], np.cumsum([it[0] for it in items])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([it[1].shape[1] for it in items])]).astype(np.int64)
    ei = np.concatenate([it[1] for it in items], axis=1) if items else np.zeros((2, 0), np.int64)
    F = np.concatenate([it[2] for it in items]) if items else np.zeros(0)
    return node_ptr, edge_ptr, ei, F, np.asarray([it[3] for it in items], dtype=np.int64)


def f32_ulps(a, b):
    """Distance in float32 ulps between the float32 roundings of a and b (finite, same sign or zero)."""
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def laplacian_bound(n, ei, F, ref64):
    """|got - ref64| <= 2^-24 |ref64| + (deg + 1) 2^-53 (deg |F_i| + sum_j |F_j|): one float32 rounding, plus the float64
    accumulation error of a (deg + 1)-term sum, which differs between summation orders."""
    A = np.zeros((n, n))
    A[ei[0], ei[1]] = 1.0
    deg = A.sum(1)
    return 2.0 ** -24 * np.abs(ref64) + (deg + 1) * 2.0 ** -53 * (deg * np.abs(F) + A @ np.abs(F))
