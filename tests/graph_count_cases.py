"""Graphs of the substructure-count label tests (test_graph_count*.py, golden/make_graph_count_golden.py): the cases the
one-word classes of the kernel serve (n <= 64), those of its large class (65 .. 2048), three for the host route, and the
helpers the test files share."""
import os

import numpy as np

from graph_property_cases import EDGE_SIZES, complete, cycle, gnp, path, served_cases, sym

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_count.npz")
LARGE_SIZES = (65, 127, 128, 129, 192, 193)
INT_COLS = slice(0, 4)              # tri, tailed, star, cyc4: exact integers; column 4 is cus


def circulant3(n):
    """i - i+1 and, for even n, i - i + n/2 (3-regular); for odd n, i - i+1 and i - i+2 (4-regular)."""
    pairs = [(i, (i + 1) % n) for i in range(n)]
    return pairs + ([(i, i + n // 2) for i in range(n // 2)] if n % 2 == 0 else [(i, (i + 2) % n) for i in range(n)])


def word_cases():
    """name -> (n, edge_index): the 53 served graphs of graph_property_cases and each edge size as a path, a complete graph
    and a cycle plus one isolated node."""
    c = dict(served_cases())
    for n in EDGE_SIZES:
        c[f"e_path{n}"] = sym(n, path(n))
        c[f"e_complete{n}"] = sym(n, complete(n))
        c[f"e_isolated{n}"] = sym(n, cycle(n - 1))
    assert len(c) == 53 + 3 * len(EDGE_SIZES)
    return c


def large_cases():
    c = {}
    for n in LARGE_SIZES:
        c[f"path{n}"] = sym(n, path(n))
        c[f"cycle{n}"] = sym(n, cycle(n))
        c[f"complete{n}"] = sym(n, complete(n))
    c["k100_100"] = sym(200, [(i, 100 + j) for i in range(100) for j in range(100)])
    rng = np.random.default_rng(431)
    c["gnp300_0.5"] = sym(300, gnp(300, 0.5, rng))
    c["gnp640_0.02"] = sym(640, gnp(640, 0.02, rng))
    c["circulant2047"] = sym(2047, circulant3(2047))
    c["circulant2048"] = sym(2048, circulant3(2048))
    return c


def host_cases():
    """Above the cap, a directed list, a self loop: the three reasons for the host route (not symmetrised: raw edge lists)."""
    tri = np.asarray([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
    loop = np.asarray([[0, 1, 1, 2, 0, 2, 1], [1, 0, 2, 1, 2, 0, 1]], dtype=np.int64)
    return {"path2049": sym(2049, path(2049)), "directed_c3": (3, tri), "triangle_loop": (3, loop)}


def groups():
    return (("word", word_cases()), ("large", large_cases()), ("host", host_cases()))


def pack(items):
    """[(n, edge_index)] -> (node_ptr, edge_ptr, edge_index [2,E]) of one call."""
    node_ptr = np.concatenate([[0], np.cumsum([it[0] for it in items])]).astype(np.int64)
    edge_ptr = np.concatenate([[0], np.cumsum([it[1].shape[1] for it in items])]).astype(np.int64)
    ei = np.concatenate([it[1] for it in items], axis=1) if items else np.zeros((2, 0), np.int64)
    return node_ptr, edge_ptr, ei


def cus_bound(n, ref):
    """|got - ref| <= (n + 8) 2^-52 |ref| + n 2^-1022: one rounding per exp on either side (<= 1 ulp each), one per product,
    n - 1 per summation in either order, all terms non-negative; the absolute floor covers terms that underflow."""
    return (n + 8) * 2.0 ** -52 * abs(float(ref)) + n * 2.0 ** -1022


def check_row(name, n, got, want):
    """got [5] float64 against the reference's row: the integer columns equal, cus within cus_bound.  Prints before it asserts."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err, bound = abs(got[4] - want[4]), cus_bound(n, want[4])
    print(f"{name}: n {n} ints {got[INT_COLS].tolist()} cus {got[4]!r} want {want[4]!r} err {err:.3e} bound {bound:.3e}")
    assert got.shape == (5,) and (got[INT_COLS] == want[INT_COLS]).all(), f"{name}: {got[INT_COLS]} vs {want[INT_COLS]}"
    assert err <= bound, f"{name}: cus {got[4]!r} vs {want[4]!r}"


def reduced_form(n, ei):
    """The integer form the kernel uses, in Python integers / float64, for a symmetric graph without loops."""
    A = np.zeros((n, n), dtype=np.int64)
    if n:
        A[ei[0], ei[1]] = 1
    d = A.sum(1)
    C = (A.astype(np.float64) @ A.astype(np.float64)).astype(np.int64)      # (exact: entries below 2^53; BLAS, not an integer loop)
    T = (A * C).sum(1)
    s = A @ d
    cus = 0.0
    for k in range(n):
        cus += float(d[k] * d[k]) * float(np.exp(-float(s[k])))
    return np.asarray([int(T.sum()) // 6, int(((T // 2) * (d - 2)).sum()), int((d * (d - 1) * (d - 2) // 6).sum()),
                       (int((C * C).sum()) + int(d.sum()) - 2 * int((d * d).sum())) // 8, cus], dtype=np.float64)
