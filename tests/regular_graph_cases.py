"""Shared by the random-regular-graph tests: the host route's answers, computed once per case and left read-only; the checks
of what a list of d-regular graphs must look like; and the definition of include/kpgnn.h (kpgnn_random_regular_graphs) once
more, in plain Python integers - one Philox call at a time, sorted() - so that the tests own a pairing they did not get from
the code under test."""
import functools

import numpy as np

# (n, d): both sides of every power-of-two padding step of the key count m = n * d (2 .. 8192), of the wavefront / block bound
# (m = 256 | 258) and of the block sizes (256 threads up to P = 512, 512 at 1024, 1024 from 2048 on: 1, 2 and 4 exchanges a
# thread), the forced answers K4 and K5, the issue's (20,3), (64,3), (65,4), (1280,3), and the limit (2048,4).
BOUND_SHAPES = ((2, 1), (4, 1), (3, 2), (4, 2), (5, 2), (8, 2), (6, 3), (8, 4), (17, 2), (16, 4), (22, 3), (32, 4), (65, 2),
                (64, 4), (86, 3), (128, 4), (257, 2), (256, 4), (342, 3), (512, 4), (1025, 2), (1024, 4), (1366, 3))
NAMED_SHAPES = ((4, 3), (5, 4), (20, 3), (64, 3), (65, 4))


def device_cases():
    """(n, d, G): G = 1 and a G that leaves the last four-graph block of the wavefront class partly filled (6), 3 for the block class."""
    cases = []
    for n, d in BOUND_SHAPES + NAMED_SHAPES:
        cases += [(n, d, 1), (n, d, 6)] if n * d <= 256 else [(n, d, 3)]
    return cases + [(1280, 3, 3), (2048, 4, 2), (2048, 4, 1)]


@functools.lru_cache(maxsize=None)
def host(G, n, d, seed=0, first_graph=0, max_attempts=4096):
    """random_regular_graphs_host(...), every array read-only."""
    from kp_gnn_amd.regular_graphs import random_regular_graphs_host
    out = random_regular_graphs_host(G, n, d, seed, first_graph=first_graph, max_attempts=max_attempts)
    for a in out:
        a.setflags(write=False)
    return out


def check_structure(node_ptr, edge_ptr, ei, G, n, d):
    """G simple d-regular graphs on n nodes each, as (src, dst)-sorted directed lists with arithmetic pointers."""
    m = n * d
    assert np.array_equal(node_ptr, np.arange(G + 1) * n) and np.array_equal(edge_ptr, np.arange(G + 1) * m)
    assert node_ptr.dtype == np.int64 and edge_ptr.dtype == np.int64
    ei = np.asarray(ei)
    assert ei.shape == (2, G * m) and ei.dtype == np.int64
    for g in range(G):
        src, dst = ei[0, g * m:(g + 1) * m], ei[1, g * m:(g + 1) * m]
        assert np.array_equal(src, np.repeat(np.arange(n), d)), g            # every node has exactly d edges, grouped by src
        assert dst.min() >= 0 and dst.max() < n and not (src == dst).any(), g
        rows = dst.reshape(n, d)
        assert (np.diff(rows, axis=1) > 0).all(), g                          # ascending and distinct within a node
        code = src * n + dst
        assert np.array_equal(np.sort(code), np.sort(dst * n + src)), g      # (u, v) iff (v, u)


# ------------------------------------------------------------------------------------------------ the definition, in integers
def philox4x32_10(c, k):
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def pairing(n, d, seed, graph_id, attempt):
    """[(stub, stub)]: the pairing number `attempt` of graph `graph_id`."""
    keys = []
    for s in range(n * d):
        w = philox4x32_10((s >> 1, attempt, graph_id & 0xFFFFFFFF, graph_id >> 32), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
        r = w[2 * (s & 1)] | (w[2 * (s & 1) + 1] << 32)
        keys.append((r & ~0x1FFF) | s)
    order = [k & 0x1FFF for k in sorted(keys)]
    return list(zip(order[0::2], order[1::2]))


def simple(pairs, d):
    """Whether the pairing is a simple graph: no self loop, no edge twice."""
    edges = [tuple(sorted((a // d, b // d))) for a, b in pairs]
    return all(u != v for u, v in edges) and len(set(edges)) == len(edges)


def graph_of(pairs, n, d):
    """The [2, n d] directed (src, dst)-sorted list of an accepted pairing."""
    edges = sorted([(a // d, b // d) for a, b in pairs] + [(b // d, a // d) for a, b in pairs])
    return np.array(edges, dtype=np.int64).T
