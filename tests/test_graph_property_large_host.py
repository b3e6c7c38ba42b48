"""CPU: what lets the device serve the graph-property labels of graphs of 65 to 128 nodes (csrc/graph_labels.hip, W = 2).
1. The overflow argument as a test: for 65 <= n <= 128 the reference squares m = 8 times, no entry is inf when the last
   squaring begins, so it forms no inf * 0 and its min > 0 is "the eighth boolean squaring has no zero" - on 145 graphs,
   dense ones included (K128 overflows to inf, which is > 0).
2. tests/golden/graph_property_large.npz: what the reference's own datasets/graph_algorithms.py answers for 17 sparse graphs of
   65 to 128 nodes, and the float64 host route - the yardstick of the GPU tests - against it."""
import functools
import math
import os

import numpy as np

import graph_property_cases as GC
import graph_property_large_cases as GL
from test_graph_property_host import check_case


@functools.lru_cache(maxsize=None)
def golden_large():
    z = np.load(GL.GOLDEN)
    out = {}
    for name in z["names"].tolist():
        out[name] = {k: z[f"{name}/{k}"] for k in ("n", "F", "source", "node", "graph")}
        out[name]["ei"] = z[f"{name}/ei"].astype(np.int64)
    return out


def items_of(g, names):
    return [(int(g[k]["n"]), g[k]["ei"], g[k]["F"], int(g[k]["source"])) for k in names]


def boolean_squarings(n, ei, m):
    """Every ordered pair has a walk of length exactly 2^m: m squarings of the boolean adjacency (float32 sums of at most 128
    zeros and ones are exact)."""
    B = np.zeros((n, n), dtype=bool)
    B[ei[0], ei[1]] = True
    for _ in range(m):
        Bf = B.astype(np.float32)
        B = Bf @ Bf > 0
    return float(B.all())


def test_the_overflow_argument_on_145_graphs():
    from kp_gnn_amd import graph_property as GP
    cases = GL.argument_cases()
    assert {"complete128", "gnp128_0.95_0", "gnp128_0.95_1", "k60_p5", "k123_p5"} <= set(cases)
    answers = []
    for name, (n, ei) in cases.items():
        assert 64 < n <= 128 and int(1 + math.ceil(math.log2(n))) == 8, name
        _, graph = GP.labels_one(n, ei, np.ones(n), 0)                  # the literal float64 squaring, overflow included
        want = boolean_squarings(n, ei, 8)
        assert graph[0] == want, f"{name}: literal {graph[0]} boolean {want}"
        answers.append(want)
    # both answers occur, and the dense graphs are on the True side: inf > 0
    _, k128 = GP.labels_one(128, cases["complete128"][1], np.ones(128), 0)
    assert k128[0] == 1.0 and 20 < sum(answers) < 125
    for n in GL.ARGUMENT_SIZES:
        assert boolean_squarings(n, cases[f"path{n}"][1], 8) == 0.0 and boolean_squarings(n, cases[f"k{n - 5}_p5"][1], 8) == 0.0


def test_fixture_has_the_cases():
    g = golden_large()
    assert list(GL.fixture_cases()) == list(g) and len(g) == 17
    sizes = {int(c["n"]) for c in g.values()}
    assert {65, 66, 96, 100, 127, 128} <= sizes and min(sizes) == 65 and max(sizes) == 128
    for k, (n, ei, F, s) in GC.inputs(GL.fixture_cases(), seed=29).items():        # the fixture is what the cases module draws
        assert n == int(g[k]["n"]) and s == int(g[k]["source"]) and np.array_equal(ei, g[k]["ei"]) and np.array_equal(F, g[k]["F"])
        assert ei.shape[1] <= 0.12 * n * (n - 1), k                                # none dense
    # the reference's rule is not connectivity: bipartite graphs answer False, so do two components and an isolated node
    for k in ("path65", "path128", "cycle66", "star100", "ladder128", "grid10x10", "caterpillar96", "iso_last65", "c63_c65"):
        assert g[k]["graph"][0] == 0.0, k
    for k in ("cycle127", "lollipop100"):
        assert g[k]["graph"][0] == 1.0, k
    assert g["path128"]["graph"][1] == 127.0 and g["cycle127"]["graph"][1] == 63.0 and g["iso_last65"]["graph"][1] == 32.0
    assert os.path.getsize(GL.GOLDEN) <= os.path.getsize(GC.GOLDEN)


def test_host_route_against_the_reference_at_65_to_128_nodes():
    from kp_gnn_amd import graph_property as GP
    g = golden_large()
    names = list(g)
    nptr, eptr, ei, F, src = GC.pack(items_of(g, names))
    node, graph = GP.labels_host_f64(nptr, eptr, ei, F, src)
    for i, k in enumerate(names):
        check_case(k, node[nptr[i]:nptr[i + 1]].astype(np.float32), graph[i].astype(np.float32), g[k])
        assert graph[i, 0] == boolean_squarings(int(g[k]["n"]), g[k]["ei"], 8), k
