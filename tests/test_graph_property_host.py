"""CPU: the float64 host route of the graph-property labels (kp_gnn_amd/graph_property.py) against what the reference's
datasets/graph_algorithms.py recorded in tests/golden/graph_property.npz (53 graphs of at most 64 nodes, three above, one of
which overflows the reference's float64 squaring next to exact zeros), and normalize_labels / source_features against a direct
torch restatement of GraphPropertyDataset.process / GenerateGraphPropertyDataset."""
import functools

import numpy as np
import pytest
import torch

import graph_property_cases as GC


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GC.GOLDEN)
    out = {}
    for group in ("served", "host"):
        for name in z[group + "/names"].tolist():
            out[name] = {k: z[f"{name}/{k}"] for k in ("n", "ei", "F", "source", "node", "graph")}
            out[name]["group"] = group
    return out


def check_case(name, got_node, got_graph, c, spectral_ref=None):
    """got_* float32 rows of one graph against the fixture case c: the four integer labels exact, the spectral radius within
    one float32 ulp (of spectral_ref when given, else of the fixture) after rounding both, the laplacian within its bound."""
    n, ei, F = int(c["n"]), c["ei"], c["F"]
    got_node, got_graph = np.asarray(got_node), np.asarray(got_graph)
    assert got_node.dtype == np.float32 and got_graph.dtype == np.float32 and got_node.shape == (n, 3), name
    assert (got_node[:, :2] == c["node"][:, :2].astype(np.float32)).all(), f"{name}: sssp / eccentricity"
    assert (got_graph[:2] == c["graph"][:2].astype(np.float32)).all(), f"{name}: is_connected / diameter {got_graph} {c['graph']}"
    want = c["graph"][2] if spectral_ref is None else spectral_ref
    ulps = int(GC.f32_ulps(got_graph[2], want))
    err = np.abs(got_node[:, 2].astype(np.float64) - c["node"][:, 2])
    bound = GC.laplacian_bound(n, ei, F, c["node"][:, 2])
    print(f"{name}: n {n} spectral {got_graph[2]!r} want {want!r} ulps {ulps}; laplacian max err {err.max():.3e} "
          f"min slack {(bound - err).min():.3e}")
    assert ulps <= 1, f"{name}: spectral radius {got_graph[2]!r} vs {want!r}"
    assert (err <= bound).all(), f"{name}: laplacian column"


def test_fixture_has_the_cases():
    g = golden()
    served = [k for k in g if g[k]["group"] == "served"]
    host = [k for k in g if g[k]["group"] == "host"]
    assert len(served) == 53 and max(int(g[k]["n"]) for k in served) == 64
    assert sorted(int(g[k]["n"]) for k in host) == [65, 80, 100]
    assert list(GC.served_cases()) == served and list(GC.host_cases()) == host
    for k, (n, ei, F, s) in {**GC.inputs(GC.served_cases()), **GC.inputs(GC.host_cases())}.items():     # the fixture is what the cases module draws
        assert n == int(g[k]["n"]) and s == int(g[k]["source"]) and np.array_equal(ei, g[k]["ei"]) and np.array_equal(F, g[k]["F"])
    # the reference's rule is not connectivity: a path, an even cycle, a star and a complete bipartite graph answer False
    for k in ("path2", "path64", "cycle64", "star64", "k32_32", "grid8x8", "ladder32"):
        assert g[k]["graph"][0] == 0.0, k
    for k in ("cycle63", "k64", "petersen"):
        assert g[k]["graph"][0] == 1.0, k
    assert g["k60_p5"]["graph"][0] == 0.0 and g["gnp100"]["graph"][0] == 1.0


def test_host_route_against_the_reference():
    from kp_gnn_amd import graph_property as GP
    g = golden()
    names = list(g)
    nptr, eptr, ei, F, src = GC.pack([(int(g[k]["n"]), g[k]["ei"], g[k]["F"], int(g[k]["source"])) for k in names])
    node, graph = GP.graph_property_labels_host(nptr, eptr, ei, F, src)
    assert node.dtype == torch.float32 and graph.dtype == torch.float32
    assert tuple(node.shape) == (int(nptr[-1]), 3) and tuple(graph.shape) == (len(names), 3)
    for i, k in enumerate(names):
        check_case(k, node[nptr[i]:nptr[i + 1]].numpy(), graph[i].numpy(), g[k])
    # float32 features are widened exactly: the same labels as from their float64 copies
    F32 = F.astype(np.float32)
    a = GP.graph_property_labels_host(nptr, eptr, torch.from_numpy(ei), torch.from_numpy(F32), torch.from_numpy(src))
    b = GP.graph_property_labels_host(nptr, eptr, ei, F32.astype(np.float64), src)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_host_route_on_a_directed_list():
    """A directed triangle 0 -> 1 -> 2 -> 0 with source 0: distances follow the edges, eccentricity is max(axis=0), the
    laplacian's diagonal is the column sum, and the spectral radius comes from eig (|lambda| = 1 three times)."""
    from kp_gnn_amd import graph_property as GP
    F = np.array([0.25, 0.5, 2.0])
    node, graph = GP.labels_host_f64([0, 3], [0, 3], np.array([[0, 1, 2], [1, 2, 0]]), F, [0])
    assert node[:, 0].tolist() == [0.0, 1.0, 2.0] and node[:, 1].tolist() == [2.0, 2.0, 2.0]
    assert node[:, 2].tolist() == [0.25 - 0.5, 0.5 - 2.0, 2.0 - 0.25]
    # (A^(2^3) = A^2 of a directed 3-cycle is a permutation matrix, whose minimum is 0: "not connected")
    assert graph[0, 0] == 0.0 and graph[0, 1] == 2.0
    # the three eigenvalues all have modulus 1; the reference keeps the REAL PART of whichever eig lists first among them
    W = np.linalg.eig(np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]))[0]
    assert graph[0, 2] == np.abs(W[np.argmax(np.absolute(W))].real)


def test_host_route_refusals():
    from kp_gnn_amd import graph_property as GP
    ok = (3, GC.sym(3, GC.path(3))[1], np.ones(3), 0)
    for bad, word in (((3, np.array([[0, 1, 1], [1, 0, 1]]), np.ones(3), 0), "self loop"),
                      ((3, np.array([[0, 3], [3, 0]]), np.ones(3), 0), "endpoint"),
                      ((3, ok[1], np.ones(3), 3), "source"), ((3, ok[1], np.ones(3), -1), "source")):
        with pytest.raises(ValueError, match=r"graph 1: .*" + word):
            GP.graph_property_labels_host(*GC.pack([ok, bad, ok]))
    with pytest.raises(ValueError):
        GP.graph_property_labels_host([0, 3], [0, 4], ok[1], np.ones(3, dtype=np.int64), [0])      # integer features


def test_normalize_labels_and_source_features():
    from kp_gnn_amd import graph_property as GP
    cases = GC.inputs({k: GC.served_cases()[k] for k in ("petersen", "c5_p7", "k3_iso2")}, seed=3)
    items = list(cases.values())
    nptr, eptr, ei, F, src = GC.pack(items)
    node, graph = GP.graph_property_labels_host(nptr, eptr, ei, F, src)
    train = [2, 0]
    got_node, got_graph = GP.normalize_labels(node, graph, nptr, train)
    # GraphPropertyDataset.process: the maximum over the training graphs, per column, then a plain division
    per_graph = [node[nptr[i]:nptr[i + 1]] for i in range(3)]
    max_node = torch.cat([per_graph[i].max(0)[0].unsqueeze(0) for i in train]).max(0)[0]
    max_graph = torch.cat([graph[i].unsqueeze(0) for i in train]).max(0)[0]
    assert torch.equal(got_node, node / max_node) and torch.equal(got_graph, graph / max_graph)
    assert got_node.dtype == torch.float32 and float(got_node[nptr[0]:nptr[1]].max()) == 1.0
    # a column whose training maximum is 0 is 0 / 0 = nan, as in the reference
    z_node, z_graph = GP.normalize_labels(node, graph * 0, nptr, train)
    assert bool(torch.isnan(z_graph).all()) and torch.equal(z_node, got_node)
    x = GP.source_features(torch.from_numpy(F), src, nptr)
    want = torch.zeros((int(nptr[-1]), 2))
    for i in range(3):
        want[int(nptr[i]) + int(src[i]), 0] = 1.0                # to_categorical(source_node, n)
    want[:, 1] = torch.from_numpy(F).float()
    assert x.dtype == torch.float32 and torch.equal(x, want)
    with pytest.raises(ValueError):
        GP.source_features(torch.from_numpy(F), [0, 12, 0], nptr)
