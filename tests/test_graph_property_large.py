"""GPU (-m gpu): the graph-property label kernel of graphs of up to 128 nodes (csrc/graph_labels.hip, W = 2), through
ops.graph_property_labels(large="device") and through raw kpgnn_graph_labels_large launches into poisoned outputs.

The rules are those of test_graph_property.py (check_case): the four integer labels bit-exact as float32, the spectral radius
within one float32 ulp of float64 eigvalsh - Householder in double at n = 128 errs about nine orders of magnitude below a
float32 ulp, so the 1 covers the rounding boundary only - and the laplacian column within graph_property_cases.laplacian_bound.
The yardstick is the fixture of the reference's own answers (tests/golden/graph_property_large.npz) where the graph is in it,
else graph_property.labels_host_f64, which test_graph_property_large_host.py ties to that fixture."""
import numpy as np
import pytest
import torch

import graph_property_cases as GC
import graph_property_large_cases as GL
from test_graph_property_host import check_case, golden
from test_graph_property_large_host import golden_large, items_of

pytestmark = pytest.mark.gpu

SMALL, LARGE = "kpgnn_graph_labels", "kpgnn_graph_labels_large"


def _dev():
    return torch.device("cuda:0")


def _spy(monkeypatch, forbid_host=False):
    """Record the launches of a call; forbid_host: the host route raises."""
    from kp_gnn_amd import _lib, graph_property as GP
    launches, real = [], _lib.launch

    def spy(name, *a, **k):
        launches.append(name)
        return real(name, *a, **k)

    def no_host(*a, **k):
        raise AssertionError("the host route was taken")
    monkeypatch.setattr(_lib, "launch", spy)
    if forbid_host:
        monkeypatch.setattr(GP, "labels_host_f64", no_host)
    return launches


def _labels(items, **kw):
    from kp_gnn_amd import ops
    nptr, eptr, ei, F, src = GC.pack(items)
    node, graph = ops.graph_property_labels(nptr, eptr, ei, F, src, _dev(), route="device", **kw)
    torch.cuda.synchronize()
    assert node.is_cuda and node.dtype == torch.float32 and tuple(node.shape) == (int(nptr[-1]), 3)
    assert graph.is_cuda and graph.dtype == torch.float32 and tuple(graph.shape) == (len(items), 3)
    return nptr, node.cpu(), graph.cpu()


def _launch_raw(items, ids, max_nodes=None, poison=float("nan")):
    """The graphs `ids` of the call `items` in ONE kpgnn_graph_labels_large launch sized for their largest (or max_nodes), into
    poisoned outputs: (node_ptr, node_out, graph_out, status) on the host, status -7 where nothing was written."""
    from kp_gnn_amd import ops
    dev = _dev()
    nptr, eptr, ei, F, src = GC.pack(items)
    G, N, E = len(items), int(nptr[-1]), int(eptr[-1])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    nptr_d, eptr_d, ei_d, F_d, src_d = t(nptr, torch.int64), t(eptr, torch.int64), t(ei, torch.int64), t(F, torch.float64), t(src, torch.int32)
    node = torch.full((N, 3), poison, dtype=torch.float32, device=dev)
    graph = torch.full((G, 3), poison, dtype=torch.float32, device=dev)
    st = torch.full((G,), -7, dtype=torch.int32, device=dev)
    ids = np.asarray(ids, dtype=np.int64)
    cap = int(np.diff(nptr)[ids].max()) if max_nodes is None else max_nodes
    ops.graph_labels_launch(G, nptr_d, eptr_d, ei_d, E, F_d, src_d, t(ids, torch.int32), cap, node, graph, st, entry=LARGE)
    torch.cuda.synchronize()
    return nptr, node.cpu(), graph.cpu(), st.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _eigvalsh_radius(n, ei):
    A = np.zeros((n, n))
    A[ei[0], ei[1]] = 1.0
    return float(np.abs(np.linalg.eigvalsh(A)).max()) if ei.size else 0.0


def test_the_fixture_graphs_in_one_call(monkeypatch):
    """The 17 graphs of the new fixture and the three of 65, 80 and 100 nodes of the existing one, in one large="device" call
    with the host route forbidden: one launch, of the large entry."""
    g, small = golden_large(), golden()
    both = {**g, **{k: small[k] for k in ("k60_p5", "gnp80", "gnp100")}}
    names = list(both)
    launches = _spy(monkeypatch, forbid_host=True)
    nptr, node, graph = _labels(items_of(both, names), large="device")
    assert launches == [LARGE]
    for i, k in enumerate(names):
        c = both[k]
        check_case(k, node[nptr[i]:nptr[i + 1]].numpy(), graph[i].numpy(), c, spectral_ref=_eigvalsh_radius(int(c["n"]), c["ei"]))
    # K60 + P5: the literal squaring meets no inf * 0 at m = 8, and the two components answer 0; dense G(100, 0.9): inf > 0
    assert graph[names.index("k60_p5"), 0] == 0.0 and graph[names.index("gnp100"), 0] == 1.0


def test_boundary_sizes_against_the_host_route():
    """n in {1, 2, 63, 64, 65, 66, 127, 128} as a path, a complete graph, a cycle, an edgeless graph and a graph whose last node
    is isolated, and G(128, 0.95), through ONE raw launch into NaN-poisoned outputs: bit 63 / bit 64 (the first of the second
    word) / bit 127, n == 64 and n == 128 (a full last word: no shift by 64), the tail masks in between, m from 1 to 8."""
    from kp_gnn_amd import graph_property as GP
    cases = GC.inputs(GL.boundary_cases(), seed=7)
    assert len(cases) == 5 * len(GL.BOUNDARY_SIZES) + 1
    items = list(cases.values())
    host_node, host_graph = GP.labels_host_f64(*GC.pack(items))
    nptr, node, graph, st = _launch_raw(items, np.arange(len(items)))
    assert st.tolist() == [0] * len(items) and not bool(torch.isnan(node).any()) and not bool(torch.isnan(graph).any())
    for i, (k, (n, ei, F, s)) in enumerate(cases.items()):
        c = {"n": n, "ei": ei, "F": F, "node": host_node[nptr[i]:nptr[i + 1]], "graph": host_graph[i]}
        check_case(k, node[nptr[i]:nptr[i + 1]].numpy(), graph[i].numpy(), c)
    names = list(cases)
    for n in GL.BOUNDARY_SIZES:
        assert graph[names.index(f"complete{n}")].tolist() == [float(n >= 3), float(n >= 2), float(n - 1)], n    # K128 included
        assert graph[names.index(f"path{n}"), 0] == 0.0 and graph[names.index(f"edgeless{n}")].tolist() == [0.0, 0.0, 0.0]
        assert graph[names.index(f"isolated{n}"), 0] == 0.0
        assert graph[names.index(f"cycle{n}"), 0] == float(n >= 3 and n % 2 == 1), n                             # an odd cycle is not bipartite
    assert graph[names.index("gnp128_0.95"), 0] == 1.0


def test_bits_depend_on_the_graph_alone():
    """The fixture graphs with each graph's edges shuffled, with the graph order reversed, with graph_ids a strict subset and
    in a launch sized for 128 whatever its members: bitwise equal rows per graph; a graph outside graph_ids keeps its NaN
    poison and its status -7."""
    from kp_gnn_amd import _lib
    g = golden_large()
    names = list(g)
    items = items_of(g, names)
    G = len(items)
    nptr, node, graph, st = _launch_raw(items, np.arange(G))
    assert st.tolist() == [0] * G and not bool(torch.isnan(node).any()) and not bool(torch.isnan(graph).any())
    rng = np.random.default_rng(2)
    shuffled = [(n, ei[:, rng.permutation(ei.shape[1])], F, s) for n, ei, F, s in items]
    _, node_s, graph_s, st_s = _launch_raw(shuffled, np.arange(G))
    assert st_s.tolist() == [0] * G and torch.equal(_bits(node_s), _bits(node)) and torch.equal(_bits(graph_s), _bits(graph))
    nptr_r, node_r, graph_r, st_r = _launch_raw(items[::-1], np.arange(G)[::-1].copy())
    assert st_r.tolist() == [0] * G and torch.equal(_bits(graph_r.flip(0)), _bits(graph))
    for i in range(G):
        j = G - 1 - i
        assert torch.equal(_bits(node_r[nptr_r[j]:nptr_r[j + 1]]), _bits(node[nptr[i]:nptr[i + 1]])), names[i]
    sub = np.sort(rng.permutation(G)[:G // 2])
    sizes = np.diff(nptr)
    for cap in (None, 128):                                 # sized for the subset's largest member, and for the entry's cap
        _, node_p, graph_p, st_p = _launch_raw(items, sub, max_nodes=cap)
        for i in range(G):
            rows = slice(int(nptr[i]), int(nptr[i + 1]))
            if i in sub:
                assert int(st_p[i]) == 0 and torch.equal(_bits(node_p[rows]), _bits(node[rows])) and torch.equal(_bits(graph_p[i]), _bits(graph[i])), names[i]
            else:
                assert int(st_p[i]) == -7 and bool(torch.isnan(node_p[rows]).all()) and bool(torch.isnan(graph_p[i]).all()), names[i]
    # a launch sized below a member: status 2 for it, nothing written, the others as before
    _, node_c, graph_c, st_c = _launch_raw(items, np.arange(G), max_nodes=100)
    for i in range(G):
        rows = slice(int(nptr[i]), int(nptr[i + 1]))
        if sizes[i] > 100:
            assert int(st_c[i]) == _lib.GL_TOO_LARGE and bool(torch.isnan(node_c[rows]).all()) and bool(torch.isnan(graph_c[i]).all()), names[i]
        else:
            assert int(st_c[i]) == 0 and torch.equal(_bits(node_c[rows]), _bits(node[rows])) and torch.equal(_bits(graph_c[i]), _bits(graph[i])), names[i]


def test_routing_inside_one_call(monkeypatch):
    """Graphs of 24, 64, 65, 128 and 129 nodes and a directed 70-node cycle in one call.  large="device": three launches, the
    third the large entry's; the 129-node graph (status 2) and the directed one (status 1, from the large kernel) carry the
    host route's float32 rows bit for bit.  The default: two launches, and the 65- and 128-node graphs carry them too."""
    from kp_gnn_amd import graph_property as GP
    rng = np.random.default_rng(64)
    items = []
    for n, p in ((24, 0.2), (64, 0.1), (65, 0.1), (128, 0.06), (129, 0.05)):
        items.append((n, GC.sym(n, GC.gnp(n, p, rng))[1], rng.random(n), int(rng.integers(0, n))))
    ring = np.stack([np.arange(70), (np.arange(70) + 1) % 70]).astype(np.int64)
    items.append((70, ring, rng.random(70), 3))
    host_node, host_graph = GP.labels_host_f64(*GC.pack(items))
    rows = lambda nptr, i: slice(int(nptr[i]), int(nptr[i + 1]))  # noqa: E731

    def host_bits(node, graph, nptr, i):
        return (np.array_equal(node[rows(nptr, i)].numpy(), host_node[rows(nptr, i)].astype(np.float32))
                and np.array_equal(graph[i].numpy(), host_graph[i].astype(np.float32)))

    launches = _spy(monkeypatch)
    nptr, node, graph = _labels(items, large="device")
    assert launches == [SMALL, SMALL, LARGE]
    for i in (4, 5):
        assert host_bits(node, graph, nptr, i), i
    for i in (0, 1, 2, 3):
        n, ei, F, _ = items[i]
        c = {"n": n, "ei": ei, "F": F, "node": host_node[rows(nptr, i)], "graph": host_graph[i]}
        check_case(f"graph {i}", node[rows(nptr, i)].numpy(), graph[i].numpy(), c)
    del launches[:]
    nptr, node_h, graph_h = _labels(items)                 # large="host" is the default
    assert launches == [SMALL, SMALL]
    for i in (2, 3, 4, 5):
        assert host_bits(node_h, graph_h, nptr, i), i
    for i in (0, 1):                                        # the classes of at most 64 nodes do not change with `large`
        assert torch.equal(_bits(node_h[rows(nptr, i)]), _bits(node[rows(nptr, i)])) and torch.equal(_bits(graph_h[i]), _bits(graph[i]))
    with pytest.raises(ValueError, match="large"):
        _labels(items, large="gpu")


def test_refusals_are_errors_not_faults():
    """A self loop, an endpoint equal to n, source == n and source == -1 in a 100-node graph under large="device": ValueError
    naming the graph, from the status the kernel wrote after checking every range before any indexed access; outputs keep
    their poison where the status is not 0; the device serves the next call as if nothing had happened."""
    from kp_gnn_amd import _lib
    ring = GC.sym(100, GC.cycle(100))[1]
    ok = (100, ring, np.ones(100), 7)
    for bad, word, code in (((100, np.concatenate([ring, [[70], [70]]], axis=1), np.ones(100), 0), "self loop", _lib.GL_SELF_LOOP),
                            ((100, np.concatenate([ring, [[99, 100], [100, 99]]], axis=1), np.ones(100), 0), "endpoint", _lib.GL_ENDPOINT),
                            ((100, ring, np.ones(100), 100), "source", _lib.GL_SOURCE), ((100, ring, np.ones(100), -1), "source", _lib.GL_SOURCE)):
        items = [ok, ok, bad, ok]
        _, node, graph, st = _launch_raw(items, np.arange(4))
        assert st.tolist() == [0, 0, code, 0]
        assert bool(torch.isnan(node[200:300]).all()) and bool(torch.isnan(graph[2]).all())        # nothing written where status != 0
        assert not bool(torch.isnan(node[:200]).any()) and not bool(torch.isnan(node[300:]).any())
        with pytest.raises(ValueError, match="graph 2: .*" + word):
            _labels(items, large="device")
    nptr, node, graph = _labels([ok], large="device")
    assert graph[0].tolist() == [0.0, 50.0, 2.0] and node[:, 1].tolist() == [50.0] * 100
