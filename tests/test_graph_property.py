"""GPU (-m gpu): the graph-property label kernel (csrc/graph_labels.hip) through ops.graph_property_labels, and the node targets
it gives carried as `pos` by KHopDataset.from_graphs.

The 53 graphs of tests/golden/graph_property.npz go in ONE call with the host route forbidden, so the kernel cannot pass by
deferring to it: the four integer labels bit-exact as float32, the spectral radius within one float32 ulp of float64 eigvalsh,
the laplacian column within its derived bound (graph_property_cases.laplacian_bound)."""
import functools

import numpy as np
import pytest
import torch

import graph_property_cases as GC
from test_graph_property_host import check_case, golden

pytestmark = pytest.mark.gpu

LAUNCH = "kpgnn_graph_labels"


def _dev():
    return torch.device("cuda:0")


def _eigvalsh_radius(n, ei):
    A = np.zeros((n, n))
    A[ei[0], ei[1]] = 1.0
    return float(np.abs(np.linalg.eigvalsh(A)).max()) if ei.size else 0.0


def _device_only(monkeypatch):
    """Forbid the host route and record the launches of a call."""
    from kp_gnn_amd import _lib, graph_property as GP
    launches, real = [], _lib.launch

    def spy(name, *a, **k):
        launches.append(name)
        return real(name, *a, **k)

    def no_host(*a, **k):
        raise AssertionError("the host route was taken")
    monkeypatch.setattr(_lib, "launch", spy)
    monkeypatch.setattr(GP, "labels_host_f64", no_host)
    return launches


def _labels(items, route="device", on_device=False):
    from kp_gnn_amd import ops
    nptr, eptr, ei, F, src = GC.pack(items)
    ei_t = torch.from_numpy(ei).to(_dev()) if on_device else ei
    node, graph = ops.graph_property_labels(nptr, eptr, ei_t, F, src, _dev(), route=route)
    torch.cuda.synchronize()
    assert node.is_cuda and node.dtype == torch.float32 and tuple(node.shape) == (int(nptr[-1]), 3)
    assert graph.is_cuda and graph.dtype == torch.float32 and tuple(graph.shape) == (len(items), 3)
    return nptr, node.cpu(), graph.cpu()


def test_the_53_fixture_graphs_in_one_call(monkeypatch):
    g = golden()
    names = [k for k in g if g[k]["group"] == "served"]
    assert len(names) == 53
    launches = _device_only(monkeypatch)
    nptr, node, graph = _labels([(int(g[k]["n"]), g[k]["ei"], g[k]["F"], int(g[k]["source"])) for k in names], on_device=True)
    assert launches == [LAUNCH, LAUNCH]                   # one per size class, nothing else
    for i, k in enumerate(names):
        c = g[k]
        check_case(k, node[nptr[i]:nptr[i + 1]].numpy(), graph[i].numpy(), c, spectral_ref=_eigvalsh_radius(int(c["n"]), c["ei"]))
    assert int(graph[:, 0].sum()) == int(sum(g[k]["graph"][0] for k in names))


def test_edge_sizes_against_the_host_route(monkeypatch):
    """n in {1, 2, 3, 31, 32, 33, 63, 64} as a path, a complete graph and a graph with one isolated node: the sizes at which a
    size class or a lane mask can go wrong (n = 64 uses bit 63 and m = 7, n = 33 is the first of the block class, n = 1 has
    m = 1 and A^2 = 0: not connected)."""
    from kp_gnn_amd import graph_property as GP
    cases = GC.inputs(GC.edge_size_cases(), seed=5)
    assert len(cases) == 3 * len(GC.EDGE_SIZES)
    items = list(cases.values())
    host_node, host_graph = GP.labels_host_f64(*GC.pack(items))
    launches = _device_only(monkeypatch)
    nptr, node, graph = _labels(items)
    assert launches == [LAUNCH, LAUNCH]
    for i, (k, (n, ei, F, s)) in enumerate(cases.items()):
        c = {"n": n, "ei": ei, "F": F, "node": host_node[nptr[i]:nptr[i + 1]], "graph": host_graph[i]}
        check_case(k, node[nptr[i]:nptr[i + 1]].numpy(), graph[i].numpy(), c)
    for n in GC.EDGE_SIZES:
        i = list(cases).index(f"complete{n}")
        assert graph[i].tolist() == [float(n >= 3), float(n >= 2), float(n - 1)], n      # K_n: walks of every length >= 2 once n >= 3
        assert graph[list(cases).index(f"path{n}"), 0] == 0.0                             # bipartite (or a single node)


def _launch_raw(items, ids, poison=float("nan")):
    """The graphs `ids` of the call `items` through ops.graph_labels_launch, one launch per size class, into poisoned outputs:
    (node_ptr, node_out, graph_out, status) on the host, status -7 where nothing was written."""
    from kp_gnn_amd import _lib, ops
    dev = _dev()
    nptr, eptr, ei, F, src = GC.pack(items)
    G, N, E = len(items), int(nptr[-1]), int(eptr[-1])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    nptr_d, eptr_d, ei_d, F_d, src_d = t(nptr, torch.int64), t(eptr, torch.int64), t(ei, torch.int64), t(F, torch.float64), t(src, torch.int32)
    node = torch.full((N, 3), poison, dtype=torch.float32, device=dev)
    graph = torch.full((G, 3), poison, dtype=torch.float32, device=dev)
    st = torch.full((G,), -7, dtype=torch.int32, device=dev)
    ids = np.asarray(ids, dtype=np.int64)
    nodes = np.diff(nptr)
    for sel in (ids[nodes[ids] <= _lib.GL_WAVE_NODES], ids[nodes[ids] > _lib.GL_WAVE_NODES]):
        if sel.size:
            ids_d = t(sel, torch.int32)
            ops.graph_labels_launch(G, nptr_d, eptr_d, ei_d, E, F_d, src_d, ids_d, min(_lib.GL_MAX_NODES, int(nodes[sel].max())), node, graph, st)
    torch.cuda.synchronize()
    return nptr, node.cpu(), graph.cpu(), st.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_bits_depend_on_the_graph_alone():
    """The same graphs with each graph's edges shuffled, with the graph order reversed, and with graph_ids a strict subset:
    bitwise equal rows per graph, and the rows of a graph outside graph_ids keep their NaN poison."""
    g = golden()
    names = [k for k in g if g[k]["group"] == "served"][::2]
    items = [(int(g[k]["n"]), g[k]["ei"], g[k]["F"], int(g[k]["source"])) for k in names]
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
    _, node_p, graph_p, st_p = _launch_raw(items, sub)
    sizes = {int(np.diff(nptr)[i]) > 32 for i in sub}
    assert sizes == {False, True}                           # both size classes are in the subset
    for i in range(G):
        rows = slice(int(nptr[i]), int(nptr[i + 1]))
        if i in sub:
            assert int(st_p[i]) == 0 and torch.equal(_bits(node_p[rows]), _bits(node[rows])) and torch.equal(_bits(graph_p[i]), _bits(graph[i]))
        else:
            assert int(st_p[i]) == -7 and bool(torch.isnan(node_p[rows]).all()) and bool(torch.isnan(graph_p[i]).all()), names[i]


def test_routing_inside_one_call(monkeypatch):
    """A 65-node graph (status 2) and a directed triangle (status 1) take the host route inside the call that serves three
    graphs on the device; only kpgnn_graph_labels is launched."""
    from kp_gnn_amd import _lib, graph_property as GP
    g = golden()
    served = [(int(g[k]["n"]), g[k]["ei"], g[k]["F"], int(g[k]["source"])) for k in ("petersen", "grid8x8", "c5_p7")]
    big = g["k60_p5"]
    items = [served[0], (65, big["ei"], big["F"], int(big["source"])), served[1],
             (3, np.array([[0, 1, 2], [1, 2, 0]]), np.array([0.25, 0.5, 2.0]), 0), served[2]]
    host_node, host_graph = GP.labels_host_f64(*GC.pack(items))
    _, _, _, st = _launch_raw(items, np.arange(5))
    assert st.tolist() == [0, _lib.GL_TOO_LARGE, 0, _lib.GL_ASYMMETRIC, 0]
    launches, real = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    nptr, node, graph = _labels(items)
    assert launches == [LAUNCH, LAUNCH]
    for i in (1, 3):                                        # host-filled: the host route's float32 rows, bit for bit
        assert np.array_equal(node[nptr[i]:nptr[i + 1]].numpy(), host_node[nptr[i]:nptr[i + 1]].astype(np.float32))
        assert np.array_equal(graph[i].numpy(), host_graph[i].astype(np.float32))
    for i in (0, 2, 4):
        n, ei, F, _ = items[i]
        c = {"n": n, "ei": ei, "F": F, "node": host_node[nptr[i]:nptr[i + 1]], "graph": host_graph[i]}
        check_case(f"graph {i}", node[nptr[i]:nptr[i + 1]].numpy(), graph[i].numpy(), c)
    nptr_h, node_h, graph_h = _labels(items, route="host")
    assert np.array_equal(node_h.numpy(), host_node.astype(np.float32)) and np.array_equal(graph_h.numpy(), host_graph.astype(np.float32))


def test_refusals_are_errors_not_faults():
    """A self loop, an endpoint equal to n, source == n and source == -1: ValueError naming the graph, from the status the kernel
    wrote after checking every range before any indexed access; the device serves the next call as if nothing had happened."""
    from kp_gnn_amd import _lib
    ok = (40, GC.sym(40, GC.cycle(40))[1], np.ones(40), 7)
    small = GC.sym(5, GC.cycle(5))[1]
    for bad, word, code in (((5, np.concatenate([small, [[2], [2]]], axis=1), np.ones(5), 0), "self loop", _lib.GL_SELF_LOOP),
                            ((5, np.concatenate([small, [[4, 5], [5, 4]]], axis=1), np.ones(5), 0), "endpoint", _lib.GL_ENDPOINT),
                            ((5, small, np.ones(5), 5), "source", _lib.GL_SOURCE), ((5, small, np.ones(5), -1), "source", _lib.GL_SOURCE),
                            ((40, ok[1], np.ones(40), 40), "source", _lib.GL_SOURCE)):
        items = [ok, ok, bad, ok]
        _, node, graph, st = _launch_raw(items, np.arange(4))
        assert st.tolist() == [0, 0, code, 0]
        rows = slice(2 * 40, 2 * 40 + bad[0])
        assert bool(torch.isnan(node[rows]).all()) and bool(torch.isnan(graph[2]).all())        # nothing written where status != 0
        with pytest.raises(ValueError, match="graph 2: .*" + word):
            _labels(items)
    nptr, node, graph = _labels([ok])
    assert graph[0].tolist() == [0.0, 20.0, 2.0] and node[:, 1].tolist() == [20.0] * 40


# ------------------------------------------------------------------------------------------------ from_graphs(pos=labels)
K_ARGS = (3, 50, 6, 3, 50, 50, "spd")


@functools.lru_cache(maxsize=None)
def _dataset(K=K_ARGS[0]):
    from kp_gnn_amd import graph_property as GP, ops
    from kp_gnn_amd.dataset import KHopDataset
    rng = np.random.default_rng(40)
    items = []
    while len(items) < 40:
        n = int(rng.integers(15, 25))
        _, ei = GC.sym(n, GC.gnp(n, 0.2, rng))
        if np.unique(ei[0]).size == n:                      # no singleton nodes, as in the reference's generator
            items.append((n, ei, rng.random(n), int(rng.integers(0, n))))
    nptr, eptr, ei, F, src = GC.pack(items)
    node, graph = ops.graph_property_labels(nptr, eptr, ei, F, src, _dev())
    x = GP.source_features(torch.from_numpy(F), src, nptr)
    ds = KHopDataset.from_graphs(nptr, eptr, ei, None, _dev(), (K,) + K_ARGS[1:], x=x, y=graph, pos=node)
    return (nptr, eptr, ei), node, graph, x, ds


def _rows(nptr, ids):
    return torch.cat([torch.arange(int(nptr[i]), int(nptr[i + 1])) for i in ids]).to(_dev())


def test_from_graphs_carries_pos_through_collate_static_batch_and_save(tmp_path):
    from kp_gnn_amd.dataset import KHopDataset
    (nptr, eptr, ei), node, graph, x, ds = _dataset()
    assert ds.node_rows["pos"].dtype == torch.float32 and torch.equal(_bits(ds.node_rows["pos"]), _bits(node))
    rng = np.random.default_rng(6)
    lists = [rng.permutation(40)[:12], np.array([39, 0, 7, 7, 21])]
    for ids in lists:
        b = ds.collate(ids)
        assert tuple(b.pos.shape) == (b.x.shape[0], 3) and torch.equal(_bits(b.pos), _bits(node[_rows(nptr, ids)]))
        assert torch.equal(b.x, x.to(_dev())[_rows(nptr, ids)]) and torch.equal(b.y, graph[torch.from_numpy(ids).to(_dev())])
    sb = ds.static_batch(12)
    for ids in (lists[0], lists[0][::-1].copy()):
        sb.stage(ids)
        sb.launch_collate()
        torch.cuda.synchronize()
        live = sb.live[0]
        assert tuple(sb.batch.pos.shape) == (sb.N_cap, 3) and torch.equal(_bits(sb.batch.pos[:live]), _bits(node[_rows(nptr, ids)]))
    path = str(tmp_path / "gp40.pt")
    ds.save(path)
    ds2 = KHopDataset.load(path, _dev())
    assert torch.equal(_bits(ds2.node_rows["pos"]), _bits(node))
    assert torch.equal(_bits(ds2.collate(lists[1]).pos), _bits(node[_rows(nptr, lists[1])]))
    # no pos given: no such rows, as before
    e5 = int(eptr[5])
    assert "pos" not in KHopDataset.from_graphs(nptr[:6], eptr[:6], ei[:, :e5], None, _dev(), K_ARGS).node_rows


@pytest.mark.parametrize("K", [1, 3])
def test_one_node_regression_step_on_pos(K):
    """One forward / backward step of a 2-layer KP-GIN+ NodeRegression against pos[:, 0] (sssp) with the L1 loss: a finite loss
    and a finite gradient on every parameter.  At K > 1 the layers hold a path-encoding table (hopk_node_path_emb) of which the
    pre-transform only ever uses the padding row: the reference gives it a zero gradient, this package none
    (layers/_base.py _path_encoding), so those tables - and nothing else - may come back without one; K = 1 has no such table."""
    import argparse
    from kp_gnn_amd import body as B, ops_dense
    from kp_gnn_amd.layers import make_gnn_layer
    _, node, graph, x, ds = _dataset(K)
    H, L = 32, 2
    ns = argparse.Namespace(model_name="KPGINPlus", hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch", init_emb=B.LinearEncoder(2, H),
                         residual=True, virtual_node=False, use_rd=False, num_hop1_edge=3, max_edge_count=50, max_hop_num=6,
                         max_distance_count=50, drop_prob=0.0)
    model = B.NodeRegression(gnn).to(_dev()).train()
    b = ds.collate(np.arange(16))
    out = model(b)
    assert tuple(out.shape) == (b.pos.shape[0],)
    loss = ops_dense.regression_loss(out, b.pos[:, 0], "l1")
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    without = [name for name, q in model.named_parameters() if q.grad is None]
    print(f"K {K}: loss {float(loss.detach()):.6f}, {len(list(model.parameters()))} parameters, without a gradient: {without}")
    assert all(name.endswith("hopk_node_path_emb.weight") for name in without) and (K > 1 or not without), without
    for name, q in model.named_parameters():
        assert q.grad is None or bool(torch.isfinite(q.grad).all()), name
