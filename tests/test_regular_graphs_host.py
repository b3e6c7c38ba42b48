"""CPU: the host route of the random regular graphs (kp_gnn_amd/regular_graphs.py: the pairing model with rejection, the
definition of include/kpgnn.h in numpy) and the front end's routing, ops.random_regular_graphs, as far as it needs no device.

What a uniform simple d-regular graph generator must give: d-regular simple graphs in the (src, dst)-sorted layout; K4 and K5
where nothing else exists; every one of the 70 labelled cubic graphs on 6 nodes equally often (chi-square against the 0.999
quantile, a deterministic run); graph g a function of (seed, first_graph + g) alone; and, against the definition written a
second time in plain integers (tests/regular_graph_cases.py), the same pairings, attempt counts and exhausted graphs."""
import numpy as np
import pytest
import torch

import regular_graph_cases as RC

STRUCTURE = ((2, 1, 16), (5, 2, 16), (4, 3, 16), (6, 3, 16), (5, 4, 16), (20, 3, 16), (64, 4, 16), (1280, 3, 2))


@pytest.mark.parametrize("n,d,G", STRUCTURE)
def test_graphs_are_simple_regular_and_sorted(n, d, G):
    node_ptr, edge_ptr, ei, attempts, status = RC.host(G, n, d)
    assert status.dtype == np.int32 and attempts.dtype == np.int32
    assert (status == 0).all() and (attempts >= 1).all() and (attempts <= 4096).all()
    RC.check_structure(node_ptr, edge_ptr, ei, G, n, d)


@pytest.mark.parametrize("n,d", ((4, 3), (5, 4)))
@pytest.mark.parametrize("seed", (0, 1, 2 ** 40 + 12345))
def test_complete_graphs_are_forced(n, d, seed):
    """The only 3-regular graph on 4 nodes is K4, the only 4-regular one on 5 nodes K5: whatever the seed."""
    _, _, ei, _, status = RC.host(16, n, d, seed)
    assert (status == 0).all()
    want = np.array([(u, v) for u in range(n) for v in range(n) if u != v], dtype=np.int64).T
    assert np.array_equal(ei, np.tile(want, (1, 16)))


def test_cubic_graphs_on_six_nodes_are_uniform():
    """7,000 graphs of (6,3) from seed 0: exactly the 70 labelled cubic graphs on 6 nodes, and Pearson's chi-square against
    100 per graph below 111.06, the 0.999 quantile at 69 degrees of freedom.  (A numpy permutation pairing model: 70 and 81.0;
    this generator: 70 and 71.14.)"""
    G, m = 7000, 18
    _, _, ei, attempts, status = RC.host(G, 6, 3)
    assert (status == 0).all()
    sets, counts = np.unique(ei[1].reshape(G, m), axis=0, return_counts=True)
    chi2 = float(((counts - 100.0) ** 2 / 100.0).sum())
    print(f"distinct edge sets {len(sets)}, chi-square {chi2:.2f}, mean attempts {attempts.mean():.3f}")
    assert len(sets) == 70
    assert chi2 < 111.06


def test_a_graph_depends_on_its_seed_and_id_alone():
    whole = RC.host(24, 20, 3)
    a, b = RC.host(10, 20, 3), RC.host(14, 20, 3, first_graph=10)
    assert np.array_equal(whole[2], np.concatenate([a[2], b[2]], axis=1))
    assert np.array_equal(whole[3], np.concatenate([a[3], b[3]])) and np.array_equal(whole[4], np.concatenate([a[4], b[4]]))
    other = RC.host(24, 20, 3, seed=1)
    differs = (whole[2][1].reshape(24, 60) != other[2][1].reshape(24, 60)).any(axis=1)
    assert differs.all()


@pytest.mark.parametrize("n,d,seed,first", ((6, 3, 0, 0), (20, 3, 7, 2 ** 33 + 5), (5, 4, -3, 1), (10, 4, 2 ** 63 - 1, 0), (5, 2, 11, 3)))
def test_the_numpy_route_follows_the_definition(n, d, seed, first):
    """The definition once more in plain integers: the first simple pairing of each graph, and how many came before it."""
    G = 4
    _, _, ei, attempts, status = RC.host(G, n, d, seed, first_graph=first)
    assert (status == 0).all()
    for g in range(G):
        a = 0
        while not RC.simple(RC.pairing(n, d, seed, first + g, a), d):
            a += 1
        assert attempts[g] == a + 1
        assert np.array_equal(ei[:, g * n * d:(g + 1) * n * d], RC.graph_of(RC.pairing(n, d, seed, first + g, a), n, d))


def test_exhausted_graphs_and_their_fill():
    """max_attempts = 1 at (6,3): a graph is exhausted exactly when its first pairing is not simple; the front end fills those
    from networkx under the seed `seed + first_graph + g`, names them, and leaves the others as the host route made them."""
    from kp_gnn_amd import batch, ops
    G, n, d, seed, first = 200, 6, 3, 0, 5
    node_ptr, edge_ptr, ei, attempts, status = RC.host(G, n, d, seed, first_graph=first, max_attempts=1)
    assert (attempts == 1).all()
    want = np.array([not RC.simple(RC.pairing(n, d, seed, first + g, 0), d) for g in range(G)])
    assert 0 < (~want).sum() < G                        # (about a tenth is accepted)
    assert np.array_equal(status != 0, want) and set(status.tolist()) == {0, 1}
    assert (ei.reshape(2, G, n * d)[:, want] == 0).all()                     # not written
    RC.check_structure(np.arange((~want).sum() + 1) * n, np.arange((~want).sum() + 1) * n * d,
                       ei.reshape(2, G, n * d)[:, ~want].reshape(2, -1), int((~want).sum()), n, d)
    r = ops.random_regular_graphs(G, n, d, seed, "cpu", first_graph=first, route="host", max_attempts=1)
    assert r.route == "host" and np.array_equal(r.exhausted, np.flatnonzero(want)) and np.array_equal(r.attempts, attempts)
    got = r.edge_index.numpy().reshape(2, G, n * d)
    assert np.array_equal(got[:, ~want], ei.reshape(2, G, n * d)[:, ~want])
    for g in np.flatnonzero(want):
        assert np.array_equal(got[:, g], batch.regular_graphs(1, seed + first + int(g), n=n, degree=d)[2]), g
    RC.check_structure(r.node_ptr, r.edge_ptr, r.edge_index.numpy(), G, n, d)


def test_arguments_and_routing():
    from kp_gnn_amd import batch, ops, ops_dataset, regular_graphs as RG
    for route in ("auto", "device", "host", "networkx"):
        for n, d in ((5, 3), (7, 1), (4, 4), (3, 5), (1, 1)):               # n * d odd, or d >= n
            with pytest.raises(ValueError):
                ops.random_regular_graphs(2, n, d, 0, "cpu", route=route)
    with pytest.raises(ValueError):
        ops.random_regular_graphs(2, 6, 3, 0, "cpu", route="pairing")
    with pytest.raises(ValueError):
        ops.random_regular_graphs(2, 6, 3, 0, "cpu", max_attempts=0)
    with pytest.raises(ValueError):                                         # the pairing routes stop at their limits ...
        RG.random_regular_graphs_host(1, 12, 5, 0)
    cpu, gpu = torch.device("cpu"), torch.device("cuda:0")
    for n, d in ((12, 5), (2050, 2), (2049, 4), (14, 6)):                    # ... and "auto" hands what lies beyond to networkx
        assert ops_dataset.regular_graphs_route(n, d, gpu) == ops_dataset.regular_graphs_route(n, d, cpu) == "networkx"
    for n, d in ((2, 1), (20, 3), (2048, 4), (1280, 3)):
        assert ops_dataset.regular_graphs_route(n, d, gpu) == "device" and ops_dataset.regular_graphs_route(n, d, cpu) == "host"
    r = ops.random_regular_graphs(3, 12, 5, 4, "cpu", first_graph=2)
    node_ptr, edge_ptr, ei = batch.regular_graphs(3, 6, n=12, degree=5)
    assert r.route == "networkx" and r.attempts is None and r.exhausted.size == 0
    assert np.array_equal(r.node_ptr, node_ptr) and np.array_equal(r.edge_ptr, edge_ptr) and np.array_equal(r.edge_index.numpy(), ei)
    r = ops.random_regular_graphs(5, 20, 3, 0, "cpu")                       # no device: the host route, the same bits
    assert r.route == "host" and r.exhausted.size == 0 and np.array_equal(r.edge_index.numpy(), RC.host(5, 20, 3)[2])
    with pytest.raises(ops._lib.KpgnnError):
        ops.random_regular_graphs(5, 20, 3, 0, "cpu", route="device")
    r = ops.random_regular_graphs(0, 20, 3, 0, "cpu")
    assert r.node_ptr.tolist() == [0] and tuple(r.edge_index.shape) == (2, 0)
