"""GPU (-m gpu): ops.random_regular_graphs on the device route and simulation.simulate(generator="device").

The yardstick is the host route (kp_gnn_amd/regular_graphs.py, held to the definition and to uniformity by
tests/test_regular_graphs_host.py): route "device" must return its edge_index, attempts and exhausted graphs bit for bit, at
the shapes of tests/regular_graph_cases.py, run to run, and however a call is split by first_graph.  End to end, the simulation
on the device generator repeats itself, gives rate 1.0 at k = 1 (every node of a regular graph has the same 1-hop picture) and
embeds exactly what the pre-transform and the layer make of the host route's graphs."""
import numpy as np
import pytest
import torch

import regular_graph_cases as RC

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("n,d,G", RC.device_cases())
def test_device_route_gives_the_host_route(n, d, G):
    from kp_gnn_amd import ops
    r = ops.random_regular_graphs(G, n, d, 0, _dev(), route="device")
    node_ptr, edge_ptr, ei, attempts, status = RC.host(G, n, d)
    assert r.route == "device" and r.edge_index.is_cuda and r.edge_index.dtype == torch.int64
    assert np.array_equal(r.node_ptr, node_ptr) and np.array_equal(r.edge_ptr, edge_ptr)
    assert r.attempts.dtype == np.int32 and np.array_equal(r.attempts, attempts) and r.exhausted.size == 0
    assert np.array_equal(r.edge_index.cpu().numpy(), ei)
    auto = ops.random_regular_graphs(G, n, d, 0, _dev())
    assert auto.route == "device" and torch.equal(auto.edge_index, r.edge_index)


def test_run_to_run_and_split_by_first_graph():
    from kp_gnn_amd import ops
    one = ops.random_regular_graphs(24, 20, 3, 0, _dev(), route="device")
    two = ops.random_regular_graphs(24, 20, 3, 0, _dev(), route="device")
    assert torch.equal(one.edge_index, two.edge_index) and np.array_equal(one.attempts, two.attempts)
    a = ops.random_regular_graphs(10, 20, 3, 0, _dev(), route="device")
    b = ops.random_regular_graphs(14, 20, 3, 0, _dev(), first_graph=10, route="device")
    assert torch.equal(one.edge_index, torch.cat([a.edge_index, b.edge_index], dim=1))
    assert np.array_equal(one.attempts, np.concatenate([a.attempts, b.attempts]))
    assert np.array_equal(one.edge_index.cpu().numpy(), RC.host(24, 20, 3)[2])
    other = ops.random_regular_graphs(24, 20, 3, 1, _dev(), route="device")
    assert (other.edge_index[1].reshape(24, 60) != one.edge_index[1].reshape(24, 60)).any(dim=1).all()


def test_exhausted_graphs_are_filled_and_named():
    """max_attempts = 1: the device route and the host route exhaust the same graphs, fill them from networkx alike and
    agree on every column."""
    from kp_gnn_amd import ops
    G, n, d = 200, 6, 3
    dev_r = ops.random_regular_graphs(G, n, d, 0, _dev(), first_graph=5, route="device", max_attempts=1)
    host_r = ops.random_regular_graphs(G, n, d, 0, "cpu", first_graph=5, route="host", max_attempts=1)
    assert 0 < dev_r.exhausted.size < G and np.array_equal(dev_r.exhausted, host_r.exhausted)
    assert np.array_equal(dev_r.exhausted, np.flatnonzero(RC.host(G, n, d, 0, 5, 1)[4]))
    assert (dev_r.attempts == 1).all()
    assert np.array_equal(dev_r.edge_index.cpu().numpy(), host_r.edge_index.numpy())
    RC.check_structure(dev_r.node_ptr, dev_r.edge_ptr, dev_r.edge_index.cpu().numpy(), G, n, d)


def test_device_route_refuses_what_the_kernel_does_not_serve():
    from kp_gnn_amd import ops
    with pytest.raises(ops._lib.KpgnnError):
        ops.random_regular_graphs(2, 12, 5, 0, _dev(), route="device")
    r = ops.random_regular_graphs(0, 20, 3, 0, _dev(), route="device")
    assert tuple(r.edge_index.shape) == (2, 0) and r.attempts.size == 0


def test_simulation_on_the_device_generator():
    from kp_gnn_amd import ops, simulation
    from kp_gnn_amd.layers import KGINConv
    dev = _dev()
    rates, outs = simulation.simulate([20], R=3, N=8, K=2, generator="device", return_outputs=True, device=dev)
    again = simulation.simulate([20], R=3, N=8, K=2, generator="device", device=dev)
    assert sorted(rates) == [(20, 1), (20, 2)] and rates == again
    assert rates[(20, 1)] == 1.0
    node_ptr, edge_ptr, ei, _, _ = (a.copy() for a in RC.host(8, 20, 3))
    for k in (1, 2):
        torch.manual_seed(0)
        model = KGINConv(16, k, pool=False).to(dev).eval()
        with torch.no_grad():
            t, status = ops.khop_transform(node_ptr, edge_ptr, ei, None, k, 10, 1, 1, 1, 1, "spd", dev, large="device")
            out = model(torch.ones((160, 1), device=dev), t["edge_index"], t["edge_attr"], t["batch"])
        assert (status.numpy() == 0).all()
        assert tuple(outs[(20, k)].shape) == (160, 16) and torch.equal(out, outs[(20, k)])
    with pytest.raises(ValueError):
        simulation.simulate([20], R=3, N=2, K=1, generator="philox", device=dev)
