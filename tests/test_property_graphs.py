"""GPU (-m gpu): ops.property_graphs on the device (csrc/property_graphs.hip) against its host route, field by field, and
graph_property.generate_split - graphs, labels and inputs from a seed without a graph on the host - against the same split
made by the host routes, and into KHopDataset.from_graphs.  The host route is the yardstick here; what holds the host route
to the reference's laws is tests/test_property_graphs_host.py."""
import numpy as np
import pytest
import torch

import graph_property_cases as GC
import property_graph_cases as PC

pytestmark = pytest.mark.gpu

TRAIN_LIKE = tuple(n for n in range(15, 25) for _ in range(16))
LARGE = tuple(n for n in (60, 61, 62, 63, 64, 95, 96, 97, 98, 99) for _ in range(4))


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _same(r, want):
    node_ptr, edge_ptr, ei, feat, source, types, attempts, status = want
    assert r.route == "device" and r.edge_index.device.type == "cuda" and r.features.device.type == "cuda"
    assert r.node_ptr.dtype == np.int64 and r.edge_ptr.dtype == np.int64 and r.edge_index.dtype == torch.int64
    assert np.array_equal(r.node_ptr, node_ptr) and np.array_equal(r.edge_ptr, edge_ptr)
    assert np.array_equal(r.edge_index.cpu().numpy(), ei)
    assert np.array_equal(r.features.cpu().numpy().view(np.uint32), feat.view(np.uint32))
    assert np.array_equal(r.source, source) and np.array_equal(r.types, types) and np.array_equal(r.attempts, attempts)
    assert np.array_equal(r.exhausted, np.flatnonzero(status != 0))


@pytest.mark.parametrize("nodes", (TRAIN_LIKE, LARGE), ids=("15-24", "60-64+95-99"))
def test_device_route_equals_host_route(nodes):
    from kp_gnn_amd import ops
    want = PC.host(nodes, 1)
    r = ops.property_graphs(list(nodes), 1, _dev(), route="device")
    _same(r, want)
    assert len(set(r.types.tolist())) >= 6 and r.exhausted.size == 0
    _same(ops.property_graphs(list(nodes), 1, _dev(), route="device"), want)                # run to run
    cut = len(nodes) // 3
    a = ops.property_graphs(list(nodes[:cut]), 1, _dev(), route="device")
    b = ops.property_graphs(list(nodes[cut:]), 1, _dev(), route="device", first_graph=cut)
    assert np.array_equal(torch.cat([a.edge_index, b.edge_index], dim=1).cpu().numpy(), want[2])
    assert np.array_equal(torch.cat([a.features, b.features]).cpu().numpy(), want[3])
    assert np.array_equal(np.concatenate([a.attempts, b.attempts]), want[6])
    auto = ops.property_graphs(list(nodes[:8]), 1, _dev())
    assert auto.route == ops.PROPERTY_GRAPHS_AUTO


def test_single_size_and_fixed_type():
    from kp_gnn_amd import ops
    for t, n in (("CATERPILLAR", 24), ("GRID", 99), ("BARABASI_ALBERT", 128)):
        _same(ops.property_graphs([n] * 6, 4, _dev(), graph_type=t, route="device"), PC.host((n,) * 6, 4, t))
    r = ops.property_graphs(20, 4, _dev(), graph_type="LADDER", route="device", randomize=False, shuffle=False)
    _same(r, PC.host((20,), 4, "LADDER", randomize=False, shuffle=False))
    assert r.edge_ptr.tolist() == [0, 56]


def test_exhausted_graphs_are_the_host_routes():
    from kp_gnn_amd import graph_property as GP, ops
    nodes = (4,) * 200 + (70,) * 20
    want = PC.host(nodes, 0, "ERDOS_RENYI", max_attempts=1)
    r = ops.property_graphs(list(nodes), 0, _dev(), graph_type="ERDOS_RENYI", route="device", max_attempts=1)
    _same(r, want)
    assert 0 < r.exhausted.size < 220 and (np.diff(r.edge_ptr)[r.exhausted] == 0).all()


def test_generate_split_equals_the_host_routes():
    """Integer labels exactly; the spectral radius and the laplacian column - two float64 computations - to one float32 ulp."""
    from kp_gnn_amd import graph_property as GP
    nodes = list(TRAIN_LIKE[::4]) + [64, 65, 99]
    d = GP.generate_split(nodes, 6, _dev(), route="device")
    h = GP.generate_split(nodes, 6, "cpu", route="host")
    assert np.array_equal(d.node_ptr, h.node_ptr) and np.array_equal(d.edge_ptr, h.edge_ptr)
    assert torch.equal(d.edge_index.cpu(), h.edge_index) and torch.equal(d.x.cpu(), h.x)
    pos, y = d.pos.cpu(), d.y.cpu()
    assert torch.equal(pos[:, :2], h.pos[:, :2]) and torch.equal(y[:, :2], h.y[:, :2])
    # (the features are multiples of 2^-24 below 1, so every float64 sum of the laplacian column is exact in either order)
    for got, want in ((pos[:, 2], h.pos[:, 2]), (y[:, 2], h.y[:, 2])):
        worst = int(GC.f32_ulps(got.numpy(), want.numpy()).max())
        print(f"float32 ulps apart at most: {worst}")
        assert worst <= 1


def test_generate_split_feeds_from_graphs():
    from kp_gnn_amd import graph_property as GP
    from kp_gnn_amd.dataset import KHopDataset
    nodes = list(range(15, 25)) * 2
    s = GP.generate_split(nodes, 8, _dev())
    pos, y = GP.normalize_labels(s.pos, s.y, s.node_ptr, np.arange(len(nodes)))
    ds = KHopDataset.from_graphs(s.node_ptr, s.edge_ptr, s.edge_index, None, _dev(), (3, 50, 6, 3, 50, 50, "spd"), x=s.x, y=y, pos=pos)
    assert torch.equal(ds.node_rows["pos"], pos)
    b = ds.collate(np.array([3, 0, 19]))
    assert tuple(b.pos.shape) == (b.x.shape[0], 3) and b.x.shape[0] == nodes[3] + nodes[0] + nodes[19]
