"""GPU (-m gpu): graphs above 64 nodes through ops.khop_transform(large="device") and KHopDataset.from_graphs(large=).
Every comparison is with the host route (khop_transform.khop_batch / from_graphs(route="host")) on the same graphs: integers,
bit for bit.  `status` is asserted exactly from the inputs, so the kernel cannot pass by deferring to the host, and the default
(large="host") is pinned to what it did before the keyword existed."""
import argparse
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from khop_device_cases import batch_of, dev, from_nx
from test_khop_device import ZINC, _molecules, _same, _same_tree

pytestmark = pytest.mark.gpu


def _both(b, args, **kw):
    from kp_gnn_amd import khop_transform as KT
    from kp_gnn_amd import ops
    nptr, eptr, ei, ea = b
    want = KT.khop_batch(nptr, eptr, ei, ea, *args)
    got, status = ops.khop_transform(nptr, eptr, torch.from_numpy(ei), None if ea is None else torch.from_numpy(ea), *args, dev(), **kw)
    assert status.dtype == torch.int32 and not status.is_cuda and tuple(status.shape) == (len(nptr) - 1,)
    return got, want, status


def _mixed(extra=()):
    """The batch of test_khop_device.test_graphs_above_the_cap_take_the_host_route_inside_the_call (+ `extra` at the end)."""
    nptr, eptr, ei, ea, _ = _molecules()
    mols = [(int(nptr[g + 1] - nptr[g]), ei[:, eptr[g]:eptr[g + 1]], ea[eptr[g]:eptr[g + 1]]) for g in range(10)]
    graphs = mols[:3] + [from_nx(nx.path_graph(70))] + mols[3:8] + [from_nx(nx.random_regular_graph(3, 80, seed=2))] + mols[8:]
    return batch_of(graphs + list(extra))


def test_the_third_class_is_served_on_the_device_and_the_default_did_not_move():
    b = _mixed()
    got, want, status = _both(b, ZINC, large="device")
    assert status.tolist() == [0] * 12
    _same(got, want)
    for kw in ({}, {"large": "host"}):
        got, want, status = _both(b, ZINC, **kw)
        assert status.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]
        _same(got, want)


def test_what_neither_kernel_serves_takes_the_host_route_inside_the_call():
    from kp_gnn_amd import _lib
    b = _mixed([from_nx(nx.path_graph(_lib.KHOP_LARGE_MAX_NODES + 1)), from_nx(nx.cycle_graph(65))])
    args = (3, 50, 2, 3, 50, 50, "gd")
    got, want, status = _both(b, args, large="device")
    assert status.tolist() == [0] * 12 + [1, 0]
    _same(got, want)
    got, want, status = _both(_mixed(), (17, 50, 6, 3, 50, 50, "spd"), large="device")     # K beyond either kernel
    assert status.tolist() == [5] * 12
    _same(got, want)


def test_range_and_endpoint_raise_what_they_raise_on_the_small_route():
    from kp_gnn_amd import KpgnnError, ops
    nptr, eptr, ei, ea = batch_of([from_nx(nx.path_graph(70), typed=False), from_nx(nx.complete_graph(70), typed=False)])
    with pytest.raises(KpgnnError, match="2\\^31"):
        ops.khop_transform(nptr, eptr, torch.from_numpy(ei), None, 8, 50, 1, 1, 1, 1, "gd", dev(), large="device")
    bad = ei.copy()
    bad[1, 2] = 70                                      # one past the path's last node
    with pytest.raises(ValueError, match="endpoint"):
        ops.khop_transform(nptr, eptr, torch.from_numpy(bad), None, *ZINC, dev(), large="device")


# ------------------------------------------------------------------------------------------------ KHopDataset.from_graphs
ARGS = (3, 50, 6, 3, 50, 50, "spd")
CHUNK = 24


@functools.lru_cache(maxsize=None)
def _raw():
    rng = np.random.default_rng(11)
    sizes = rng.integers(20, 201, size=40)
    sizes[:4] = (20, 200, 64, 65)
    graphs = [from_nx(nx.gnm_random_graph(int(n), 2 * int(n), seed=int(s))) for s, n in enumerate(sizes)]
    nptr, eptr, ei, ea = batch_of(graphs)
    assert (np.diff(nptr) > 64).sum() >= 10 and (np.diff(nptr) > 128).sum() >= 3 and (np.diff(nptr) <= 64).sum() >= 3
    x = torch.from_numpy(rng.integers(0, 21, size=(int(nptr[-1]), 1)))
    y = torch.randn(40, generator=torch.Generator().manual_seed(3))
    return nptr, eptr, ei, ea, x, y


@functools.lru_cache(maxsize=None)
def _dataset(how, with_rd):
    from kp_gnn_amd.dataset import KHopDataset
    nptr, eptr, ei, ea, x, y = _raw()
    kw = dict(route="host") if how == "host" else dict(route="device", large=how)
    return KHopDataset.from_graphs(nptr, eptr, ei, ea, dev(), ARGS, x=x, y=y, chunk_graphs=CHUNK, with_rd=with_rd, **kw)


@pytest.mark.parametrize("how", ["device", "auto"])
def test_from_graphs_is_the_host_dataset_bit_for_bit(how):
    a, b = _dataset(how, False), _dataset("host", False)
    for i, (u, v) in enumerate(zip(a.state(), b.state())):
        _same_tree(u, v, (how, i))
    assert a.uid is not None and torch.equal(a.uid, b.uid) and torch.equal(a.pdict.rows, b.pdict.rows)


def test_from_graphs_with_rd_gives_the_same_column_up_to_the_rd_kernels_cap():
    a, b = _dataset("device", True), _dataset("host", True)
    nptr = _raw()[0]
    keep = torch.from_numpy(np.repeat(np.diff(nptr) <= 128, np.diff(nptr)))
    ra, rb = a.node_rows["rd"].cpu(), b.node_rows["rd"].cpu()
    assert ra.shape == rb.shape and ra.shape[0] == int(nptr[-1]) and bool(keep.any()) and not bool(keep.all())
    assert torch.equal(ra[keep], rb[keep])


def test_a_training_step_is_the_same_step_on_either_dataset():
    """Loss and every gradient bitwise: the collated inputs are bitwise equal and the kernels reproducible."""
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    K, L, H = ARGS[0], 2, 33
    ns = argparse.Namespace(model_name="KPGINPlus", hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(0)
    gnn = B.GNNPlus(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch", init_emb=B.EmbeddingEncoder(21, H),
                    residual=True, virtual_node=False, use_rd=False, num_hop1_edge=3, max_edge_count=50, max_hop_num=6,
                    max_distance_count=50, drop_prob=0.0)
    model = B.GraphRegression(gnn, "sum").to(dev()).train()
    ids = [1, 0, 39, 3, 2, 17, 30, 8]                   # graphs of 200, 20, 64 and 65 nodes among them
    res = []
    for how in ("device", "host"):
        batch = _dataset(how, False).collate(ids)
        model.zero_grad(set_to_none=True)
        loss = (model(batch) - batch.y).abs().mean()
        loss.backward()
        res.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    (l0, g0), (l1, g1) = res
    assert torch.equal(l0, l1) and bool(torch.isfinite(l0))
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n
