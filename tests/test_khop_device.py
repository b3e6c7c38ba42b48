"""GPU (-m gpu): the device K-hop pre-transform through ops.khop_transform, the drop-in
khop_transform.extract_multi_hop_neighbors on a device edge list, and KHopDataset.from_graphs.  Every comparison is with the
host route (khop_transform.khop_batch / KHopDataset.from_collated) on the same graphs: integers, bit for bit, shapes
included.  `status` is asserted exactly, so the kernel cannot pass by deferring to the host."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from khop_device_cases import batch_of, dev, from_nx

pytestmark = pytest.mark.gpu

ZINC = (8, 50, 6, 3, 50, 50, "spd")
KEYS = ("edge_index", "edge_attr", "pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr", "batch", "edge_ptr",
        "node_ptr")


def _same(got, want, where=""):
    """Every key of the khop_batch dict: None where the host gives None, else int64 on the device and equal, shape included."""
    assert set(got) == set(KEYS) == set(want), where
    for k in KEYS:
        if want[k] is None:
            assert got[k] is None, (where, k)
            continue
        assert got[k] is not None and got[k].is_cuda and got[k].dtype == torch.int64, (where, k)
        assert tuple(got[k].shape) == tuple(want[k].shape) and torch.equal(got[k].cpu(), want[k]), (where, k)


def _both(nptr, eptr, ei, ea, args, on_device=False):
    from kp_gnn_amd import khop_transform as KT
    from kp_gnn_amd import ops
    want = KT.khop_batch(nptr, eptr, ei, ea, *args)
    t_ei, t_ea = torch.from_numpy(ei), None if ea is None else torch.from_numpy(ea)
    if on_device:
        t_ei, t_ea = t_ei.to(dev()), None if t_ea is None else t_ea.to(dev())
    got, status = ops.khop_transform(nptr, eptr, t_ei, t_ea, *args, dev())
    assert status.dtype == torch.int32 and not status.is_cuda and tuple(status.shape) == (len(nptr) - 1,)
    return got, want, status


@functools.lru_cache(maxsize=None)
def _molecules(qm9=False):
    from kp_gnn_amd import khop_transform as KT
    return KT.synth_molecules(24, seed0=100, shape=KT.qm9_shape() if qm9 else None)


@pytest.mark.parametrize("args,qm9", [((5, 4, 3, 2, 3, 5, "spd"), False), ((5, 4, 3, 2, 3, 5, "gd"), False), (ZINC, False),
                                      ((16, 50, 6, 3, 50, 50, "gd"), False), ((6, 50, 5, 4, 20, 15, "spd"), True)],
                         ids=["small_spd", "small_gd", "zinc", "zinc_gd16", "qm9"])
def test_molecules_match_khop_batch(args, qm9):
    nptr, eptr, ei, ea, _ = _molecules(qm9)
    got, want, status = _both(nptr, eptr, ei, ea, args, on_device=qm9)
    assert status.tolist() == [0] * 24                  # degrees <= 3: every walk count <= 3^16 < 2^31
    _same(got, want)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_directed_multigraphs_match_the_host_route(seed):
    """The trials of test_khop_host.test_host_random_multigraphs_vs_oracle (seed 0: the same generator, the same draws), and
    three more seeds: duplicates, self loops, mixed types."""
    rng = np.random.default_rng(seed)
    ran = 0
    for trial in range(12):
        n = int(rng.integers(3, 14))
        E = int(rng.integers(1, 40))
        ei = rng.integers(0, n, size=(2, E))
        ea = rng.integers(2, 5, size=E)
        kernel = "spd" if trial % 2 else "gd"
        args = (int(rng.integers(1, 5)), 6, int(rng.integers(1, 4)), int(rng.integers(1, 4)), 3, 4, kernel)
        if (ei[0] != ei[1]).sum() == 0:
            continue
        got, want, status = _both(np.array([0, n]), np.array([0, E]), np.ascontiguousarray(ei), ea, args)
        assert status.tolist() == [0], (seed, trial)
        _same(got, want, (seed, trial))
        ran += 1
    assert ran >= 10


def test_equal_counts_go_to_the_lower_type():
    """K_6, max_edge_type = 2: inside node 0's 1-hop set {1..5} the directed edges carry types 4, 3 and 2 six times each (and
    type 5 twice), listed with the high types first.  The stable descending sort keeps types 2 and 3."""
    ei = np.array(sorted(nx.complete_graph(6).to_directed().edges), dtype=np.int64).T
    inner = np.flatnonzero((ei[0] > 0) & (ei[1] > 0))
    assert inner.size == 20
    ea = np.full(ei.shape[1], 2, dtype=np.int64)
    ea[inner] = [4] * 6 + [3] * 6 + [2] * 6 + [5] * 2
    got, want, status = _both(np.array([0, 6]), np.array([0, 30]), np.ascontiguousarray(ei), ea, (2, 5, 2, 2, 50, 50, "spd"))
    assert status.tolist() == [0]
    assert want["peripheral_edge_attr"][0, 0].tolist() == [[0, 6], [1, 6]]
    _same(got, want)


@pytest.mark.parametrize("args,none", [((3, 5, 0, 2, 3, 5, "spd"), ("peripheral_edge_attr", "peripheral_configuration_attr")),
                                       ((3, 5, 2, 0, 3, 5, "gd"), ("peripheral_edge_attr", "peripheral_configuration_attr")),
                                       ((1, 5, 2, 2, 3, 5, "spd"), ("pe_attr",))], ids=["no_hops", "no_types", "k1"])
def test_absent_tensors_are_none(args, none):
    nptr, eptr, ei, ea, _ = _molecules()
    got, want, status = _both(nptr[:7], eptr[:7], np.ascontiguousarray(ei[:, :eptr[6]]), ea[:eptr[6]], args)
    assert status.tolist() == [0] * 6
    for k in none:
        assert got[k] is None and want[k] is None
    _same(got, want)


def test_graphs_above_the_cap_take_the_host_route_inside_the_call():
    nptr, eptr, ei, ea, _ = _molecules()
    mols = [(int(nptr[g + 1] - nptr[g]), ei[:, eptr[g]:eptr[g + 1]], ea[eptr[g]:eptr[g + 1]]) for g in range(10)]
    graphs = mols[:3] + [from_nx(nx.path_graph(70))] + mols[3:8] + [from_nx(nx.random_regular_graph(3, 80, seed=2))] + mols[8:]
    b = batch_of(graphs)
    got, want, status = _both(*b, ZINC)
    assert status.tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]
    _same(got, want)
    got, want, status = _both(*b, (17, 50, 6, 3, 50, 50, "spd"))           # K beyond the kernel: the host serves all of them
    assert status.tolist() == [5] * 12
    _same(got, want)


def test_range_and_endpoint_raise_what_the_host_route_raises():
    from kp_gnn_amd import KpgnnError, ops
    from kp_gnn_amd import khop_transform as KT
    nptr, eptr, ei, ea = batch_of([from_nx(nx.path_graph(5), typed=False), from_nx(nx.complete_graph(8), typed=False)])
    args = (16, 50, 1, 1, 1, 1, "gd")
    with pytest.raises(KpgnnError) as host:
        KT.khop_batch([0, 8], [0, 56], ei[:, 8:], None, *args)
    with pytest.raises(KpgnnError) as device:
        ops.khop_transform(nptr, eptr, torch.from_numpy(ei), None, *args, dev())
    assert "2^31" in str(host.value) and "2^31" in str(device.value)
    bad = ei.copy()
    bad[1, 2] = 5                                       # one past the path's last node
    with pytest.raises(ValueError):
        KT.khop_batch(nptr, eptr, bad, None, *ZINC)
    with pytest.raises(ValueError):
        ops.khop_transform(nptr, eptr, torch.from_numpy(bad).to(dev()), None, *ZINC, dev())


class _Data:
    pass


def test_extract_multi_hop_neighbors_on_a_device_edge_list():
    from kp_gnn_amd import khop_transform as KT
    nptr, eptr, ei, ea, _ = _molecules()
    n, sl = int(nptr[1]), slice(0, int(eptr[1]))
    out = []
    for where in ("cpu", dev()):
        d = _Data()
        d.x, d.num_nodes = torch.ones(n, 1), n
        d.edge_index, d.edge_attr = torch.from_numpy(ei[:, sl]).to(where), torch.from_numpy(ea[sl]).to(where)
        assert KT.extract_multi_hop_neighbors(d, *ZINC) is d
        out.append(d)
    for k in ("edge_index", "edge_attr", "pe_attr", "peripheral_edge_attr", "peripheral_configuration_attr"):
        h, g = getattr(out[0], k), getattr(out[1], k)
        assert not h.is_cuda and g.is_cuda and g.dtype == torch.int64 and tuple(g.shape) == tuple(h.shape), k
        assert torch.equal(g.cpu(), h), k


# ------------------------------------------------------------------------------------------------ KHopDataset.from_graphs
IDS = [5, 63, 0, 17, 17, 40]


@functools.lru_cache(maxsize=None)
def _raw():
    from kp_gnn_amd import khop_transform as KT
    nptr, eptr, ei, ea, x = KT.synth_molecules(64, seed0=7)
    y = torch.randn(64, generator=torch.Generator().manual_seed(7))
    return nptr, eptr, ei, ea, torch.from_numpy(x).view(-1, 1), y


@functools.lru_cache(maxsize=None)
def _collated(with_rd):
    from kp_gnn_amd.batch import collate_khop
    from kp_gnn_amd.dataset import KHopDataset
    nptr, eptr, ei, ea, x, y = _raw()
    hb = collate_khop(nptr, eptr, ei, ea, x, ZINC, y=y)
    return KHopDataset.from_collated(hb, nptr, dev(), with_rd=with_rd)


@functools.lru_cache(maxsize=None)
def _graphs(route, with_rd, chunk):
    from kp_gnn_amd.dataset import KHopDataset
    nptr, eptr, ei, ea, x, y = _raw()
    return KHopDataset.from_graphs(nptr, eptr, ei, ea, dev(), ZINC, x=x, y=y, chunk_graphs=chunk, with_rd=with_rd, route=route)


def _same_tree(a, b, where):
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), where
        for k in a:
            _same_tree(a[k], b[k], where + (k,))
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(a, b), where
    else:
        assert a == b, where


def _same_dataset(a, b, where):
    for i, (u, v) in enumerate(zip(a.state(), b.state())):
        _same_tree(u, v, (where, i))
    for k in ("h_nodes", "h_pairs", "h_ents", "h_hop_pairs", "h_edges"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), (where, k)
    assert (a.max_code0, a.max_codek, a.G, a.K, a.Nd) == (b.max_code0, b.max_codek, b.G, b.K, b.Nd), where
    assert a.uid is not None and torch.equal(a.uid, b.uid) and torch.equal(a.pdict.rows, b.pdict.rows), where
    assert a.pdict.col_max == b.pdict.col_max and torch.equal(a.pdict.dominant, b.pdict.dominant), where


@pytest.mark.parametrize("route,with_rd,chunk", [("device", False, 4096), ("device", True, 4096), ("device", False, 10),
                                                 ("device", True, 10), ("host", False, 4096), ("auto", True, 4096)],
                         ids=["device", "device_rd", "device_chunks", "device_rd_chunks", "host", "auto_rd"])
def test_from_graphs_equals_from_collated(route, with_rd, chunk):
    a, b = _graphs(route, with_rd, chunk), _collated(with_rd)
    assert ("rd" in a.node_rows) == with_rd
    _same_dataset(a, b, route)


@pytest.mark.parametrize("with_rd", [False, True])
def test_a_collated_batch_is_the_same_from_either_dataset(with_rd):
    """Tensor for tensor: what makes a training step on either dataset the same step."""
    a, b = _graphs("device", with_rd, 4096).collate(IDS), _collated(with_rd).collate(IDS)
    torch.cuda.synchronize()
    names = ["x", "y", "batch"] + (["rd"] if with_rd else [])
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert (a.csr.N, a.csr.A, a.csr.E, a.num_khop_edges) == (b.csr.N, b.csr.A, b.csr.E, b.num_khop_edges)
    A = a.csr.A
    for k in ("rowptr_dst", "rowptr_src", "tile_ptr", "graph_ptr"):
        assert torch.equal(getattr(a.csr, k), getattr(b.csr, k)), k
    for k in ("col_dst", "col_src", "code_dst", "code_src"):
        assert torch.equal(getattr(a.csr, k)[:A], getattr(b.csr, k)[:A]), k
    n_ent = int(a.csr.tile_ptr[-1])
    assert torch.equal(a.csr.tile_pack[:n_ent], b.csr.tile_pack[:n_ent])
    assert torch.equal(a.peripheral_dict.uid, b.peripheral_dict.uid)
    assert torch.equal(a.peripheral_dict.pdict.rows, b.peripheral_dict.pdict.rows)
