"""GPU (-m gpu): the batched resistance-distance kernel (csrc/resistance.hip) through ops.resistance_distance, the device route
of the drop-in khop_transform.resistance_distance(data), and KHopDataset.from_collated(with_rd=True).

Every graph of tests/golden/resistance_distance.pt goes in ONE call, ordered so that the two size classes (a wavefront per
graph up to 32 nodes, a block per graph up to 128) alternate.  The kernel's rows are held to the two bounds of
tests/test_resistance_cabi.py - one float32 ulp of the float64 pseudo-inverse + 1e-9, and never further from the reference
than the reference is from float64 - and `status` is asserted exactly, so the kernel cannot pass by deferring to the host."""
import functools

import numpy as np
import pytest
import torch

from test_resistance_cabi import check_bounds, golden

pytestmark = pytest.mark.gpu

LAUNCH = "kpgnn_resistance_distance"


def _dev():
    return torch.device("cuda:0")


def _order():
    """Fixture names, a graph of the block class after every eighth of the wavefront class."""
    g = golden()
    small = sorted(k for k in g if int(g[k]["n"]) <= 32)
    large = sorted(k for k in g if int(g[k]["n"]) > 32)
    assert {int(g[k]["n"]) for k in large} >= {33, 37, 64, 65, 128, 129} and len(small) >= 8 * len(large)
    out = []
    for i, k in enumerate(small):
        out.append(k)
        if i % 8 == 3 and large:
            out.append(large.pop(0))
    return out + large


def _concat(names, reverse=False):
    """(node_ptr, edge_ptr, edge_index with global ids) of the fixture graphs `names`; reverse: each graph's edges backwards."""
    g = golden()
    nptr, eptr, eis = [0], [0], []
    for k in names:
        ei = g[k]["edge_index"].long()
        eis.append((ei.flip(1) if reverse else ei) + nptr[-1])
        nptr.append(nptr[-1] + int(g[k]["n"]))
        eptr.append(eptr[-1] + ei.shape[1])
    return np.array(nptr, dtype=np.int64), np.array(eptr, dtype=np.int64), torch.cat(eis, dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def _run(reverse=False, on_device=True):
    from kp_gnn_amd import ops
    names = _order()
    nptr, eptr, ei = _concat(names, reverse)
    rd, status = ops.resistance_distance(nptr, eptr, ei.to(_dev()) if on_device else ei, _dev())
    torch.cuda.synchronize()
    assert rd.is_cuda and rd.dtype == torch.float32 and tuple(rd.shape) == (int(nptr[-1]), 1)
    assert status.dtype == torch.int32 and tuple(status.shape) == (len(names),)
    return names, nptr, rd.cpu().reshape(-1), status.cpu()


def _want_status(name):
    return {"path129": 2, "directed_cycle3": 1}.get(name, 0)


def test_status_is_exact():
    names, _, _, status = _run()
    assert status.tolist() == [_want_status(k) for k in names]
    assert int((status == 0).sum()) == len(names) - 2


def test_parity_with_the_reference_and_with_float64():
    names, nptr, rd, status = _run()
    g = golden()
    for i, k in enumerate(names):
        got = rd[nptr[i]:nptr[i + 1]].double().numpy()
        print(f"rd {k}: n {int(g[k]['n'])} status {int(status[i])} max|got - ref64| {float(np.abs(got - g[k]['ref64'].numpy()).max()):.3e}")
        check_bounds(got, g[k], k)               # the kernel's rows (status 0) and the two host-filled graphs alike


def test_exact_values():
    names, nptr, rd, _ = _run()
    for i in range(len(names)):
        assert float(rd[nptr[i]]) == 0.0 and not np.signbit(float(rd[nptr[i]])), names[i]
    i = names.index("path128")
    assert torch.equal(rd[nptr[i]:nptr[i + 1]], torch.arange(128, dtype=torch.float32))
    for k in ("path32", "path33", "path64", "path65", "path5"):
        i = names.index(k)
        assert torch.equal(rd[nptr[i]:nptr[i + 1]], torch.arange(int(nptr[i + 1] - nptr[i]), dtype=torch.float32)), k
    i = names.index("isolated3")
    assert rd[nptr[i]:nptr[i + 1]].tolist() == [0.0, 0.0, 0.0]          # three 1 x 1 blocks: M^-1 - J = 1 - 1, L+ = 0 as pinv(0) is


def test_bitwise_reproducible_and_independent_of_the_edge_order():
    _run.cache_clear()
    a = _run()
    _run.cache_clear()
    b = _run()
    c = _run(reverse=True)
    d = _run(on_device=False)                    # a host edge list is moved to the device: same launches
    for other, what in ((b, "second run"), (c, "reversed edge order"), (d, "host edge list")):
        assert torch.equal(a[2].view(torch.int32), other[2].view(torch.int32)), what
        assert torch.equal(a[3], other[3]), what


def test_range_errors_raise_and_launch_nothing_else(monkeypatch):
    from kp_gnn_amd import _lib, ops
    names = ["path5", "cycle37", "complete20"]
    nptr, eptr, ei = _concat(names)
    launches, real = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    for e, v in ((3, int(nptr[1])),            # path5's edge points at the first node of the next graph: valid in the call, not in its graph
                 (int(eptr[1]) + 4, 4),        # cycle37's edge points back into path5
                 (int(eptr[2]) + 7, int(nptr[3])),     # beyond the last node
                 (0, -1)):
        bad = ei.clone()
        bad[1, e] = v
        del launches[:]
        with pytest.raises(IndexError, match="outside"):
            ops.resistance_distance(nptr, eptr, bad.to(_dev()), _dev())
        assert launches == [LAUNCH] * 2, launches          # the two class launches, the one read-back, then nothing
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.resistance_distance(nptr, eptr, ei[:, :-1].to(_dev()), _dev())
    with pytest.raises(ValueError):
        ops.resistance_distance(nptr[::-1].copy(), eptr, ei.to(_dev()), _dev())


def test_no_graphs_and_empty_graphs(monkeypatch):
    from kp_gnn_amd import ops
    rd, status = ops.resistance_distance([0], [0], torch.zeros((2, 0), dtype=torch.long), _dev())
    assert tuple(rd.shape) == (0, 1) and tuple(status.shape) == (0,)
    # a graph without nodes between two paths, and a lone node
    g = golden()
    p5 = g["path5"]["edge_index"].long()
    ei = torch.cat([p5, p5 + 5], dim=1)
    rd, status = ops.resistance_distance([0, 5, 5, 10, 11], [0, 8, 8, 16, 16], ei.to(_dev()), _dev())
    assert status.tolist() == [0, 0, 0, 0]
    assert rd.reshape(-1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] * 2 + [0.0]


def test_drop_in_takes_the_device_route_for_a_device_edge_list(monkeypatch):
    import types
    from kp_gnn_amd import _lib
    from kp_gnn_amd.khop_transform import resistance_distance
    launches, real = [], _lib.launch
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real(name, *a, **k))[1])
    case = golden()["mol07"]
    n = int(case["n"])
    data = types.SimpleNamespace(edge_index=case["edge_index"].long().to(_dev()), num_nodes=n)
    assert resistance_distance(data) is data and launches == [LAUNCH]
    assert data.rd.is_cuda and data.rd.dtype == torch.float32 and tuple(data.rd.shape) == (n, 1)
    check_bounds(data.rd.cpu().reshape(-1).double().numpy(), case, "drop-in, device")
    # the directed list comes back from the host route, on the device all the same
    case = golden()["directed_cycle3"]
    data = types.SimpleNamespace(edge_index=case["edge_index"].long().to(_dev()), num_nodes=3)
    check_bounds(resistance_distance(data).rd.cpu().reshape(-1).double().numpy(), case, "drop-in, directed")
    assert data.rd.is_cuda


# ------------------------------------------------------------------------------------------------ the resident dataset
K_ARGS = (4, 50, 6, 3, 50, 50, "spd")


@functools.lru_cache(maxsize=None)
def _dataset():
    from test_dataset import molecules
    from kp_gnn_amd.dataset import KHopDataset
    raw = molecules(64, seed0=11)
    host = raw.collated(K_ARGS)
    return raw, host, KHopDataset.from_collated(host, raw.node_ptr, _dev(), with_rd=True)


def test_dataset_rd_is_the_feature_of_the_khop_edge_list():
    """The same 64 molecules and K-hop lists as the fixture's mol00 .. mol63 (synth_molecules(64, 11), K = 4, spd)."""
    from kp_gnn_amd.dataset import KHopDataset
    raw, host, ds = _dataset()
    rd = ds.node_rows["rd"]
    assert rd.dtype == torch.float32 and tuple(rd.shape) == (int(raw.node_ptr[-1]), 1) and rd.is_cuda
    g = golden()
    rows = rd.cpu().reshape(-1)
    for i in range(64):
        check_bounds(rows[raw.node_ptr[i]:raw.node_ptr[i + 1]].double().numpy(), g["mol%02d" % i], "dataset mol%02d" % i)
    # several chunks give the bits of one; without the flag there is no such row; a given rd is carried as it is
    assert torch.equal(KHopDataset.from_collated(host, raw.node_ptr, _dev(), chunk_graphs=10, with_rd=True).node_rows["rd"], rd)
    assert "rd" not in KHopDataset.from_collated(host, raw.node_ptr, _dev()).node_rows
    host.rd = torch.arange(int(raw.node_ptr[-1]), dtype=torch.float32).reshape(-1, 1)
    try:
        for flag in (False, True):
            given = KHopDataset.from_collated(host, raw.node_ptr, _dev(), with_rd=flag).node_rows["rd"]
            assert torch.equal(given.cpu(), host.rd)
    finally:
        del host.rd


def _rows_of(ds, raw, ids):
    rd = ds.node_rows["rd"]
    return torch.cat([rd[int(raw.node_ptr[i]):int(raw.node_ptr[i + 1])] for i in ids])


def test_collate_save_load_and_static_batch_carry_rd(tmp_path):
    from kp_gnn_amd.dataset import KHopDataset
    raw, _, ds = _dataset()
    ids = np.random.default_rng(5).permutation(64)[:20]
    want = _rows_of(ds, raw, ids)
    b = ds.collate(ids)
    assert tuple(b.rd.shape) == (b.x.shape[0], 1) and torch.equal(b.rd, want)
    path = str(tmp_path / "rd64.pt")
    ds.save(path)
    ds2 = KHopDataset.load(path, _dev())
    assert torch.equal(ds2.node_rows["rd"], ds.node_rows["rd"]) and torch.equal(ds2.collate(ids).rd, want)
    sb = ds.static_batch(20)
    for sel in (ids, ids[::-1].copy()):
        sb.stage(sel)
        sb.launch_collate()
        torch.cuda.synchronize()
        live = sb.live[0]
        assert live < sb.N_cap and tuple(sb.batch.rd.shape) == (sb.N_cap, 1)
        assert torch.equal(sb.batch.rd[:live], _rows_of(ds, raw, sel))
