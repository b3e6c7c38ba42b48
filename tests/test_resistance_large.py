"""GPU (-m gpu): the resistance-distance kernel for graphs of 129 to 2048 nodes (csrc/resistance_large.hip) through
ops.resistance_distance(large="device"), and KHopDataset.from_graphs(rd_large="device").

ONE call holds a mix of the three size classes: a few molecules, cycle37, path128 and path129 of
tests/golden/resistance_distance.pt, every case of tests/golden/resistance_distance_large.pt, and path257 and path2048 made
here.  `status` is asserted exactly and a spy on khop_transform.resistance_distance_host sees exactly the graphs whose status is
not 0, so the kernel cannot pass by deferring to the host.

Bounds: the two of tests/test_resistance_cabi.py on every fixture case.  For the graphs without a fixture, and for the closed
forms (path: y; cycle: y (n - y) / n; star: 1 and 2; complete: 2 / n), bound (1): one float32 ulp of the float64 value + 1e-9.
A float64 numpy restatement of the unpivoted blocked sweep (b = 32) differs from pinv by at most 3.2e-7 (path of 2048 nodes,
0.3 % of the bound at its worst element) and by less than 3e-10 up to 257 nodes, so the bound holds with room and the paths of
129, 130 and 257 nodes must come out as arange(n) bit for bit."""
import functools

import numpy as np
import pytest
import torch

from test_resistance_cabi import check_bounds, golden, ulp32
from test_resistance_large_cabi import golden_large

pytestmark = pytest.mark.gpu

SMALL, LARGE = "kpgnn_resistance_distance", "kpgnn_resistance_distance_large"
ORDER = ["mol00", "path130", "cycle37", "path2048", "mol01", "cycle160", "path128", "star161", "path129", "complete150",
         "mol02", "gnm191_dup_loop", "directed_cycle200", "two_paths_plus_isolated257", "mol03", "path257", "node0_isolated140"]


def _dev():
    return torch.device("cuda:0")


def _path(n):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])])


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(n, edge_index int64 with local ids, the fixture case or None)."""
    for g in (golden(), golden_large()):
        if name in g:
            return int(g[name]["n"]), g[name]["edge_index"].long(), g[name]
    assert name.startswith("path")
    return int(name[4:]), _path(int(name[4:])), None


@functools.lru_cache(maxsize=None)
def _host64(name):
    """The parent's float64 host route, once per graph."""
    from kp_gnn_amd.khop_transform import resistance_distance_host
    n, ei, _ = _graph(name)
    return resistance_distance_host(n, ei)


def _closed_form(name):
    n = _graph(name)[0]
    y = np.arange(n, dtype=np.float64)
    if name.startswith("path"):
        return y
    if name.startswith("cycle"):
        return y * (n - y) / n
    if name.startswith("star"):
        return np.where(y == 0, 0.0, 1.0)                 # node 0 is the centre: 1 to every leaf (2 between leaves)
    if name.startswith("complete"):
        return np.where(y == 0, 0.0, 2.0 / n)
    return None


def _concat(names, reverse=False):
    nptr, eptr, eis = [0], [0], []
    for k in names:
        n, ei, _ = _graph(k)
        eis.append((ei.flip(1) if reverse else ei) + nptr[-1])
        nptr.append(nptr[-1] + n)
        eptr.append(eptr[-1] + ei.shape[1])
    return np.array(nptr, dtype=np.int64), np.array(eptr, dtype=np.int64), torch.cat(eis, dim=1).contiguous()


def _call(names, reverse=False, on_device=True, **kw):
    from kp_gnn_amd import ops
    nptr, eptr, ei = _concat(names, reverse)
    rd, status = ops.resistance_distance(nptr, eptr, ei.to(_dev()) if on_device else ei, _dev(), **kw)
    torch.cuda.synchronize()
    assert rd.is_cuda and rd.dtype == torch.float32 and tuple(rd.shape) == (int(nptr[-1]), 1)
    assert status.dtype == torch.int32 and tuple(status.shape) == (len(names),)
    return nptr, rd.cpu().reshape(-1), status.cpu()


@functools.lru_cache(maxsize=None)
def _mix():
    return _call(ORDER, large="device")


def _rows(res, i):
    nptr, rd, _ = res
    return rd[nptr[i]:nptr[i + 1]]


def _spies(monkeypatch, stub=False):
    """Record the launches and the node counts handed to the host route (stub: which then returns zeros)."""
    from kp_gnn_amd import _lib
    from kp_gnn_amd import khop_transform as KT
    launches, hosted, real_launch, real_host = [], [], _lib.launch, KT.resistance_distance_host
    monkeypatch.setattr(_lib, "launch", lambda name, *a, **k: (launches.append(name), real_launch(name, *a, **k))[1])
    monkeypatch.setattr(KT, "resistance_distance_host",
                        lambda n, ei: (hosted.append(int(n)), np.zeros(int(n)) if stub else real_host(n, ei))[1])
    return launches, hosted


def test_the_mix_holds_all_three_classes_and_every_large_fixture_case():
    sizes = [_graph(k)[0] for k in ORDER]
    assert set(golden_large()) <= set(ORDER)
    assert min(sizes) <= 32 and any(32 < n <= 128 for n in sizes) and {129, 130, 257, 2048} <= set(sizes)


def test_status_is_exact_and_the_host_fills_only_what_the_kernel_did_not_serve(monkeypatch):
    launches, hosted = _spies(monkeypatch)
    _, _, status = _call(ORDER, large="device")
    assert status.tolist() == [1 if k == "directed_cycle200" else 0 for k in ORDER]
    assert hosted == [200]                                # the directed cycle and nothing else
    assert launches == [SMALL, SMALL, LARGE]
    assert torch.equal(status, _mix()[2])


def test_a_graph_above_2048_nodes_gets_status_2_and_the_host_route(monkeypatch):
    launches, hosted = _spies(monkeypatch, stub=True)
    _, rd, status = _call(["path129", "path2049", "mol00"], large="device")
    assert status.tolist() == [0, 2, 0] and hosted == [2049]
    assert launches == [SMALL, SMALL, LARGE]              # 2049 nodes ride the block-class launch, which says 2
    assert torch.equal(rd[:129], torch.arange(129, dtype=torch.float32)) and not bool(rd[129:129 + 2049].any())


def test_parity_with_the_reference_with_float64_and_with_the_closed_forms():
    res = _mix()
    for i, k in enumerate(ORDER):
        n, _, case = _graph(k)
        got = _rows(res, i).double().numpy()
        if case is not None:
            print(f"rd {k}: n {n} status {int(res[2][i])} max|got - ref64| {float(np.abs(got - case['ref64'].numpy()).max()):.3e}")
            check_bounds(got, case, k)                   # the kernels' rows and the host-filled directed cycle alike
        else:
            want = _host64(k)
            err = np.abs(got - want)
            print(f"rd {k}: n {n} status {int(res[2][i])} max|got - host float64| {float(err.max()):.3e}")
            assert bool((err <= ulp32(want) + 1e-9).all()), (k, float(err.max()))
        exact = _closed_form(k)
        if exact is not None:
            err = np.abs(got - exact)
            print(f"rd {k}: max|got - closed form| {float(err.max()):.3e}")
            assert bool((err <= ulp32(exact) + 1e-9).all()), (k, float(err.max()))


def test_exact_values():
    res = _mix()
    for i, k in enumerate(ORDER):
        first = float(_rows(res, i)[0])
        assert first == 0.0 and not np.signbit(first), k
    for k in ("path128", "path129", "path130", "path257"):
        assert torch.equal(_rows(res, ORDER.index(k)), torch.arange(_graph(k)[0], dtype=torch.float32)), k
    exact = torch.equal(_rows(res, ORDER.index("path2048")), torch.arange(2048, dtype=torch.float32))
    print("path2048 equals arange(2048) bit for bit:", exact)


def test_bits_do_not_depend_on_the_run_the_edge_order_the_edge_lists_home_or_the_workspace(monkeypatch):
    from kp_gnn_amd import _lib
    a = _mix()
    slab300 = int(_lib.load().kpgnn_rd_large_workspace_bytes(300, 1))
    launches, _ = _spies(monkeypatch)
    runs = (("second run", dict()), ("reversed edge order", dict(reverse=True)), ("host edge list", dict(on_device=False)),
            ("one 300-node graph per launch", dict(workspace_bytes=slab300)), ("a graph per launch", dict(workspace_bytes=1)))
    counts = {}
    for what, kw in runs:
        del launches[:]
        b = _call(ORDER, large="device", **kw)
        counts[what] = launches.count(LARGE)
        assert launches[:2] == [SMALL, SMALL] and set(launches[2:]) == {LARGE}, what
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), what
        assert torch.equal(a[2], b[2]), what
    n_large = sum(_graph(k)[0] > 128 for k in ORDER)
    assert counts["second run"] == counts["reversed edge order"] == counts["host edge list"] == 1
    assert counts["a graph per launch"] == n_large == 11
    # a slab is sized for its launch's largest graph, rounded up to 32 rows: slab(300) holds one graph of 193 nodes or more, two
    # of 161 .. 192, three of up to 160.  In call order: 130 | 2048 | 160, 161 | 129, 150 | 191 | 200 | 257 | 257 | 140
    assert 1 < counts["one 300-node graph per launch"] < n_large
    assert counts["one 300-node graph per launch"] == 9


@pytest.mark.parametrize("name", [k for k in ORDER if k in ("path129", "path257", "path2048") or k in golden_large()])
def test_a_large_graph_alone_gives_the_bits_it_has_in_the_mix(name):
    a = _mix()
    _, rd, status = _call([name], large="device")
    i = ORDER.index(name)
    assert int(status[0]) == int(a[2][i])
    assert torch.equal(rd.view(torch.int32), _rows(a, i).view(torch.int32))


def test_range_errors_raise_and_nothing_is_filled_afterwards(monkeypatch):
    from kp_gnn_amd import ops
    names = ["cycle160", "path130", "mol00"]
    nptr, eptr, ei = _concat(names)
    launches, hosted = _spies(monkeypatch)
    for e, v in ((5, 160),                       # cycle160's edge points at the first node of its neighbour
                 (int(eptr[1]) + 3, 159),        # path130's edge points back into cycle160
                 (int(eptr[1]) + 3, int(nptr[3])),
                 (0, -1)):
        bad = ei.clone()
        bad[1, e] = v
        del launches[:]
        with pytest.raises(IndexError, match="outside"):
            ops.resistance_distance(nptr, eptr, bad.to(_dev()), _dev(), large="device")
        assert launches == [SMALL, LARGE] and hosted == [], launches
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.resistance_distance(nptr, eptr, ei.to(_dev()), _dev(), large="gpu")


def test_the_default_is_pinned_to_the_host_route(monkeypatch):
    launches, hosted = _spies(monkeypatch, stub=True)
    names = [k for k in ORDER if k != "path2048"]
    want = [2 if _graph(k)[0] > 128 else 0 for k in names]
    for kw in ({}, {"large": "host"}):
        del launches[:], hosted[:]
        _, _, status = _call(names, **kw)
        assert launches == [SMALL, SMALL], kw
        assert status.tolist() == want, kw
        assert hosted == [_graph(k)[0] for k in names if _graph(k)[0] > 128], kw


def test_drop_in_passes_the_keyword_on_for_a_device_edge_list(monkeypatch):
    import types
    from kp_gnn_amd.khop_transform import resistance_distance
    launches, hosted = _spies(monkeypatch)
    n, ei, case = _graph("cycle160")
    data = types.SimpleNamespace(edge_index=ei.to(_dev()), num_nodes=n)
    assert resistance_distance(data, large="device") is data and launches == [LARGE] and hosted == []
    assert data.rd.is_cuda and tuple(data.rd.shape) == (n, 1)
    check_bounds(data.rd.cpu().reshape(-1).double().numpy(), case, "drop-in, device")
    del launches[:]
    resistance_distance(data)
    assert launches == [SMALL] and hosted == [160]


def test_through_the_c_abi_a_graph_above_the_launchs_max_nodes_gets_status_2_and_its_rows_stay():
    """One launch sized for 160 nodes: the 191-node graph is status 2 with its rows untouched, an id outside [0, G) is skipped,
    a graph the launch does not name is not written, and a workspace full of NaN bit patterns (it need not be zeroed) gives the
    bits of the mix."""
    import ctypes
    from kp_gnn_amd import _lib
    names = ["cycle160", "gnm191_dup_loop", "path129", "mol00", "path130"]
    nptr, eptr, ei = _concat(names)
    dev = _dev()
    ids = torch.tensor([0, 1, 7, 2, 3], dtype=torch.int32, device=dev)          # 7 is no graph of the call; path130 is not named
    out = torch.full((int(nptr[-1]),), -7.0, device=dev)
    st = torch.full((len(names),), -1, dtype=torch.int32, device=dev)
    need = int(_lib.load().kpgnn_rd_large_workspace_bytes(160, 5))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    keep = [torch.from_numpy(nptr).to(dev), torch.from_numpy(eptr).to(dev), ei.to(dev)]
    d = _lib.RdLargeDesc()
    d.G, d.n_ids, d.E, d.max_nodes = len(names), 5, int(eptr[-1]), 160
    d.node_ptr, d.edge_ptr, d.edge_index, d.graph_ids = keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), ids.data_ptr()
    d.out, d.status, d.workspace, d.workspace_bytes = out.data_ptr(), st.data_ptr(), ws.data_ptr(), need
    _lib.launch(LARGE, dev, ctypes.byref(d))
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [0, 2, 0, 0, -1]
    out = out.cpu()
    mix = _mix()
    for i, k in enumerate(names):
        rows = out[nptr[i]:nptr[i + 1]]
        if k in ("gnm191_dup_loop", "path130"):
            assert bool((rows == -7.0).all()), k
        elif k == "mol00":                                # 26 nodes: the kernel serves any n up to the launch's max_nodes
            check_bounds(rows.double().numpy(), _graph(k)[2], k + " on the large kernel")
        else:
            assert torch.equal(rows.view(torch.int32), _rows(mix, ORDER.index(k)).view(torch.int32)), k


# ------------------------------------------------------------------------------------------------ the resident dataset
@functools.lru_cache(maxsize=None)
def _dataset(rd_large, chunk):
    from test_khop_large import ARGS, _raw
    from kp_gnn_amd.dataset import KHopDataset
    nptr, eptr, ei, ea, x, y = _raw()
    kw = {} if rd_large is None else {"rd_large": rd_large}
    return KHopDataset.from_graphs(nptr, eptr, ei, ea, _dev(), ARGS, x=x, y=y, chunk_graphs=chunk, with_rd=True, route="device",
                                   large="device", **kw)


def test_from_graphs_computes_the_rd_column_of_large_graphs_on_the_device(monkeypatch):
    from test_khop_large import CHUNK, _raw
    nptr = _raw()[0]
    nodes = np.diff(nptr)
    launches, hosted = _spies(monkeypatch)
    dev_ds = _dataset("device", CHUNK)
    assert hosted == [] and launches.count(LARGE) == 2                    # 40 graphs in chunks of 24, large ones in both
    default = _dataset(None, CHUNK)
    assert hosted == [int(n) for n in nodes if n > 128]                   # the default still asks the host for each of them
    a, b = dev_ds.node_rows["rd"].cpu().reshape(-1), default.node_rows["rd"].cpu().reshape(-1)
    assert a.shape == b.shape == (int(nptr[-1]),)
    small = torch.from_numpy(np.repeat(nodes <= 128, nodes))
    assert bool(small.any()) and int((nodes > 128).sum()) >= 3
    assert torch.equal(a[small].view(torch.int32), b[small].view(torch.int32))
    big_a, big_b = a[~small].double().numpy(), b[~small].double().numpy()
    err = np.abs(big_a - big_b)
    print(f"dataset rows of graphs above 128 nodes: max|device - host| {float(err.max()):.3e}")
    assert bool((err <= ulp32(big_b) + 1e-9).all()), float(err.max())
    other = _dataset("device", 7)
    assert torch.equal(other.node_rows["rd"].view(torch.int32), dev_ds.node_rows["rd"].view(torch.int32))
    ids = np.random.default_rng(2).permutation(40)[:12]
    want = torch.cat([dev_ds.node_rows["rd"][int(nptr[i]):int(nptr[i + 1])] for i in ids])
    assert torch.equal(dev_ds.collate(ids).rd, want)
