"""GPU (-m gpu): the substructure-count label kernel (csrc/count_labels.hip) through ops.count_labels, and the labels it gives
carried as `y` by KHopDataset.from_graphs.

Every graph of tests/golden/graph_count.npz that the kernel serves goes in ONE call per group with the host route forbidden,
so the kernel cannot pass by deferring to it: the four integer labels equal to the reference's, cus within its derived bound
(graph_count_cases.cus_bound)."""
import numpy as np
import pytest
import torch

import graph_count_cases as GC
from graph_property_cases import cycle, gnp, sym
from test_graph_count_host import golden, host_rows

pytestmark = pytest.mark.gpu

LAUNCH = "kpgnn_count_labels"


def _dev():
    return torch.device("cuda:0")


def _spy(monkeypatch, forbid_host=True):
    """Record the launches of a call and (unless told otherwise) forbid the host route."""
    from kp_gnn_amd import _lib, graph_count as GCN
    launches, real = [], _lib.launch

    def spy(name, *a, **k):
        launches.append(name)
        return real(name, *a, **k)

    def no_host(*a, **k):
        raise AssertionError("the host route was taken")
    monkeypatch.setattr(_lib, "launch", spy)
    if forbid_host:
        monkeypatch.setattr(GCN, "count_labels_host_f64", no_host)
    return launches


def _labels(items, route="device", on_device=False, **kw):
    from kp_gnn_amd import ops
    nptr, eptr, ei = GC.pack(items)
    ei_t = torch.from_numpy(ei).to(_dev()) if on_device else ei
    y = ops.count_labels(nptr, eptr, ei_t, _dev(), route=route, **kw)
    torch.cuda.synchronize()
    assert y.is_cuda and y.dtype == torch.float64 and tuple(y.shape) == (len(items), 5)
    return y.cpu()


def _launch_raw(items, ids, max_nodes, poison=float("nan")):
    """The graphs `ids` of the call `items` through ONE ops.count_labels_launch sized for max_nodes, into poisoned outputs:
    (out [G,5], status [G]) on the host, status -7 where nothing was written."""
    from kp_gnn_amd import _lib, ops
    dev = _dev()
    nptr, eptr, ei = GC.pack(items)
    G, E = len(items), int(eptr[-1])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)  # noqa: E731
    out = torch.full((G, 5), poison, dtype=torch.float64, device=dev)
    st = torch.full((G,), -7, dtype=torch.int32, device=dev)
    ids_d = t(np.asarray(ids), torch.int32)
    nbytes = len(ids) * int(_lib.load().kpgnn_count_labels_workspace_bytes(max_nodes))
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    ops.count_labels_launch(G, t(nptr, torch.int64), t(eptr, torch.int64), t(ei, torch.int64), E, ids_d, max_nodes, out, st, ws, nbytes)
    torch.cuda.synchronize()
    return out.cpu(), st.cpu()


def _bits(t):
    return t.contiguous().view(torch.int64)


def test_every_word_case_in_one_call(monkeypatch):
    g = golden()
    names = [k for k in g if g[k]["group"] == "word"]
    assert len(names) == 77
    launches = _spy(monkeypatch)
    y = _labels([(g[k]["n"], g[k]["ei"]) for k in names], on_device=True)
    assert launches == [LAUNCH, LAUNCH]                   # the wavefront class and the block class, nothing else
    for i, k in enumerate(names):
        GC.check_row(k, g[k]["n"], y[i].numpy(), g[k]["y"])


def test_every_large_case_in_one_call(monkeypatch):
    g = golden()
    names = [k for k in g if g[k]["group"] == "large"]
    assert len(names) == 23
    launches = _spy(monkeypatch)
    y = _labels([(g[k]["n"], g[k]["ei"]) for k in names])
    assert launches == [LAUNCH]                           # one run: the slabs of 23 graphs fit the default workspace
    for i, k in enumerate(names):
        GC.check_row(k, g[k]["n"], y[i].numpy(), g[k]["y"])


def test_host_group_mixed_with_served_graphs(monkeypatch):
    """A path of 2049 nodes (status 3, set without a launch), a directed 3-cycle (1) and a triangle with a self loop (2) take the
    host route inside the call that serves graphs of all three classes on the device."""
    from kp_gnn_amd import _lib
    g, rows = golden(), host_rows()
    names = ["petersen", "path2049", "grid8x8", "directed_c3", "cycle129", "triangle_loop", "gnp640_0.02", "k3_iso2"]
    items = [(g[k]["n"], g[k]["ei"]) for k in names]
    small = [i for i, k in enumerate(names) if g[k]["n"] <= 32]
    _, st = _launch_raw(items, small, 32)
    assert [int(st[i]) for i in small] == [0, _lib.CL_ASYMMETRIC, _lib.CL_SELF_LOOP, 0]
    launches = _spy(monkeypatch, forbid_host=False)
    y = _labels(items)
    assert launches == [LAUNCH] * 3
    for i, k in enumerate(names):
        GC.check_row(k, g[k]["n"], y[i].numpy(), g[k]["y"])
        if g[k]["group"] == "host":                         # host-filled: the host route's rows, bit for bit
            assert np.array_equal(y[i].numpy(), rows[k]), k
    alone = _labels([items[i] for i in (0, 2, 4, 6, 7)])   # the served ones are untouched by the fill
    assert torch.equal(_bits(alone), _bits(y[[0, 2, 4, 6, 7]]))
    assert np.array_equal(_labels(items, route="host").numpy(), np.stack([rows[k] for k in names]))


def test_too_large_for_the_launch_and_graph_ids_subsets():
    """A graph above the launch's max_nodes gets status 3 and no row; graphs outside graph_ids keep their poison."""
    from kp_gnn_amd import _lib
    g = golden()
    names = ["petersen", "grid8x8", "cycle129", "ladder32", "path65"]
    items = [(g[k]["n"], g[k]["ei"]) for k in names]
    for cap, want in ((32, [0, 3, 3, 0, 3]), (64, [0, 0, 3, 0, 3]), (100, [0, 0, 3, 0, 0]), (2048, [0, 0, 0, 0, 0])):
        out, st = _launch_raw(items, [0, 1, 2, 3, 4], cap)
        assert st.tolist() == want, cap
        for i, k in enumerate(names):
            if want[i] == 0:
                GC.check_row(f"{k} cap {cap}", g[k]["n"], out[i].numpy(), g[k]["y"])
            else:
                assert want[i] == _lib.CL_TOO_LARGE and bool(torch.isnan(out[i]).all())
    out, st = _launch_raw(items, [3, 0], 64)
    assert st.tolist() == [0, -7, -7, 0, -7] and bool(torch.isnan(out[[1, 2, 4]]).all()) and not bool(torch.isnan(out[[0, 3]]).any())


def test_bits_depend_on_the_graph_alone():
    """Bitwise equal rows for the same graph: alone and inside a 200-graph call; with its edge list shuffled and with
    duplicated edges; through the wavefront class, the block class and the large class (direct launches with a larger
    max_nodes)."""
    g = golden()
    rng = np.random.default_rng(8)
    picks = ["petersen", "ladder32", "grid8x8", "k64", "gnp300_0.5", "cycle129"]
    crowd = []
    while len(crowd) < 200 - len(picks):
        n = int(rng.integers(1, 90))
        crowd.append(sym(n, gnp(n, 0.3, rng)))
    where = np.sort(rng.permutation(200)[:len(picks)])
    items, it = [], iter(crowd)
    for i in range(200):
        items.append((g[picks[list(where).index(i)]]["n"], g[picks[list(where).index(i)]]["ei"]) if i in where else next(it))
    y200 = _labels(items)
    for slot, k in zip(where, picks):
        n, ei = g[k]["n"], g[k]["ei"]
        alone = _labels([(n, ei)])
        assert torch.equal(_bits(alone[0]), _bits(y200[slot])), k
        GC.check_row(k, n, alone[0].numpy(), g[k]["y"])
        shuffled = ei[:, rng.permutation(ei.shape[1])]
        doubled = np.concatenate([ei, ei[:, ::3], ei], axis=1)
        doubled = doubled[:, rng.permutation(doubled.shape[1])]
        again = _labels([(n, shuffled), (n, doubled)])
        assert torch.equal(_bits(again[0]), _bits(alone[0])) and torch.equal(_bits(again[1]), _bits(alone[0])), k
    small = [(g[k]["n"], g[k]["ei"]) for k in g if g[k]["group"] == "word" and g[k]["n"] <= 32]
    assert len(small) >= 20
    ids = np.arange(len(small))
    wave, st_w = _launch_raw(small, ids, 32)
    for cap in (33, 64, 65, 130):                           # the block class; the large class at W = 2 and W = 3 slabs
        other, st_o = _launch_raw(small, ids, cap)
        assert st_w.tolist() == st_o.tolist() == [0] * len(small)
        assert torch.equal(_bits(other), _bits(wave)), cap
    mid = [(g[k]["n"], g[k]["ei"]) for k in g if g[k]["group"] == "word" and g[k]["n"] > 32]
    block, st_b = _launch_raw(mid, np.arange(len(mid)), 64)
    large, st_l = _launch_raw(mid, np.arange(len(mid))[::-1].copy(), 200)
    assert st_b.tolist() == st_l.tolist() == [0] * len(mid) and torch.equal(_bits(block), _bits(large))


def test_tiny_workspace_gives_one_large_graph_per_launch(monkeypatch):
    g = golden()
    names = ["path65", "complete129", "gnp640_0.02", "cycle193", "k100_100"]
    items = [(g[k]["n"], g[k]["ei"]) for k in names]
    whole = _labels(items)
    launches = _spy(monkeypatch)
    tiny = _labels(items, workspace_bytes=1)
    assert launches == [LAUNCH] * len(names)
    assert torch.equal(_bits(tiny), _bits(whole))
    launches.clear()
    two = _labels(items, workspace_bytes=2 * 129 * 3 * 8)   # path65 and complete129 share a run; each of the others runs alone
    assert launches == [LAUNCH] * 4 and torch.equal(_bits(two), _bits(whole))


def test_endpoint_outside_the_graph_is_an_error_not_a_fault():
    from kp_gnn_amd import _lib
    ok = sym(40, cycle(40))
    c5 = sym(5, cycle(5))[1]
    big = sym(70, cycle(70))[1]
    for bad in ((5, np.concatenate([c5, [[4, 5], [5, 4]]], axis=1)), (5, np.concatenate([c5, [[-1, 0], [0, -1]]], axis=1)),
                (70, np.concatenate([big, [[3, 70], [70, 3]]], axis=1)), (70, np.concatenate([big, [[1 << 40, 0], [0, 1 << 40]]], axis=1))):
        items = [ok, ok, bad, ok]
        for cap in ((32, 64, 2048) if bad[0] <= 32 else (2048,)):
            out, st = _launch_raw(items, [2], cap)
            assert st.tolist() == [-7, -7, _lib.CL_ENDPOINT, -7] and bool(torch.isnan(out).all())
        with pytest.raises(ValueError, match="graph 2: .*endpoint"):
            _labels(items)
    y = _labels([ok])                                       # the device serves the next call as if nothing had happened
    assert y[0, :4].tolist() == [0.0, 0.0, 0.0, 0.0]


def test_no_graphs_and_empty_graphs(monkeypatch):
    from kp_gnn_amd import ops
    launches = _spy(monkeypatch)
    y = ops.count_labels(np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros((2, 0), np.int64), _dev(), route="device")
    assert y.is_cuda and y.dtype == torch.float64 and tuple(y.shape) == (0, 5) and launches == []
    g = golden()
    empty = (0, np.zeros((2, 0), np.int64))
    items = [empty, (g["petersen"]["n"], g["petersen"]["ei"]), empty, empty, (g["cycle129"]["n"], g["cycle129"]["ei"]), empty]
    y = _labels(items)
    for i in (0, 2, 3, 5):
        assert y[i].tolist() == [0.0] * 5
    GC.check_row("petersen", 10, y[1].numpy(), g["petersen"]["y"])
    GC.check_row("cycle129", 129, y[4].numpy(), g["cycle129"]["y"])
    out, st = _launch_raw(items, np.arange(6), 32)
    assert st.tolist() == [0, 0, 0, 0, 3, 0] and out[0].tolist() == [0.0] * 5


def test_labels_into_a_dataset_and_a_collated_batch():
    """ops.count_labels -> normalize_count_labels -> KHopDataset.from_graphs(y=...) -> collate: the batch's y rows are the
    normalised float64 labels of the selected graphs, bit for bit."""
    from kp_gnn_amd import graph_count as GCN, ops
    from kp_gnn_amd.dataset import KHopDataset
    rng = np.random.default_rng(40)
    items = []
    while len(items) < 24:
        n = int(rng.integers(10, 31))
        items.append(sym(n, gnp(n, 0.3, rng)))
    nptr, eptr, ei = GC.pack(items)
    y = ops.count_labels(nptr, eptr, ei, _dev(), route="device")
    yn = GCN.normalize_count_labels(y)
    assert yn.dtype == torch.float64 and yn.is_cuda and bool(torch.isfinite(yn[:, :4]).all())
    ds = KHopDataset.from_graphs(nptr, eptr, ei, None, _dev(), (3, 50, 6, 3, 50, 50, "spd"), y=yn)
    for ids in (rng.permutation(24)[:9], np.array([23, 0, 7, 7, 12])):
        b = ds.collate(ids)
        assert b.y.dtype == torch.float64 and tuple(b.y.shape) == (len(ids), 5)
        assert torch.equal(_bits(b.y), _bits(yn[torch.from_numpy(ids).to(_dev())]))
        t = GCN.count_targets(b.y, "cyc4")
        assert t.dtype == torch.float32 and tuple(t.shape) == (len(ids),) and torch.equal(t, b.y[:, 3].float())


def test_device_route_needs_a_gpu_device():
    from kp_gnn_amd import _lib, ops
    nptr, eptr, ei = GC.pack([sym(5, cycle(5))])
    with pytest.raises(_lib.KpgnnError, match="route='device'"):
        ops.count_labels(nptr, eptr, ei, "cpu", route="device")
    assert ops.COUNT_LABELS_AUTO in ("device", "host")
    auto = ops.count_labels(nptr, eptr, ei, _dev())
    assert torch.equal(auto.cpu()[:, :4], ops.count_labels(nptr, eptr, ei, _dev(), route="device").cpu()[:, :4])
