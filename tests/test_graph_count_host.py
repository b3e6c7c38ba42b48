"""CPU: the float64 host route of the substructure-count labels (kp_gnn_amd/graph_count.py) against what the reference's
GraphCountDataset.process recorded in tests/golden/graph_count.npz, against closed forms, against the reduced integer form the
kernel uses, and normalize_count_labels / count_targets against a direct torch restatement of train_structure_counting.py."""
import functools
from math import comb

import numpy as np
import pytest
import torch

import graph_count_cases as GC
from graph_property_cases import complete, cycle, served_cases, sym


@functools.lru_cache(maxsize=None)
def golden():
    """name -> dict(group, n, ei, y): the fixture, the edge lists of graphs above 64 nodes regenerated from the cases module
    (and checked against the recorded node and edge counts)."""
    z = np.load(GC.GOLDEN)
    out = {}
    for group, cases in GC.groups():
        names = z[group + "/names"].tolist()
        assert names == list(cases), group
        for k in names:
            n, ei = cases[k]
            assert n == int(z[f"{k}/n"]) and ei.shape[1] == int(z[f"{k}/edges"]), k
            if n <= 64:
                assert np.array_equal(ei, z[f"{k}/ei"].astype(np.int64)), k
            out[k] = dict(group=group, n=n, ei=ei, y=z[f"{k}/y"])
    return out


@functools.lru_cache(maxsize=None)
def host_rows():
    """The host route on every fixture graph, computed once: name -> y [5]."""
    from kp_gnn_amd import graph_count as GCN
    g = golden()
    y = GCN.count_labels_host_f64(*GC.pack([(c["n"], c["ei"]) for c in g.values()]))
    return dict(zip(g, y))


def test_fixture_has_the_cases():
    g = golden()
    by = {grp: [k for k in g if g[k]["group"] == grp] for grp in ("word", "large", "host")}
    assert len(by["word"]) == 53 + 24 and max(g[k]["n"] for k in by["word"]) == 64
    assert len(by["large"]) == 18 + 5 and min(g[k]["n"] for k in by["large"]) == 65 and max(g[k]["n"] for k in by["large"]) == 2048
    assert by["host"] == ["path2049", "directed_c3", "triangle_loop"]
    for k in g:
        assert g[k]["y"].dtype == np.float64 and g[k]["y"].shape == (5,)
    # the literal expressions on a directed list and on a self loop are not integers: the reason these go to the host route
    assert g["directed_c3"]["y"][0] == 0.5 and g["triangle_loop"]["y"][0] != int(g["triangle_loop"]["y"][0])


def test_host_route_against_the_reference():
    g, rows = golden(), host_rows()
    for k, c in g.items():
        GC.check_row(k, c["n"], rows[k], c["y"])


def test_closed_forms():
    from kp_gnn_amd import graph_count as GCN
    for n in (3, 4, 5, 9, 33, 64, 65):
        y = GCN.labels_one(*sym(n, complete(n)))
        assert y[:4].tolist() == [comb(n, 3), n * comb(n - 1, 2) * (n - 3), n * comb(n - 1, 3), 3 * comb(n, 4)], n
    for n in (5, 6, 31, 64, 129):
        assert GCN.labels_one(*sym(n, cycle(n)))[:4].tolist() == [0, 0, 0, 0], n
    for a, b in ((2, 3), (5, 5), (32, 32), (100, 100)):
        y = GCN.labels_one(*sym(a + b, [(i, a + j) for i in range(a) for j in range(b)]))
        assert y[0] == 0 and y[3] == comb(a, 2) * comb(b, 2), (a, b)
    y = GCN.labels_one(*served_cases()["petersen"])
    assert y[[0, 1, 2, 3]].tolist() == [0, 0, 10, 0]
    assert GCN.labels_one(0, np.zeros((2, 0), np.int64)).tolist() == [0.0] * 5
    assert GCN.labels_one(1, np.zeros((2, 0), np.int64)).tolist() == [0.0] * 5


def test_reduced_integer_form_equals_the_literal_form():
    """What the kernel computes (popcounts, int64 sums, one exp per node) is the reference's expression on every symmetric
    loop-free case; the host group's directed list and self loop are exactly where it is not."""
    g, rows = golden(), host_rows()
    for k, c in g.items():
        if k in ("directed_c3", "triangle_loop"):
            continue
        GC.check_row(k, c["n"], GC.reduced_form(c["n"], c["ei"]), rows[k])
    for k in ("directed_c3", "triangle_loop"):
        assert not (GC.reduced_form(g[k]["n"], g[k]["ei"])[:4] == g[k]["y"][:4]).all(), k


def test_duplicates_and_order_do_not_matter():
    from kp_gnn_amd import graph_count as GCN
    n, ei = served_cases()["gnp64_0.2"]
    rng = np.random.default_rng(3)
    again = np.concatenate([ei, ei[:, :40]], axis=1)[:, rng.permutation(ei.shape[1] + 40)]
    assert np.array_equal(GCN.labels_one(n, again)[:4], GCN.labels_one(n, ei)[:4])


def test_normalize_and_targets():
    from kp_gnn_amd import graph_count as GCN
    assert GCN.COUNT_LABELS == ("tri", "tailed", "star", "cyc4", "cus")
    g = golden()
    names = [k for k in g if g[k]["group"] == "word"]
    y = torch.from_numpy(np.stack([g[k]["y"] for k in names]))
    got = GCN.normalize_count_labels(y)
    assert got.dtype == torch.float64 and torch.equal(got, y / y.std(0))
    assert torch.equal(got, y / y.std(0, unbiased=True)) and not torch.equal(got, y / y.std(0, unbiased=False))
    for task, name in enumerate(GCN.COUNT_LABELS):
        t = GCN.count_targets(got, task)
        assert t.dtype == torch.float32 and t.shape == (len(names),) and t.is_contiguous()
        assert torch.equal(t, got[:, task].float()) and torch.equal(t, GCN.count_targets(got, name))
    flat = torch.zeros((4, 5), dtype=torch.float64)
    assert bool(torch.isnan(GCN.normalize_count_labels(flat)).all())             # 0 / 0, as in the reference
    for bad in (5, -1):
        with pytest.raises(ValueError):
            GCN.count_targets(got, bad)


def test_host_tensor_route_and_refusals():
    from kp_gnn_amd import graph_count as GCN, ops
    g = golden()
    items = [(g[k]["n"], g[k]["ei"]) for k in ("petersen", "directed_c3", "k3_iso2")]
    nptr, eptr, ei = GC.pack(items)
    y = GCN.count_labels_host(nptr, eptr, torch.from_numpy(ei))
    assert y.dtype == torch.float64 and tuple(y.shape) == (3, 5) and y.device.type == "cpu"
    assert np.array_equal(y.numpy(), GCN.count_labels_host_f64(nptr, eptr, ei))
    assert torch.equal(ops.count_labels(nptr, eptr, ei, "cpu", route="host"), y)
    only = GCN.count_labels_host_f64(nptr, eptr, ei, graphs=[2])
    assert np.array_equal(only[2], y[2].numpy()) and not only[:2].any()
    for bad, at in ((np.asarray([[0, 10], [1, 0]]), 0), (np.asarray([[0, -1], [1, 0]]), 0)):
        bad_items = [items[2], (10, bad.astype(np.int64))]
        with pytest.raises(ValueError, match="graph 1"):
            GCN.count_labels_host_f64(*GC.pack(bad_items))
    with pytest.raises(ValueError):
        GCN.count_labels_host_f64(nptr[:-1], eptr, ei)
    with pytest.raises(ValueError):
        GCN.count_labels_host_f64(nptr, eptr, ei[:, :-1])
    with pytest.raises(ValueError):
        ops.count_labels(nptr, eptr, ei, "cpu", route="nowhere")
