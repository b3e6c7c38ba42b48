"""CPU: the host side of the raw-graph dataset ops (kp_gnn_amd/ops_dataset.py, kp_gnn_amd/raw_graphs.py) - which entry
point runs over which graphs with which max_nodes and workspace, as literal tables, and what a malformed call raises.

The tables are written from the class limits of include/kpgnn.h (KPGNN_{RD,GL,CL,KHOP}_WAVE_NODES 32; KPGNN_RD_MAX_NODES 128;
KPGNN_{GL,KHOP}_MAX_NODES and KPGNN_CL_WORD_NODES 64; KPGNN_{RD_LARGE,KHOP_LARGE,CL}_MAX_NODES 2048) and the docstrings of the
ops: only the slab sizes come from the library's *_workspace_bytes entries.  tests/test_ops_dataset.py holds the launches of
real calls to the same tables."""
import contextlib

import numpy as np
import pytest
import torch

SIZES = (0, 1, 32, 33, 64, 65, 128, 129, 200, 300, 2048, 2049)      # graph g has SIZES[g] nodes
GPU_SIZES = (1, 32, 33, 64, 65, 128, 129, 200, 300, 0)              # the call of tests/test_ops_dataset.py
RD, RD_LARGE, GL, CL = "kpgnn_resistance_distance", "kpgnn_resistance_distance_large", "kpgnn_graph_labels", "kpgnn_count_labels"
DEV, LARGE = "kpgnn_khop_dev", "kpgnn_khop_large"
KINDS = ("rd_host", "rd_device", "graph_labels", "count_labels", "count_labels_ws1", "khop_host", "khop_device")


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


def cycle_edges(sizes):
    """Edges of a call of cycles (both directions; 2 nodes: one edge; fewer: none)."""
    return sum(2 * n if n > 2 else 2 * (n == 2) for n in sizes)


def slabs(sizes):
    """The three slab-size callbacks of a call of cycles of `sizes` nodes, from the library."""
    from kp_gnn_amd import _lib
    lib, N, E = _lib.load(), sum(sizes), cycle_edges(sizes)
    return (lambda cap: int(lib.kpgnn_rd_large_workspace_bytes(cap, 1)), lambda cap: int(lib.kpgnn_count_labels_workspace_bytes(cap)),
            lambda cap: int(lib.kpgnn_khop_large_workspace_bytes(N, E, cap)))


def both_passes(classes):
    return [(pair + pass_, ids, cap, nbytes) for pass_ in ("_count", "_fill") for pair, ids, cap, nbytes in classes]


def table(kind, sizes):
    """The launches of one call, in order: [(entry point, graph ids, max_nodes, workspace_bytes)]."""
    rd, cl, khl = slabs(sizes)
    dev_bytes = 16 * sum(sizes)                             # kpgnn_khop_dev: 2N int64
    if sizes == SIZES:
        return {
            "rd_host": [(RD, [0, 1, 2], 32, 0), (RD, [3, 4, 5, 6, 7, 8, 9, 10, 11], 128, 0)],
            # 2049 nodes: no class serves it, it rides the block class for its status 2
            "rd_device": [(RD, [0, 1, 2], 32, 0), (RD, [3, 4, 5, 6, 11], 128, 0), (RD_LARGE, [7, 8, 9, 10], 2048, 4 * rd(2048))],
            "graph_labels": [(GL, [0, 1, 2], 32, 0), (GL, [3, 4, 5, 6, 7, 8, 9, 10, 11], 64, 0)],
            # 2049 nodes: in no launch
            "count_labels": [(CL, [0, 1, 2], 32, 0), (CL, [3, 4], 64, 0), (CL, [5, 6, 7, 8, 9, 10], 2048, 6 * cl(2048))],
            "count_labels_ws1": [(CL, [0, 1, 2], 32, 0), (CL, [3, 4], 64, 0), (CL, [5], 65, cl(65)), (CL, [6], 128, cl(128)),
                                 (CL, [7], 129, cl(129)), (CL, [8], 200, cl(200)), (CL, [9], 300, cl(300)), (CL, [10], 2048, cl(2048))],
            "khop_host": both_passes([(DEV, [0, 1, 2], 32, dev_bytes), (DEV, [3, 4, 5, 6, 7, 8, 9, 10, 11], 64, dev_bytes)]),
            # 2049 nodes: in the large class, which is sized for 2048
            "khop_device": both_passes([(DEV, [0, 1, 2], 32, dev_bytes), (DEV, [3, 4], 64, dev_bytes),
                                        (LARGE, [5, 6, 7, 8, 9, 10, 11], 2048, khl(2048) // 8 * 8)]),
        }[kind]
    assert sizes == GPU_SIZES
    return {
        "rd_host": [(RD, [0, 1, 9], 32, 0), (RD, [2, 3, 4, 5, 6, 7, 8], 128, 0)],
        "rd_device": [(RD, [0, 1, 9], 32, 0), (RD, [2, 3, 4, 5], 128, 0), (RD_LARGE, [6, 7, 8], 300, 3 * rd(300))],
        "graph_labels": [(GL, [0, 1, 9], 32, 0), (GL, [2, 3, 4, 5, 6, 7, 8], 64, 0)],
        "count_labels": [(CL, [0, 1, 9], 32, 0), (CL, [2, 3], 64, 0), (CL, [4, 5, 6, 7, 8], 300, 5 * cl(300))],
        "count_labels_ws1": [(CL, [0, 1, 9], 32, 0), (CL, [2, 3], 64, 0), (CL, [4], 65, cl(65)), (CL, [5], 128, cl(128)),
                             (CL, [6], 129, cl(129)), (CL, [7], 200, cl(200)), (CL, [8], 300, cl(300))],
        "khop_host": both_passes([(DEV, [0, 1, 9], 32, dev_bytes), (DEV, [2, 3, 4, 5, 6, 7, 8], 64, dev_bytes)]),
        "khop_device": both_passes([(DEV, [0, 1, 9], 32, dev_bytes), (DEV, [2, 3], 64, dev_bytes),
                                    (LARGE, [4, 5, 6, 7, 8], 300, khl(300) // 8 * 8)]),
    }[kind]


def plan(kind, sizes):
    """The plan function's answer for the same call, ids as lists."""
    from kp_gnn_amd import ops_dataset as OD
    rd, cl, khl = slabs(sizes)
    nodes = np.asarray(sizes, dtype=np.int64)
    got = {"rd_host": lambda: OD.resistance_plan(nodes, "host"), "rd_device": lambda: OD.resistance_plan(nodes, "device", rd),
           "graph_labels": lambda: OD.graph_labels_plan(nodes), "count_labels": lambda: OD.count_labels_plan(nodes, cl),
           "count_labels_ws1": lambda: OD.count_labels_plan(nodes, cl, workspace_bytes=1),
           "khop_host": lambda: OD.khop_plan(nodes, "host"), "khop_device": lambda: OD.khop_plan(nodes, "device", khl)}[kind]()
    return [(entry, ids.tolist(), int(cap), int(nbytes)) for entry, ids, cap, nbytes in got]


@pytest.mark.parametrize("kind", KINDS)
def test_plan_equals_the_literal_table(built, kind):
    for sizes in (SIZES, GPU_SIZES):
        assert plan(kind, sizes) == table(kind, sizes), (kind, sizes)


def test_the_cap_rules(built):
    """The resistance, graph-label and k-hop classes are sized for their LARGEST MEMBER (at most the kernel's maximum, at
    least 1), the count-label classes for their bound; an empty class is no launch."""
    from kp_gnn_amd import ops_dataset as OD
    short = lambda p: [(entry, ids.tolist(), int(cap)) for entry, ids, cap, _ in p]  # noqa: E731
    cl = slabs((1,))[1]
    nodes = np.array([20, 0, 50, 1], dtype=np.int64)
    assert short(OD.resistance_plan(nodes)) == [(RD, [0, 1, 3], 20), (RD, [2], 50)]
    assert short(OD.graph_labels_plan(nodes)) == [(GL, [0, 1, 3], 20), (GL, [2], 50)]
    assert short(OD.khop_plan(nodes)) == [(DEV + "_count", [0, 1, 3], 20), (DEV + "_count", [2], 50),
                                          (DEV + "_fill", [0, 1, 3], 20), (DEV + "_fill", [2], 50)]
    assert short(OD.count_labels_plan(nodes, cl)) == [(CL, [0, 1, 3], 32), (CL, [2], 64)]
    empty = np.array([0], dtype=np.int64)
    assert short(OD.resistance_plan(empty)) == [(RD, [0], 1)] and short(OD.graph_labels_plan(empty)) == [(GL, [0], 1)]
    assert short(OD.khop_plan(empty, "device")) == [(DEV + "_count", [0], 1), (DEV + "_fill", [0], 1)]
    assert short(OD.count_labels_plan(empty, cl)) == [(CL, [0], 32)]
    over = np.array([2049], dtype=np.int64)                 # above every cap
    assert short(OD.resistance_plan(over)) == short(OD.resistance_plan(over, "device")) == [(RD, [0], 128)]
    assert short(OD.graph_labels_plan(over)) == [(GL, [0], 64)]
    assert short(OD.khop_plan(over)) == [(DEV + "_count", [0], 64), (DEV + "_fill", [0], 64)]
    assert short(OD.khop_plan(over, "device", lambda cap: 8)) == [(LARGE + "_count", [0], 65), (LARGE + "_fill", [0], 65)]
    assert list(OD.count_labels_plan(over, cl)) == []
    none = np.zeros(0, dtype=np.int64)
    assert list(OD.resistance_plan(none, "device")) == OD.graph_labels_plan(none) == OD.khop_plan(none, "device") == []
    assert list(OD.count_labels_plan(none, cl)) == []


def test_raw_graphs_is_the_validated_view():
    from kp_gnn_amd.raw_graphs import RawGraphs, i64
    g = RawGraphs(torch.tensor([0, 3, 3, 5], dtype=torch.int32), [0, 4, 4, 6], np.arange(12).reshape(2, 6), source=(1, 0, 1))
    assert (g.G, g.N, g.E) == (3, 5, 6) and g.nodes.tolist() == [3, 0, 2] and g.source.tolist() == [1, 0, 1]
    for a in (g.node_ptr, g.edge_ptr, g.source, g.nodes):
        assert a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]
    assert torch.is_tensor(g.edge_index) and tuple(g.edge_index.shape) == (2, 6) and g.edge_index.dtype == torch.int64
    assert np.array_equal(g.edge_index_host(), np.arange(12).reshape(2, 6))
    flat = RawGraphs([0, 5], [0, 6], torch.arange(12, dtype=torch.int32))          # a flat list reshapes to [2, E]
    assert tuple(flat.edge_index.shape) == (2, 6) and flat.edge_index.dtype == torch.int32 and flat.edge_index_host().dtype == np.int64
    assert flat.source is None and RawGraphs([0], [0], np.zeros((2, 0))).G == 0
    assert i64(torch.tensor([[1, 2], [3, 4]], dtype=torch.int16)).tolist() == [1, 2, 3, 4]


# what the parent commit raises, copied from its source (kp_gnn_amd/ops.py, graph_property.py, graph_count.py)
COUNT = "node_ptr and edge_ptr must both have G + 1 entries"
COUNT_SOURCE = "node_ptr and edge_ptr must have G + 1 entries and source G"
OFFSETS = "node_ptr / edge_ptr must start at 0 and not decrease"
WIDTH = "edge_index does not match edge_ptr"
K3 = (3, 50, 6, 3, 50, 50, "spd")


def _calls():
    """name -> (call(node_ptr, edge_ptr, edge_index), whether it takes a source)."""
    from kp_gnn_amd import graph_count as GCN, graph_property as GP, ops
    feat = lambda nptr: np.zeros(max(int(np.asarray(nptr).reshape(-1)[-1:].sum()), 0))  # noqa: E731
    src = lambda nptr: np.zeros(max(len(nptr) - 1, 0), dtype=np.int64)  # noqa: E731
    return {
        "ops.resistance_distance": lambda n, e, ei: ops.resistance_distance(n, e, ei, "cuda:0"),
        "ops.resistance_distance large": lambda n, e, ei: ops.resistance_distance(n, e, ei, "cuda:0", large="device"),
        "ops.graph_property_labels": lambda n, e, ei: ops.graph_property_labels(n, e, ei, feat(n), src(n), "cuda:0", route="device"),
        "ops.count_labels": lambda n, e, ei: ops.count_labels(n, e, ei, "cuda:0", route="device"),
        "ops.khop_transform": lambda n, e, ei: ops.khop_transform(n, e, ei, None, *K3, "cuda:0"),
        "ops.khop_transform large": lambda n, e, ei: ops.khop_transform(n, e, ei, None, *K3, "cuda:0", large="device"),
        "graph_property.labels_host_f64": lambda n, e, ei: GP.labels_host_f64(n, e, ei, feat(n), src(n)),
        "ops.graph_property_labels host": lambda n, e, ei: ops.graph_property_labels(n, e, ei, feat(n), src(n), "cpu", route="host"),
        "graph_count.count_labels_host_f64": lambda n, e, ei: GCN.count_labels_host_f64(n, e, ei),
        "ops.count_labels host": lambda n, e, ei: ops.count_labels(n, e, ei, "cpu", route="host"),
    }


MALFORMED = {       # (node_ptr, edge_ptr, columns of edge_index) -> the text; two graphs of 3 and 2 nodes, 4 and 2 edges when sound
    "edge_ptr one short": (([0, 3, 5], [0, 4], 4), COUNT),
    "edge_ptr one long": (([0, 3, 5], [0, 4, 6, 6], 6), COUNT),
    "node_ptr one short": (([0, 3], [0, 4, 6], 6), COUNT),
    "node_ptr empty": (([], [], 0), COUNT),
    "node_ptr starts at 1": (([1, 3, 5], [0, 4, 6], 6), OFFSETS),
    "edge_ptr starts at 1": (([0, 3, 5], [1, 4, 6], 6), OFFSETS),
    "node_ptr decreases": (([0, 5, 3], [0, 4, 6], 6), OFFSETS),
    "edge_ptr decreases": (([0, 3, 5], [0, 6, 4], 4), OFFSETS),
    "edge_index one column short": (([0, 3, 5], [0, 4, 6], 5), WIDTH),
    "edge_index one column long": (([0, 3, 5], [0, 4, 6], 7), WIDTH),
    "edge_index empty": (([0, 3, 5], [0, 4, 6], 0), WIDTH),
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_a_malformed_call_raises_what_it_always_raised(case):
    """Before any device is touched: these run without a GPU, the device ops on "cuda:0" included."""
    (node_ptr, edge_ptr, cols), text = MALFORMED[case]
    for name, call in _calls().items():
        want = COUNT_SOURCE if text == COUNT and "graph_property" in name else text
        for as_array in (False, True):
            n, e = (np.asarray(node_ptr, dtype=np.int64), np.asarray(edge_ptr, dtype=np.int64)) if as_array else (node_ptr, edge_ptr)
            with pytest.raises(ValueError) as err:
                call(n, e, torch.zeros((2, cols), dtype=torch.int64))
            assert str(err.value) == want, (name, case)


def test_the_source_count_is_checked_with_the_offsets():
    from kp_gnn_amd import graph_property as GP, ops
    ei = torch.zeros((2, 6), dtype=torch.int64)
    for call in (lambda s: GP.labels_host_f64([0, 3, 5], [0, 4, 6], ei, np.zeros(5), s),
                 lambda s: ops.graph_property_labels([0, 3, 5], [0, 4, 6], ei, np.zeros(5), s, "cuda:0", route="device")):
        for source in ([0], [0, 0, 0]):
            with pytest.raises(ValueError) as err:
                call(source)
            assert str(err.value) == COUNT_SOURCE


def test_two_defects_raise_in_the_order_they_always_did():
    """The device ops that name their keyword first still do; khop_transform and resistance_distance look at the graphs before
    the device, the two label ops at the device before the graphs."""
    from kp_gnn_amd import _lib, ops
    ei = torch.zeros((2, 6), dtype=torch.int64)
    bad = ([0, 3, 5], [0, 4], ei)
    with pytest.raises(ValueError, match="unknown large"):
        ops.resistance_distance(*bad, "cpu", large="auto")
    with pytest.raises(ValueError, match="unknown large"):
        ops.khop_transform(*bad, None, *K3, "cpu", large="auto")
    with pytest.raises(ValueError, match="unknown route"):
        ops.count_labels(*bad, "cpu", route="gpu")
    with pytest.raises(ValueError, match="unknown route"):
        ops.graph_property_labels(*bad, np.zeros(5), [0, 0], "cpu", route="gpu")
    with pytest.raises(ValueError, match="G \\+ 1 entries"):
        ops.resistance_distance(*bad, "cpu")
    with pytest.raises(ValueError, match="G \\+ 1 entries"):
        ops.khop_transform(*bad, None, *K3, "cpu")
    with pytest.raises(_lib.KpgnnError, match="route='device'"):
        ops.count_labels(*bad, "cpu", route="device")
    with pytest.raises(_lib.KpgnnError, match="route='device'"):
        ops.graph_property_labels(*bad, np.zeros(5), [0, 0], "cpu", route="device")
    good = ([0, 3, 5], [0, 4, 6], ei)
    with pytest.raises(ValueError, match="unknown kernel"):
        ops.khop_transform(*good, None, 3, 50, 6, 3, 50, 50, "sp", "cpu")
    with pytest.raises(_lib.KpgnnError, match="device route"):
        ops.khop_transform(*good, None, *K3, "cpu")
    with pytest.raises(_lib.KpgnnError, match="device route"):
        ops.resistance_distance(*good, "cpu")


def test_the_refusals_keep_each_ops_precedence():
    """refusals(): the entries in the op's order, each naming the FIRST graph with one of its codes; the rest is the host's."""
    from kp_gnn_amd import ops_dataset as OD
    status = np.array([0, 2, 4, 3, 1, 3], dtype=np.int32)
    assert OD.refusals(status, []).tolist() == [1, 2, 3, 4, 5]
    assert OD.refusals(np.zeros(3, dtype=np.int32), [((3,), lambda g, code: ValueError())]).size == 0
    with pytest.raises(IndexError, match="graph 3 code 3"):          # one entry per code: the entry decides (khop_transform)
        OD.refusals(status, [((3,), lambda g, code: IndexError(f"graph {g} code {code}")), ((4,), lambda g, code: ValueError("later"))])
    with pytest.raises(ValueError, match="graph 2 code 4"):          # one entry of several codes: the graph decides (graph labels)
        OD.refusals(status, [((3, 4, 5), lambda g, code: ValueError(f"graph {g} code {code}"))])


@contextlib.contextmanager
def launches_recorded():
    """Record (entry point, n_ids, max_nodes, workspace_bytes) of every _lib.launch inside the block."""
    from kp_gnn_amd import _lib
    seen, real = [], _lib.launch

    def spy(name, *args, **kw):
        d = args[1]._obj
        seen.append((name, int(d.n_ids), int(d.max_nodes), int(getattr(d, "workspace_bytes", 0))))
        return real(name, *args, **kw)
    _lib.launch = spy
    try:
        yield seen
    finally:
        _lib.launch = real


def test_the_launch_list_of_a_call_is_its_plan_without_a_gpu(built):
    """run_plan() hands the launch callback the plan's entries in order, the ids as int32, and ONE workspace of the largest
    entry's size to every entry that asks for bytes - on the host here, with a callback that only records.  A plan that is a
    generator is advanced to its workspace entries only after the entries before them are launched."""
    from kp_gnn_amd import ops_dataset as OD
    p = [(CL, np.array([0, 2]), 32, 0), (CL, np.array([1]), 65, 520), (CL, np.array([3, 4]), 300, 4800)]
    seen = []
    st = torch.tensor([0, 0, 1, 0, 2], dtype=torch.int32)
    status, todo = OD.run_plan(p, torch.device("cpu"), lambda *a: seen.append(a), st, [])
    assert [(e, ids.tolist(), ids.dtype, cap, nbytes) for e, ids, cap, _, nbytes in seen] == [
        (CL, [0, 2], torch.int32, 32, 0), (CL, [1], torch.int32, 65, 520), (CL, [3, 4], torch.int32, 300, 4800)]
    assert seen[0][3] is None and seen[1][3] is seen[2][3] and seen[1][3].numel() == 4800 and seen[1][3].dtype == torch.uint8
    assert torch.equal(status, st) and todo.tolist() == [2, 4]
    order = []

    def lazy():
        yield p[0]
        order.append("the runs are cut")
        yield from p[1:]
    OD.run_plan(lazy(), torch.device("cpu"), lambda entry, ids, *a: order.append(ids.tolist()), st, [])
    assert order == [[0, 2], "the runs are cut", [1], [3, 4]]
