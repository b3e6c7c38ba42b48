"""CPU: the C ABI of the resistance-distance kernel for graphs of up to 2048 nodes (include/kpgnn.h
kpgnn_resistance_distance_large / kpgnn_rd_large_workspace_bytes, csrc/resistance_large.hip) - declaration, export, binding,
descriptor layout, the workspace query and the argument checks that run before any device call - and the host-side pieces of
ops.resistance_distance(large=): the keyword's values and the cut of the large graphs into runs that fit a workspace.  The
fixture tests/golden/resistance_distance_large.pt (tests/golden/make_rd_large_golden.py) is held to the host route here; the
kernel is held to it in tests/test_resistance_large.py."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

from test_resistance_cabi import check_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["G", "n_ids", "node_ptr", "edge_ptr", "edge_index", "E", "graph_ids", "max_nodes", "reserved", "out", "status",
          "workspace", "workspace_bytes"]
NAMES = ("kpgnn_rd_large_workspace_bytes", "kpgnn_resistance_distance_large")


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


@functools.lru_cache(maxsize=None)
def golden_large():
    return torch.load(os.path.join(ROOT, "tests", "golden", "resistance_distance_large.pt"), weights_only=True)


def _header():
    return open(os.path.join(ROOT, "include", "kpgnn.h")).read()


def test_symbols_are_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(built[0])
    assert re.search(r"\bsize_t\s+%s\s*\(\s*int32_t\s+max_nodes\s*,\s*int32_t\s+n_ids\s*\)" % NAMES[0], txt)
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+kpgnn_rd_large_desc\s*\*" % NAMES[1], txt)
    for n in NAMES:
        assert hasattr(lib, n), n
    restype, argtypes = _lib.SIGNATURES[NAMES[0]]
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int32, ctypes.c_int32]
    restype, argtypes = _lib.SIGNATURES[NAMES[1]]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.RdLargeDesc) and len(argtypes) == 2
    assert _lib.load().kpgnn_abi_version() == 1
    assert _lib.RD_LARGE_MAX_NODES == 2048 and _lib.RD_MAX_NODES == 128
    assert re.search(r"#define\s+KPGNN_RD_LARGE_MAX_NODES\s+2048\b", txt) and re.search(r"#define\s+KPGNN_RD_MAX_NODES\s+128\b", txt)


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_rd_large_desc \{(.*?)\} kpgnn_rd_large_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int64_t": 8, "int32_t": 4, "size_t": 8}
    names, want, total = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int64_t|int32_t|size_t|float|void)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for name in (s.strip() for s in m.group(3).split(",")):
            names.append(name)
            want[name] = 8 if m.group(2) else size[m.group(1)]
    assert names == FIELDS
    assert [f[0] for f in _lib.RdLargeDesc._fields_] == names
    assert names[:11] == [f[0] for f in _lib.RdDesc._fields_]        # the fields of kpgnn_rd_desc, then the workspace
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.RdLargeDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == ctypes.sizeof(_lib.RdDesc) + 16 == 88
    assert ctypes.sizeof(_lib.RdLargeDesc) == total


def test_workspace_query(built):
    from kp_gnn_amd import _lib
    fn = _lib.load().kpgnn_rd_large_workspace_bytes
    for n in (1, 128, 129, 130, 160, 161, 300, 620, 1280, 2047, 2048):
        one = fn(n, 1)
        assert one >= n * (n | 1) * 8, n
        for ids in (0, 1, 2, 7, 100):
            assert fn(n, ids) == ids * one >= ids * n * (n | 1) * 8, (n, ids)
    sizes = [fn(n, 3) for n in range(1, 2049)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))               # monotone in max_nodes ...
    assert all(fn(300, i) < fn(300, i + 1) for i in range(0, 50))       # ... and in n_ids
    assert 34 * 10 ** 6 < fn(2048, 1) < 36 * 10 ** 6                    # one graph of 2048 nodes: 33.6 MB of matrix plus the panels
    assert fn(0, 1) == 0 and fn(2049, 1) == 0 and fn(128, -1) == 0      # nothing this kernel serves


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, 8-byte aligned: never dereferenced
    d = _lib.RdLargeDesc()
    d.G, d.n_ids, d.E, d.max_nodes = 3, 3, 10, 300
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status", "workspace"):
        setattr(d, f, a)
    d.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    fn = lib.kpgnn_resistance_distance_large
    assert fn(None, None) == -1
    assert b"resistance_distance_large" in lib.kpgnn_last_error()
    for bad in (dict(G=-1), dict(n_ids=-1), dict(E=-1), dict(max_nodes=0), dict(max_nodes=-5)):
        assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
        assert b"resistance_distance_large" in lib.kpgnn_last_error(), bad
    assert fn(ctypes.byref(_desc(G=0, n_ids=0)), None) == 0                  # no graphs: nothing to do, no launch
    assert fn(ctypes.byref(_desc(n_ids=0, graph_ids=None, workspace=None, workspace_bytes=0)), None) == 0
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status", "workspace"):
        assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, f
    assert b"workspace" in lib.kpgnn_last_error()
    assert fn(ctypes.byref(_desc(max_nodes=2049)), None) == _lib.ELIMIT == -3   # the cap is 2048 nodes
    assert b"2048" in lib.kpgnn_last_error()
    for n, ids in ((300, 3), (129, 1), (2048, 2)):
        need = lib.kpgnn_rd_large_workspace_bytes(n, ids)
        assert fn(ctypes.byref(_desc(max_nodes=n, n_ids=ids, workspace_bytes=need - 1)), None) == -1, (n, ids)
        assert str(need).encode() in lib.kpgnn_last_error()
    assert fn(ctypes.byref(_desc(workspace=0x10004)), None) == -1             # a double does not live there
    # the small kernel's entry point and descriptor did not move
    assert ctypes.sizeof(_lib.RdDesc) == 72
    assert lib.kpgnn_resistance_distance(ctypes.byref(_lib.RdDesc()), None) == 0


def test_large_keyword_values_are_checked_before_anything_else():
    from kp_gnn_amd import ops
    from kp_gnn_amd.dataset import KHopDataset
    from kp_gnn_amd.khop_transform import resistance_distance
    ei = torch.zeros((2, 0), dtype=torch.long)
    with pytest.raises(ValueError, match="large"):
        ops.resistance_distance([0, 3], [0, 0], ei, "cuda:0", large="auto")
    with pytest.raises(ValueError, match="large"):
        resistance_distance(types.SimpleNamespace(edge_index=ei, num_nodes=3), large="gpu")
    with pytest.raises(ValueError, match="rd_large"):
        KHopDataset.from_graphs([0, 3], [0, 0], ei, None, "cuda:0", (3, 50, 6, 3, 50, 50, "spd"), rd_large="auto")
    with pytest.raises(ValueError, match="rd_large"):
        KHopDataset.from_collated(types.SimpleNamespace(edge_index=ei), [0, 3], "cuda:0", rd_large=None)
    data = types.SimpleNamespace(edge_index=torch.tensor([[0, 1], [1, 0]]), num_nodes=2)
    assert resistance_distance(data, large="device").rd.reshape(-1).tolist() == [0.0, 1.0]     # a host list: the host route


def test_runs_of_large_graphs_fit_the_workspace(built):
    from kp_gnn_amd import _lib, ops_dataset
    slab = lambda cap: int(_lib.load().kpgnn_rd_large_workspace_bytes(cap, 1))  # noqa: E731
    nodes = np.array([5, 300, 129, 300, 40, 2048, 130, 257, 300, 300], dtype=np.int64)
    ids = np.flatnonzero(nodes > 128)
    for budget in (1, slab(300), 2 * slab(300), slab(2048), 1 << 30):
        runs = ops_dataset.workspace_runs(ids, nodes, slab, budget)
        assert np.concatenate([r[0] for r in runs]).tolist() == ids.tolist()          # every graph once, in call order
        for run_ids, cap, nbytes in runs:
            assert cap == int(nodes[run_ids].max()) and nbytes == len(run_ids) * slab(cap)
            assert nbytes <= budget or len(run_ids) == 1                                # a single graph always runs
    assert len(ops_dataset.workspace_runs(ids, nodes, slab, 1)) == ids.size
    assert len(ops_dataset.workspace_runs(ids, nodes, slab, 1 << 30)) == 1
    one300 = ops_dataset.workspace_runs(ids, nodes, slab, slab(300))
    assert all(len(r[0]) == 1 for r in one300 if 300 in nodes[r[0]].tolist())           # never two 300-node graphs in a launch


@pytest.mark.parametrize("name", sorted(golden_large()))
def test_host_route_against_the_large_fixture(name):
    from kp_gnn_amd.khop_transform import resistance_distance_host
    case = golden_large()[name]
    n = int(case["n"])
    got = resistance_distance_host(n, case["edge_index"].long())
    assert got[0] == 0.0
    check_bounds(got, case, name)
    check_bounds(got.astype(np.float32).astype(np.float64), case, name + " as float32")


def test_large_fixture_holds_the_cases_the_kernel_is_held_to():
    g = golden_large()
    assert {k: int(v["n"]) for k, v in g.items()} == {
        "path130": 130, "cycle160": 160, "star161": 161, "complete150": 150, "gnm191_dup_loop": 191,
        "two_paths_plus_isolated257": 257, "node0_isolated140": 140, "directed_cycle200": 200}
    for k, v in g.items():
        assert v["edge_index"].dtype == torch.int16 and v["ref32"].dtype == torch.float32 and v["ref64"].dtype == torch.float64, k
    ei = g["gnm191_dup_loop"]["edge_index"].long()
    assert ei.shape[1] == 2 * 382 + 2 + 1 and int((ei[0] == ei[1]).sum()) == 1          # the duplicate (both ways) and the loop
    pairs = [(int(u), int(v)) for u, v in ei.t()]
    assert len(set(pairs)) == len(pairs) - 2
    ei = g["directed_cycle200"]["edge_index"].long()
    assert {(int(u), int(v)) for u, v in ei.t()}.isdisjoint({(int(v), int(u)) for u, v in ei.t()})
    ei = g["node0_isolated140"]["edge_index"].long()
    assert int(ei.min()) == 1
    assert torch.equal(g["path130"]["ref64"].round(), torch.arange(130, dtype=torch.float64))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "resistance_distance_large.pt")) < 300 * 1024
