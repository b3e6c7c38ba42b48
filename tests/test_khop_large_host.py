"""CPU: the C ABI of the K-hop pre-transform for graphs above 64 nodes (include/kpgnn.h kpgnn_khop_large_*,
csrc/khop_large.hip) - declaration, binding, the cap and the argument validation that answers without a GPU - and the
refusals of ops.khop_transform(large=) and KHopDataset.from_graphs(large=) that need none either."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("kpgnn_khop_large_count", "kpgnn_khop_large_fill")
N, E_IN, MAX_NODES = 20, 10, 100


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kpgnn.h")).read(), flags=re.S)


def test_symbols_are_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = _header()
    lib = ctypes.CDLL(built[0])
    for n in ENTRY:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+kpgnn_khop_dev_desc\s*\*" % n, txt), n
        assert hasattr(lib, n), n
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.KhopDevDesc) and len(argtypes) == 2
    assert re.search(r"\bsize_t\s+kpgnn_khop_large_workspace_bytes\s*\(\s*int64_t\s+N\s*,\s*int64_t\s+E_in\s*,\s*int32_t\s+max_nodes\s*\)", txt)
    assert hasattr(lib, "kpgnn_khop_large_workspace_bytes")
    restype, argtypes = _lib.SIGNATURES["kpgnn_khop_large_workspace_bytes"]
    assert restype is ctypes.c_size_t and argtypes == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]


def test_the_cap_covers_the_simulation_graphs_and_the_small_cap_did_not_move():
    from kp_gnn_amd import _lib
    txt = _header()
    cap = int(re.search(r"#define\s+KPGNN_KHOP_LARGE_MAX_NODES\s+(\d+)\b", txt).group(1))
    assert cap == _lib.KHOP_LARGE_MAX_NODES
    assert cap >= 1280 and cap & (cap - 1) == 0
    assert re.search(r"#define\s+KPGNN_KHOP_MAX_NODES\s+64\b", txt) and _lib.KHOP_MAX_NODES == 64


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, 8-byte aligned: never dereferenced
    d = _lib.KhopDevDesc()
    d.G, d.n_ids, d.N, d.E_in, d.max_nodes, d.E_out = 3, 3, N, E_IN, MAX_NODES, 40
    d.K, d.max_edge_attr_num, d.max_hop_num, d.max_edge_type, d.max_edge_count, d.max_distance_count, d.kernel = 4, 5, 3, 2, 4, 6, 0
    d.workspace_bytes = _lib.load().kpgnn_khop_large_workspace_bytes(N, E_IN, MAX_NODES)
    for f in ("graph_ids", "node_ptr", "edge_ptr", "edge_index", "edge_attr", "workspace", "status", "node_off", "out_edge_index",
              "out_edge_attr", "out_pe_attr", "out_pea", "out_pca", "out_batch"):
        setattr(d, f, a)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    need = lib.kpgnn_khop_large_workspace_bytes(N, E_IN, MAX_NODES)
    words = (MAX_NODES + 63) // 64
    assert need % 8 == 0 and need >= 8 * N + 8 * N * words          # the degrees and the any-hop masks at the least
    assert lib.kpgnn_khop_large_workspace_bytes(0, 0, 1) == 0
    assert lib.kpgnn_khop_large_workspace_bytes(N, E_IN, 2 * MAX_NODES) > need > lib.kpgnn_khop_large_workspace_bytes(N, 0, MAX_NODES)
    for name in ENTRY:
        fn = getattr(lib, name)
        assert fn(None, None) == -1
        assert name.encode() in lib.kpgnn_last_error()
        for bad in (dict(G=-1), dict(n_ids=-1), dict(N=-1), dict(E_in=-1), dict(E_in=2 ** 31), dict(max_nodes=0), dict(max_nodes=-5),
                    dict(K=0), dict(max_edge_attr_num=-1), dict(max_hop_num=-1), dict(max_edge_type=-1), dict(max_edge_count=-1),
                    dict(max_distance_count=-1), dict(kernel=2), dict(kernel=-1), dict(workspace_bytes=need - 1),
                    dict(workspace=0x10004)):
            assert fn(ctypes.byref(_desc(**bad)), None) == -1, (name, bad)
            assert name.encode() in lib.kpgnn_last_error(), (name, bad)
        assert fn(ctypes.byref(_desc(kernel=7)), None) == -1 and b"unknown kernel id 7" in lib.kpgnn_last_error()
        assert fn(ctypes.byref(_desc(G=0, n_ids=0)), None) == 0                  # no graphs: nothing to do, no launch
        assert fn(ctypes.byref(_desc(n_ids=0, graph_ids=None)), None) == 0       # no graphs for this launch
        for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "status", "workspace"):
            assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, (name, f)
        assert fn(ctypes.byref(_desc(max_nodes=_lib.KHOP_LARGE_MAX_NODES + 1)), None) == _lib.ELIMIT == -3
        assert str(_lib.KHOP_LARGE_MAX_NODES).encode() in lib.kpgnn_last_error()
    fill = lib.kpgnn_khop_large_fill
    for f in ("node_off", "out_edge_index", "out_edge_attr", "out_pea", "out_pca"):         # outputs the fill pass must have
        assert fill(ctypes.byref(_desc(**{f: None})), None) == -1, f
        assert b"kpgnn_khop_large_fill" in lib.kpgnn_last_error(), f
    assert fill(ctypes.byref(_desc(E_out=-1)), None) == -1


def test_unknown_values_of_large_are_refused(built):
    from kp_gnn_amd import ops
    from kp_gnn_amd.dataset import KHopDataset
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="large"):
        ops.khop_transform([0, 2], [0, 2], ei, None, 2, 5, 1, 1, 1, 1, "spd", "cpu", large="gpu")
    with pytest.raises(ValueError, match="large"):
        KHopDataset.from_graphs([0, 2], [0, 2], np.array([[0, 1], [1, 0]]), None, "cpu", (2, 5, 1, 1, 1, 1, "spd"), large="fast")
    assert KHopDataset.LARGE_AUTO in ("host", "device")
