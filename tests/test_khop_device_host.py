"""CPU: the C ABI of the device K-hop pre-transform (include/kpgnn.h kpgnn_khop_dev_*, csrc/khop_transform.hip) - declaration,
binding, descriptor layout and the argument validation that answers without a GPU - and the refusals of ops.khop_transform
and KHopDataset.from_graphs that need none either."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("kpgnn_khop_dev_count", "kpgnn_khop_dev_fill")
FIELDS = ["G", "n_ids", "graph_ids", "max_nodes", "reserved", "N", "node_ptr", "edge_ptr", "edge_index", "edge_attr", "E_in",
          "K", "max_edge_attr_num", "max_hop_num", "max_edge_type", "max_edge_count", "max_distance_count", "kernel", "reserved2",
          "workspace", "workspace_bytes", "status", "node_off", "E_out", "out_edge_index", "out_edge_attr", "out_pe_attr",
          "out_pea", "out_pca", "out_batch"]


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


def _header():
    return open(os.path.join(ROOT, "include", "kpgnn.h")).read()


def test_symbols_are_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(built[0])
    for n in ENTRY:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+kpgnn_khop_dev_desc\s*\*" % n, txt), n
        assert hasattr(lib, n), n
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.KhopDevDesc) and len(argtypes) == 2
    assert re.search(r"\bsize_t\s+kpgnn_khop_dev_workspace_bytes\s*\(\s*int64_t\s+N\s*\)", txt)
    assert _lib.SIGNATURES["kpgnn_khop_dev_workspace_bytes"][0] is ctypes.c_size_t
    for name, value in (("MAX_NODES", _lib.KHOP_MAX_NODES), ("WAVE_NODES", _lib.KHOP_WAVE_NODES), ("MAX_TYPE", _lib.KHOP_MAX_TYPE),
                        ("MAX_K", _lib.KHOP_MAX_K), ("MAX_T", _lib.KHOP_MAX_T), ("MAX_H", _lib.KHOP_MAX_H)):
        assert re.search(r"#define\s+KPGNN_KHOP_%s\s+%d\b" % (name, value), txt), name
    assert _lib.KHOP_MAX_NODES >= 64 and _lib.KHOP_MAX_TYPE >= 63
    assert (_lib.KHOP_MAX_K, _lib.KHOP_MAX_T, _lib.KHOP_MAX_H) >= (16, 8, 8)
    enum = re.search(r"enum\s*\{\s*KPGNN_KHOP_OK\s*=\s*0,\s*KPGNN_KHOP_TOO_LARGE\s*=\s*1,\s*KPGNN_KHOP_RANGE\s*=\s*2,\s*"
                     r"KPGNN_KHOP_ENDPOINT\s*=\s*3,\s*KPGNN_KHOP_TYPE\s*=\s*4,\s*KPGNN_KHOP_SHAPE\s*=\s*5\s*\}", txt)
    assert enum and (_lib.KHOP_OK, _lib.KHOP_TOO_LARGE, _lib.KHOP_RANGE, _lib.KHOP_ENDPOINT, _lib.KHOP_TYPE,
                     _lib.KHOP_SHAPE) == (0, 1, 2, 3, 4, 5)


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_khop_dev_desc \{(.*?)\} kpgnn_khop_dev_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int64_t": 8, "int32_t": 4, "size_t": 8}
    names, want, total = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int64_t|int32_t|size_t|void)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for name in (s.strip() for s in m.group(3).split(",")):
            names.append(name)
            want[name] = 8 if m.group(2) else size[m.group(1)]
    assert names == FIELDS
    assert [f[0] for f in _lib.KhopDevDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.KhopDevDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert ctypes.sizeof(_lib.KhopDevDesc) == total


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, 8-byte aligned: never dereferenced
    d = _lib.KhopDevDesc()
    d.G, d.n_ids, d.N, d.E_in, d.max_nodes, d.E_out = 3, 3, 20, 10, 32, 40
    d.K, d.max_edge_attr_num, d.max_hop_num, d.max_edge_type, d.max_edge_count, d.max_distance_count, d.kernel = 4, 5, 3, 2, 4, 6, 0
    d.workspace_bytes = 16 * 20
    for f in ("graph_ids", "node_ptr", "edge_ptr", "edge_index", "edge_attr", "workspace", "status", "node_off", "out_edge_index",
              "out_edge_attr", "out_pe_attr", "out_pea", "out_pca", "out_batch"):
        setattr(d, f, a)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    assert lib.kpgnn_khop_dev_workspace_bytes(20) == 16 * 20 and lib.kpgnn_khop_dev_workspace_bytes(0) == 0
    for name in ENTRY:
        fn = getattr(lib, name)
        assert fn(None, None) == -1
        assert name.encode() in lib.kpgnn_last_error()
        for bad in (dict(G=-1), dict(n_ids=-1), dict(N=-1), dict(E_in=-1), dict(E_in=2 ** 31), dict(max_nodes=0), dict(max_nodes=-5),
                    dict(K=0), dict(max_edge_attr_num=-1), dict(max_hop_num=-1), dict(max_edge_type=-1), dict(max_edge_count=-1),
                    dict(max_distance_count=-1), dict(kernel=2), dict(kernel=-1), dict(workspace_bytes=16 * 20 - 1),
                    dict(workspace=0x10004)):
            assert fn(ctypes.byref(_desc(**bad)), None) == -1, (name, bad)
            assert name.encode() in lib.kpgnn_last_error(), (name, bad)
        assert fn(ctypes.byref(_desc(kernel=7)), None) == -1 and b"unknown kernel id 7" in lib.kpgnn_last_error()
        assert fn(ctypes.byref(_desc(G=0, n_ids=0)), None) == 0                  # no graphs: nothing to do, no launch
        assert fn(ctypes.byref(_desc(n_ids=0, graph_ids=None)), None) == 0       # no graphs for this class
        for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "status", "workspace"):
            assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, (name, f)
        assert fn(ctypes.byref(_desc(max_nodes=_lib.KHOP_MAX_NODES + 1)), None) == _lib.ELIMIT == -3
        assert str(_lib.KHOP_MAX_NODES).encode() in lib.kpgnn_last_error()
    fill = lib.kpgnn_khop_dev_fill
    for f in ("node_off", "out_edge_index", "out_edge_attr", "out_pea", "out_pca"):         # outputs the fill pass must have
        assert fill(ctypes.byref(_desc(**{f: None})), None) == -1, f
        assert b"kpgnn_khop_dev_fill" in lib.kpgnn_last_error(), f
    assert fill(ctypes.byref(_desc(E_out=-1)), None) == -1


def test_ops_khop_transform_refuses_a_cpu_device_and_bad_arguments(built):
    from kp_gnn_amd import KpgnnError, ops
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(KpgnnError, match="khop_batch"):
        ops.khop_transform([0, 2], [0, 2], ei, None, 2, 5, 1, 1, 1, 1, "spd", "cpu")
    with pytest.raises(ValueError):
        ops.khop_transform([0, 2], [0, 2], ei, None, 2, 5, 1, 1, 1, 1, "bfs", "cpu")
    with pytest.raises(ValueError):
        ops.khop_transform([0, 2], [0, 3], ei, None, 2, 5, 1, 1, 1, 1, "spd", "cpu")
    with pytest.raises(ValueError):
        ops.khop_transform([0, 2], [0, 2], ei, torch.tensor([2]), 2, 5, 1, 1, 1, 1, "spd", "cpu")


def test_from_graphs_refuses_an_unknown_route_and_a_cpu_device(built):
    from kp_gnn_amd import KpgnnError
    from kp_gnn_amd.dataset import KHopDataset
    ei = np.array([[0, 1], [1, 0]])
    with pytest.raises(ValueError, match="route"):
        KHopDataset.from_graphs([0, 2], [0, 2], ei, None, "cpu", (2, 5, 1, 1, 1, 1, "spd"), route="fast")
    with pytest.raises(KpgnnError, match="khop_batch"):
        KHopDataset.from_graphs([0, 2], [0, 2], ei, None, "cpu", (2, 5, 1, 1, 1, 1, "spd"), route="device")
