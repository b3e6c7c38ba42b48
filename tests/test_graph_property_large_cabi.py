"""CPU: the C ABI of the graph-property labels' third size class (include/kpgnn.h kpgnn_graph_labels_large,
csrc/graph_labels.hip, W = 2) - declaration, export, binding, the argument checks that run before any device call - and the
launch plan of ops.graph_property_labels(large=)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GL, GL_LARGE = "kpgnn_graph_labels", "kpgnn_graph_labels_large"


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


def test_symbol_is_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kpgnn.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+kpgnn_graph_labels_large\s*\(\s*const\s+kpgnn_graph_labels_desc\s*\*\s*\w*\s*,\s*kpgnn_stream_t", txt)
    assert re.search(r"#define\s+KPGNN_GL_LARGE_MAX_NODES\s+128\b", txt) and _lib.GL_LARGE_MAX_NODES == 128
    assert re.search(r"#define\s+KPGNN_GL_MAX_NODES\s+64\b", txt) and _lib.GL_MAX_NODES == 64          # the small entry keeps its cap
    assert hasattr(ctypes.CDLL(built[0]), GL_LARGE)
    restype, argtypes = _lib.SIGNATURES[GL_LARGE]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.GraphLabelsDesc) and argtypes[1] is ctypes.c_void_p
    assert len(argtypes) == 2 and _lib.SIGNATURES[GL_LARGE] == _lib.SIGNATURES[GL]                     # one descriptor, no new struct
    assert _lib.load().kpgnn_abi_version() == 1           # a new entry point, the same ABI version


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, aligned: never dereferenced
    d = _lib.GraphLabelsDesc()
    d.G, d.n_ids, d.E, d.max_nodes = 4, 4, 10, 100
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "features", "source", "node_out", "graph_out", "status"):
        setattr(d, f, a)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    fn = lib.kpgnn_graph_labels_large
    assert fn(None, None) == -1                          # NULL descriptor
    assert b"kpgnn_graph_labels_large: NULL descriptor" in lib.kpgnn_last_error()
    for bad in (dict(max_nodes=0), dict(max_nodes=-1), dict(G=-1), dict(n_ids=-1), dict(E=-1)):
        assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad           # KPGNN_EINVAL
        assert b"kpgnn_graph_labels_large" in lib.kpgnn_last_error(), bad
    assert fn(ctypes.byref(_desc(max_nodes=129)), None) == -3            # KPGNN_ELIMIT: beyond the cap, the host route's job
    assert b"cap of 128" in lib.kpgnn_last_error()
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "features", "source", "node_out", "graph_out", "status"):
        assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, f
        assert b"kpgnn_graph_labels_large: NULL" in lib.kpgnn_last_error(), f
    # n_ids == 0 (and G == 0) are valid and launch nothing: they return before any device call, whatever else the descriptor holds
    assert fn(ctypes.byref(_desc(n_ids=0)), None) == 0
    assert fn(ctypes.byref(_desc(n_ids=0, max_nodes=0, node_ptr=None, status=None)), None) == 0
    assert fn(ctypes.byref(_desc(G=0)), None) == 0
    # the small entry is as it was: 65 is beyond ITS cap
    assert lib.kpgnn_graph_labels(ctypes.byref(_desc(max_nodes=65)), None) == -3 and b"cap of 64" in lib.kpgnn_last_error()


def test_the_plan_of_each_setting():
    from kp_gnn_amd import ops_dataset as OD
    short = lambda plan: [(entry, ids.tolist(), cap, nbytes) for entry, ids, cap, nbytes in plan]  # noqa: E731
    nodes = np.array([24, 64, 65, 128, 129], dtype=np.int64)
    host = [(GL, [0], 24, 0), (GL, [1, 2, 3, 4], 64, 0)]                 # 65, 128 and 129 ride the block class for their status 2
    assert short(OD.graph_labels_plan(nodes)) == short(OD.graph_labels_plan(nodes, "host")) == short(OD.graph_labels_plan(nodes, large="host")) == host
    # the large class is sized by its largest member; 129 stays in the block class
    assert short(OD.graph_labels_plan(nodes, "device")) == [(GL, [0], 24, 0), (GL, [1, 4], 64, 0), (GL_LARGE, [2, 3], 128, 0)]
    assert short(OD.graph_labels_plan(np.array([70, 3, 100, 66], dtype=np.int64), "device")) == [(GL, [1], 3, 0), (GL_LARGE, [0, 2, 3], 100, 0)]
    # nothing for the large class: the plan of "host"
    small = np.array([20, 0, 50, 1, 300], dtype=np.int64)
    assert short(OD.graph_labels_plan(small, "device")) == short(OD.graph_labels_plan(small))
    assert OD.graph_labels_plan(np.zeros(0, dtype=np.int64), "device") == []


def test_an_unknown_large_is_refused_before_anything_else():
    from kp_gnn_amd import ops
    for route in ("auto", "device", "host"):
        with pytest.raises(ValueError, match="large"):
            ops.graph_property_labels([0, 2], [0, 2], np.array([[0, 1], [1, 0]]), np.ones(2), [0], "cpu", route=route, large="gpu")
