"""CPU: the C ABI of the graph-property labels (include/kpgnn.h kpgnn_graph_labels, csrc/graph_labels.hip) - declaration, export,
binding, descriptor layout and the argument checks that run before any device call."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


def _header():
    return open(os.path.join(ROOT, "include", "kpgnn.h")).read()


def test_symbol_is_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(built[0])
    assert re.search(r"\bint\s+kpgnn_graph_labels\s*\(\s*const\s+kpgnn_graph_labels_desc\s*\*\s*\w*\s*,\s*kpgnn_stream_t", txt)
    assert re.search(r"#define\s+KPGNN_GL_MAX_NODES\s+64\b", txt) and _lib.GL_MAX_NODES == 64
    assert re.search(r"#define\s+KPGNN_GL_WAVE_NODES\s+32\b", txt) and _lib.GL_WAVE_NODES == 32
    assert hasattr(lib, "kpgnn_graph_labels")
    restype, argtypes = _lib.SIGNATURES["kpgnn_graph_labels"]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.GraphLabelsDesc) and len(argtypes) == 2
    assert _lib.load().kpgnn_abi_version() == 1           # a new entry point, the same ABI version
    enum = re.search(r"enum\s*\{([^}]*KPGNN_GL_OK[^}]*)\}", txt).group(1)
    got = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(",") if item.strip())}
    assert got == {"KPGNN_GL_OK": _lib.GL_OK, "KPGNN_GL_ASYMMETRIC": _lib.GL_ASYMMETRIC, "KPGNN_GL_TOO_LARGE": _lib.GL_TOO_LARGE,
                   "KPGNN_GL_ENDPOINT": _lib.GL_ENDPOINT, "KPGNN_GL_SELF_LOOP": _lib.GL_SELF_LOOP, "KPGNN_GL_SOURCE": _lib.GL_SOURCE}
    assert [got[k] for k in got] == [0, 1, 2, 3, 4, 5]


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_graph_labels_desc \{(.*?)\} kpgnn_graph_labels_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int64_t": 8, "int32_t": 4, "float": 4, "double": 8}
    names, want, total = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int64_t|int32_t|float|double)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for name in (s.strip() for s in m.group(3).split(",")):
            names.append(name)
            want[name] = 8 if m.group(2) else size[m.group(1)]
    assert names == ["G", "n_ids", "node_ptr", "edge_ptr", "edge_index", "E", "graph_ids", "max_nodes", "reserved", "features",
                     "source", "node_out", "graph_out", "status"]
    assert [f[0] for f in _lib.GraphLabelsDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.GraphLabelsDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == 4 * 4 + 10 * 8 == 96 and ctypes.sizeof(_lib.GraphLabelsDesc) == total
    # the first nine fields are kpgnn_rd_desc's, in its order
    assert names[:9] == [f[0] for f in _lib.RdDesc._fields_][:9]


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, aligned: never dereferenced
    d = _lib.GraphLabelsDesc()
    d.G, d.n_ids, d.E, d.max_nodes = 4, 4, 10, 24
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "features", "source", "node_out", "graph_out", "status"):
        setattr(d, f, a)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    fn = lib.kpgnn_graph_labels
    assert fn(None, None) == -1                          # NULL descriptor
    assert b"kpgnn_graph_labels: NULL descriptor" in lib.kpgnn_last_error()
    for bad in (dict(max_nodes=0), dict(max_nodes=-1), dict(G=-1), dict(n_ids=-1), dict(E=-1)):
        assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
        assert b"kpgnn_graph_labels" in lib.kpgnn_last_error(), bad
    assert fn(ctypes.byref(_desc(max_nodes=65)), None) == -3       # KPGNN_ELIMIT: beyond the cap, the host route's job
    assert b"cap of 64" in lib.kpgnn_last_error()
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "features", "source", "node_out", "graph_out", "status"):
        assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, f
        assert b"kpgnn_graph_labels: NULL" in lib.kpgnn_last_error(), f
    # n_ids == 0 (and G == 0) are valid and launch nothing: they return before any device call, whatever else the descriptor holds
    assert fn(ctypes.byref(_desc(n_ids=0)), None) == 0
    assert fn(ctypes.byref(_desc(n_ids=0, max_nodes=0, node_ptr=None, status=None)), None) == 0
    assert fn(ctypes.byref(_desc(G=0)), None) == 0
