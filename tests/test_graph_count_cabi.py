"""CPU: the C ABI of the substructure-count labels (include/kpgnn.h kpgnn_count_labels, csrc/count_labels.hip) - declaration,
export, binding, descriptor layout, the workspace size and the argument checks that run before any device call."""
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


def test_symbols_are_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(built[0])
    assert re.search(r"\bint\s+kpgnn_count_labels\s*\(\s*const\s+kpgnn_count_labels_desc\s*\*\s*\w*\s*,\s*kpgnn_stream_t", txt)
    assert re.search(r"\bsize_t\s+kpgnn_count_labels_workspace_bytes\s*\(\s*int\s+\w*\s*\)", txt)
    assert re.search(r"#define\s+KPGNN_CL_WAVE_NODES\s+32\b", txt) and _lib.CL_WAVE_NODES == 32
    assert re.search(r"#define\s+KPGNN_CL_WORD_NODES\s+64\b", txt) and _lib.CL_WORD_NODES == 64
    assert re.search(r"#define\s+KPGNN_CL_MAX_NODES\s+2048\b", txt) and _lib.CL_MAX_NODES == 2048
    assert hasattr(lib, "kpgnn_count_labels") and hasattr(lib, "kpgnn_count_labels_workspace_bytes")
    restype, argtypes = _lib.SIGNATURES["kpgnn_count_labels"]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.CountLabelsDesc) and len(argtypes) == 2
    assert _lib.SIGNATURES["kpgnn_count_labels_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int])
    assert _lib.load().kpgnn_abi_version() == 1           # new entry points, the same ABI version
    enum = re.search(r"enum\s*\{([^}]*KPGNN_CL_OK[^}]*)\}", txt).group(1)
    got = {k.strip(): int(v) for k, v in (item.split("=") for item in enum.split(",") if item.strip())}
    assert got == {"KPGNN_CL_OK": _lib.CL_OK, "KPGNN_CL_ASYMMETRIC": _lib.CL_ASYMMETRIC, "KPGNN_CL_SELF_LOOP": _lib.CL_SELF_LOOP,
                   "KPGNN_CL_TOO_LARGE": _lib.CL_TOO_LARGE, "KPGNN_CL_ENDPOINT": _lib.CL_ENDPOINT}
    assert [got[k] for k in got] == [0, 1, 2, 3, 4]


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_count_labels_desc \{(.*?)\} kpgnn_count_labels_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int64_t": 8, "int32_t": 4, "double": 8, "size_t": 8, "void": None}
    names, want, total = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int64_t|int32_t|double|size_t|void)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for name in (s.strip() for s in m.group(3).split(",")):
            names.append(name)
            want[name] = 8 if m.group(2) else size[m.group(1)]
    assert names == ["G", "n_ids", "node_ptr", "edge_ptr", "edge_index", "E", "graph_ids", "max_nodes", "reserved", "out", "status",
                     "workspace", "workspace_bytes"]
    assert [f[0] for f in _lib.CountLabelsDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.CountLabelsDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == 4 * 4 + 9 * 8 == 88 and ctypes.sizeof(_lib.CountLabelsDesc) == total
    # the descriptor of kpgnn_resistance_distance_large, field for field (`out` is double [G,5] here)
    assert names == [f[0] for f in _lib.RdLargeDesc._fields_]


def test_workspace_bytes(built):
    from kp_gnn_amd import _lib
    fn = _lib.load().kpgnn_count_labels_workspace_bytes
    assert fn(2048) >= 2048 * 32 * 8
    sizes = [fn(n) for n in range(-2, 2200)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))                      # never decreases with max_nodes
    assert fn(64) == 0 and fn(65) >= 65 * 2 * 8 and fn(129) >= 129 * 3 * 8     # the one-word classes keep their rows in LDS
    for n in (65, 127, 128, 129, 1280, 2047, 2048):
        assert fn(n) >= n * ((n + 63) // 64) * 8 and fn(n) % 8 == 0, n


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, aligned: never dereferenced
    d = _lib.CountLabelsDesc()
    d.G, d.n_ids, d.E, d.max_nodes = 4, 4, 10, 24
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status"):
        setattr(d, f, a)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    fn = lib.kpgnn_count_labels
    assert fn(None, None) == -1                          # NULL descriptor
    assert b"kpgnn_count_labels: NULL descriptor" in lib.kpgnn_last_error()
    for bad in (dict(max_nodes=0), dict(max_nodes=-1), dict(G=-1), dict(n_ids=-1), dict(E=-1)):
        assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
        assert b"kpgnn_count_labels" in lib.kpgnn_last_error(), bad
    assert fn(ctypes.byref(_desc(max_nodes=2049)), None) == -3     # KPGNN_ELIMIT: beyond the cap, the host route's job
    assert b"cap of 2048" in lib.kpgnn_last_error()
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status"):
        for cap in (24, 64, 200):
            assert fn(ctypes.byref(_desc(**{f: None}, max_nodes=cap, workspace=0x10000, workspace_bytes=1 << 30)), None) == -1, f
            assert b"kpgnn_count_labels: NULL" in lib.kpgnn_last_error(), f
    # the large class needs its workspace: present, aligned and one slab per graph of the launch
    slab = lib.kpgnn_count_labels_workspace_bytes(200)
    for bad in (dict(workspace=None, workspace_bytes=4 * slab), dict(workspace=0x10004, workspace_bytes=4 * slab),
                dict(workspace=0x10000, workspace_bytes=4 * slab - 1), dict(workspace=0x10000, workspace_bytes=0)):
        assert fn(ctypes.byref(_desc(max_nodes=200, **bad)), None) == -1, bad
        assert b"kpgnn_count_labels" in lib.kpgnn_last_error() and b"workspace" in lib.kpgnn_last_error(), bad
    # n_ids == 0 (and G == 0) are valid and launch nothing: they return before any device call, whatever else the descriptor holds
    assert fn(ctypes.byref(_desc(n_ids=0)), None) == 0
    assert fn(ctypes.byref(_desc(n_ids=0, max_nodes=0, node_ptr=None, status=None)), None) == 0
    assert fn(ctypes.byref(_desc(G=0)), None) == 0
