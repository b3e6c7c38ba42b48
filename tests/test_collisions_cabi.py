"""CPU: the C ABI of the collision count (include/kpgnn.h kpgnn_collision_count / kpgnn_collision_workspace_bytes,
csrc/collisions.hip) - declaration, export, binding, descriptor layout and the argument checks that run before any device call."""
import ctypes
import math
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
    assert re.search(r"\bint\s+kpgnn_collision_count\s*\(\s*const\s+kpgnn_collision_desc\s*\*\s*\w*\s*,\s*kpgnn_stream_t", txt)
    assert re.search(r"\bint64_t\s+kpgnn_collision_workspace_bytes\s*\(\s*int64_t\s+\w+\s*\)", txt)
    for n in ("kpgnn_collision_count", "kpgnn_collision_workspace_bytes"):
        assert hasattr(lib, n), n
    restype, argtypes = _lib.SIGNATURES["kpgnn_collision_count"]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.CollisionDesc) and len(argtypes) == 2
    assert _lib.SIGNATURES["kpgnn_collision_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64])
    assert _lib.load().kpgnn_abi_version() == 1           # new entry points, same ABI version


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_collision_desc \{(.*?)\} kpgnn_collision_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int64_t": 8, "int32_t": 4, "float": 4, "void": 8}
    names, want, total = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int64_t|int32_t|float|void)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for name in (s.strip() for s in m.group(3).split(",")):
            names.append(name)
            want[name] = 8 if m.group(2) else size[m.group(1)]
    assert names == ["N", "D", "eps", "x", "x_stride", "out", "workspace", "workspace_bytes"]
    assert [f[0] for f in _lib.CollisionDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.CollisionDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == 8 + 4 + 4 + 5 * 8 == 56
    assert ctypes.sizeof(_lib.CollisionDesc) == total


def _desc(N=300, D=16, eps=1e-10):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, 16-B aligned: never dereferenced
    d = _lib.CollisionDesc()
    d.N, d.D, d.eps = N, D, eps
    d.x = d.out = d.workspace = a
    d.x_stride = max(D, 1)
    d.workspace_bytes = max(_lib.load().kpgnn_collision_workspace_bytes(N), 16)
    return d


def test_workspace_bytes_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    ws = lib.kpgnn_collision_workspace_bytes
    assert ws(-1) == 0
    assert ws(0) == ws(1) == ws(128) == 16                # one block, one pair of 64-bit partials
    assert ws(129) == 3 * 16 and ws(1000) == 36 * 16       # 2 and 8 tile rows: 3 and 36 tiles of the upper triangle
    big = ws(128000)
    assert big == ws(10 ** 9) and big % 16 == 0 and 16 * 256 <= big <= 1 << 20      # the persistent grid is bounded


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    fn = lib.kpgnn_collision_count
    assert fn(None, None) == -1
    assert b"collision_count" in lib.kpgnn_last_error()
    for bad in (dict(N=-1), dict(D=0), dict(D=-3), dict(D=257), dict(eps=-1e-10), dict(eps=math.inf), dict(eps=-math.inf),
                dict(eps=math.nan)):
        assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
        assert b"collision_count" in lib.kpgnn_last_error(), bad
    for f in ("x", "out", "workspace"):
        d = _desc()
        setattr(d, f, None)
        assert fn(ctypes.byref(d), None) == -1, f
        assert b"collision_count" in lib.kpgnn_last_error()
    d = _desc()
    d.x_stride = 15
    assert fn(ctypes.byref(d), None) == -1
    assert b"collision_count" in lib.kpgnn_last_error()
    d = _desc(N=1000)
    d.workspace_bytes -= 1
    assert fn(ctypes.byref(d), None) == -1
    assert b"collision_count: workspace" in lib.kpgnn_last_error()
    d = _desc()
    d.workspace_bytes = -8
    assert fn(ctypes.byref(d), None) == -1
    # N == 0 is valid and launches nothing: it returns before any device call, on a machine without a device too
    assert fn(ctypes.byref(_desc(N=0)), None) == 0
    assert fn(ctypes.byref(_desc(N=0, eps=0.0)), None) == 0
