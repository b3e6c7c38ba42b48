"""CPU: the C ABI of the resistance-distance kernel (include/kpgnn.h kpgnn_resistance_distance, csrc/resistance.hip) -
declaration, export, binding, descriptor layout, the argument checks that run before any device call - and the host route
khop_transform.resistance_distance_host / the drop-in resistance_distance(data) against tests/golden/resistance_distance.pt
(the reference's own output ref32 and a float64 pinv of the same Laplacian ref64, tests/golden/make_rd_golden.py).

Bounds.  (1) |host - ref64| <= 1 float32 ulp of |ref64| + 1e-9: both sides are float64 computations at condition numbers below
1e4, so 1e-9 is orders above their rounding; where ref64 is noise around 0 (isolated nodes, y = 0) the absolute term decides.
(2) |host - ref32| <= |ref32 - ref64| + 1 ulp: never further from the reference than the reference is from float64."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["G", "n_ids", "node_ptr", "edge_ptr", "edge_index", "E", "graph_ids", "max_nodes", "reserved", "out", "status"]


@pytest.fixture(scope="module")
def built():
    from kp_gnn_amd import build
    return build.build_all()


@functools.lru_cache(maxsize=None)
def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "resistance_distance.pt"), weights_only=True)


def ulp32(x):
    """One float32 ulp at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def check_bounds(got, case, name):
    """Both bounds of the module docstring for `got` (float64 array [n]) on one fixture case."""
    r64, r32 = case["ref64"].numpy(), case["ref32"].double().numpy()
    e64, e32 = np.abs(got - r64), np.abs(got - r32)
    assert bool((e64 <= ulp32(r64) + 1e-9).all()), (name, float(e64.max()))
    assert bool((e32 <= np.abs(r32 - r64) + ulp32(r32)).all()), (name, float(e32.max()))


def _header():
    return open(os.path.join(ROOT, "include", "kpgnn.h")).read()


def test_symbol_is_declared_exported_and_bound(built):
    from kp_gnn_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = ctypes.CDLL(built[0])
    n = "kpgnn_resistance_distance"
    assert re.search(r"\bint\s+%s\s*\(\s*const\s+kpgnn_rd_desc\s*\*" % n, txt)
    assert hasattr(lib, n)
    restype, argtypes = _lib.SIGNATURES[n]
    assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.RdDesc) and len(argtypes) == 2
    assert _lib.load().kpgnn_abi_version() == 1
    assert (_lib.RD_MAX_NODES, _lib.RD_WAVE_NODES) == (128, 32)
    assert re.search(r"#define\s+KPGNN_RD_MAX_NODES\s+128\b", txt) and re.search(r"#define\s+KPGNN_RD_WAVE_NODES\s+32\b", txt)
    enum = re.search(r"enum\s*\{\s*KPGNN_RD_OK\s*=\s*0,\s*KPGNN_RD_ASYMMETRIC\s*=\s*1,\s*KPGNN_RD_TOO_LARGE\s*=\s*2,\s*"
                     r"KPGNN_RD_PIVOT\s*=\s*3,\s*KPGNN_RD_RANGE\s*=\s*4\s*\}", txt)
    assert enum and (_lib.RD_OK, _lib.RD_ASYMMETRIC, _lib.RD_TOO_LARGE, _lib.RD_PIVOT, _lib.RD_RANGE) == (0, 1, 2, 3, 4)


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_rd_desc \{(.*?)\} kpgnn_rd_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"int64_t": 8, "int32_t": 4}
    names, want, total = [], {}, 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(int64_t|int32_t|float)\s*(\*?)\s*(.*)$", decl)
        assert m, decl
        for name in (s.strip() for s in m.group(3).split(",")):
            names.append(name)
            want[name] = 8 if m.group(2) else size[m.group(1)]
    assert names == FIELDS
    assert [f[0] for f in _lib.RdDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.RdDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == 4 + 4 + 3 * 8 + 8 + 8 + 4 + 4 + 8 + 8 == 72
    assert ctypes.sizeof(_lib.RdDesc) == total


def _desc(**kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL: never dereferenced
    d = _lib.RdDesc()
    d.G, d.n_ids, d.E, d.max_nodes = 3, 3, 10, 32
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status"):
        setattr(d, f, a)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    fn = lib.kpgnn_resistance_distance
    assert fn(None, None) == -1
    assert b"resistance_distance" in lib.kpgnn_last_error()
    for bad in (dict(G=-1), dict(n_ids=-1), dict(E=-1), dict(max_nodes=0), dict(max_nodes=-5)):
        assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
        assert b"resistance_distance" in lib.kpgnn_last_error(), bad
    assert fn(ctypes.byref(_desc(G=0, n_ids=0)), None) == 0                  # no graphs: nothing to do, no launch
    assert fn(ctypes.byref(_desc(n_ids=0, graph_ids=None)), None) == 0       # no graphs for this class
    for f in ("node_ptr", "edge_ptr", "edge_index", "graph_ids", "out", "status"):
        assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, f
    assert fn(ctypes.byref(_desc(max_nodes=129)), None) == _lib.ELIMIT == -3   # the cap is 128 nodes
    assert b"128" in lib.kpgnn_last_error()


@pytest.mark.parametrize("name", sorted(golden()))
def test_host_route_against_the_fixture(name):
    from kp_gnn_amd.khop_transform import resistance_distance_host
    case = golden()[name]
    n = int(case["n"])
    got = resistance_distance_host(n, case["edge_index"].long())
    assert got.dtype == np.float64 and got.shape == (n,)
    assert got[0] == 0.0                                 # (a + a - a) - a, in that order
    check_bounds(got, case, name)
    check_bounds(got.astype(np.float32).astype(np.float64), case, name + " as float32")


def test_fixture_holds_the_cases_the_kernel_is_held_to():
    g = golden()
    assert len(g) == 80 and sum(k.startswith("mol") for k in g) == 64
    assert {int(g["path%d" % n]["n"]) for n in (32, 33, 64, 65, 128, 129)} == {32, 33, 64, 65, 128, 129}
    assert torch.equal(g["path128"]["ref64"].round(), torch.arange(128, dtype=torch.float64))
    ei = g["self_loop"]["edge_index"]
    assert bool((ei[0] == ei[1]).any())                                   # the self-loop is in the list the reference saw ...
    no_loop = ei[:, ei[0] != ei[1]].long()
    from kp_gnn_amd.khop_transform import resistance_distance_host
    check_bounds(resistance_distance_host(4, no_loop), g["self_loop"], "self-loop ignored")    # ... and it ignored it
    ei = g["directed_cycle3"]["edge_index"].long()
    assert {(int(u), int(v)) for u, v in ei.t()} != {(int(v), int(u)) for u, v in ei.t()}      # a directed list


def test_host_route_rejects_an_endpoint_outside_the_graph():
    from kp_gnn_amd.khop_transform import resistance_distance_host
    with pytest.raises(IndexError):
        resistance_distance_host(3, torch.tensor([[0, 3], [3, 0]]))
    assert resistance_distance_host(0, torch.zeros((2, 0), dtype=torch.long)).shape == (0,)


def test_drop_in_on_a_cpu_data_object():
    """The reference's contract (data_utils.py:280-303): data.rd [n,1] float32 from data.edge_index / data.num_nodes."""
    from kp_gnn_amd.khop_transform import resistance_distance
    case = golden()["cycle37"]
    data = types.SimpleNamespace(edge_index=case["edge_index"].long(), num_nodes=37, x=torch.zeros(37, 1))
    out = resistance_distance(data)
    assert out is data and data.rd.dtype == torch.float32 and tuple(data.rd.shape) == (37, 1) and not data.rd.is_cuda
    check_bounds(data.rd.reshape(-1).double().numpy(), case, "drop-in")
    data = types.SimpleNamespace(edge_index=golden()["path5"]["edge_index"].long(), num_nodes=None, x=torch.zeros(5, 3))
    assert resistance_distance(data).rd.reshape(-1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]       # num_nodes from x, as PyG has it
