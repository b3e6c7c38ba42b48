"""CPU: the C ABI of the max graph readout (include/kpgnn.h kpgnn_segment_max_fwd / _bwd, csrc/pool_max.hip) - declaration,
export, binding, descriptor layout and the argument checks that run before any device call - and the CPU route of
body.global_max_pool, which stays the framework's scatter (even split of a tied column's gradient)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kpgnn_segment_max_fwd", "kpgnn_segment_max_bwd")


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
    for n in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+kpgnn_pool_max_desc\s*\*" % n, txt), n
        assert hasattr(lib, n), n
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.PoolMaxDesc) and len(argtypes) == 2


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_pool_max_desc \{(.*?)\} kpgnn_pool_max_desc;", _header(), flags=re.S).group(1)
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
    assert names == ["N", "G", "D", "graph_ptr", "batch", "x", "x_stride", "out", "arg", "gout", "gx", "gx_stride", "n_dyn"]
    assert [f[0] for f in _lib.PoolMaxDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.PoolMaxDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == 8 + 4 + 4 + 3 * 8 + 8 + 2 * 8 + 2 * 8 + 8 + 8 == 96
    assert ctypes.sizeof(_lib.PoolMaxDesc) == total


def _desc(N=8, G=2, D=4):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, 16-B aligned: never dereferenced
    d = _lib.PoolMaxDesc()
    d.N, d.G, d.D = N, G, D
    for f in ("graph_ptr", "batch", "x", "out", "arg", "gout", "gx"):
        setattr(d, f, a)
    d.x_stride = d.gx_stride = max(D, 1)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    for fn in (lib.kpgnn_segment_max_fwd, lib.kpgnn_segment_max_bwd):
        assert fn(None, None) == -1
        for bad in (dict(D=0), dict(G=-1), dict(N=-1), dict(D=1025)):
            assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
            assert b"segment_max" in lib.kpgnn_last_error(), bad
    assert lib.kpgnn_segment_max_fwd(ctypes.byref(_desc(G=0)), None) == 0
    assert lib.kpgnn_segment_max_bwd(ctypes.byref(_desc(N=0)), None) == 0
    # NULL required pointers and strides below D
    for fn, fields in ((lib.kpgnn_segment_max_fwd, ("graph_ptr", "x", "out")),
                       (lib.kpgnn_segment_max_bwd, ("batch", "arg", "gout", "gx"))):
        for f in fields:
            d = _desc()
            setattr(d, f, None)
            assert fn(ctypes.byref(d), None) == -1, f
            assert b"segment_max" in lib.kpgnn_last_error()
    d = _desc()
    d.x_stride = 3
    assert lib.kpgnn_segment_max_fwd(ctypes.byref(d), None) == -1
    d = _desc()
    d.gx_stride = 3
    assert lib.kpgnn_segment_max_bwd(ctypes.byref(d), None) == -1
    # D = 1023 is odd: vec = 1, 1023 lanes > 256
    for fn in (lib.kpgnn_segment_max_fwd, lib.kpgnn_segment_max_bwd):
        assert fn(ctypes.byref(_desc(D=1023)), None) == _lib.ELIMIT == -3
        assert b"segment_max: D=1023 too wide" in lib.kpgnn_last_error()


def test_cpu_route_is_the_framework_expression_bit_for_bit():
    from kp_gnn_amd import body
    g = torch.Generator().manual_seed(5)
    sizes = torch.tensor([1, 2, 3, 4, 5, 7, 8, 9, 37, 0, 6, 0])
    G, N, D = len(sizes), int(sizes.sum()), 13
    batch = torch.repeat_interleave(torch.arange(G), sizes)
    x = torch.randint(-3, 4, (N, D), generator=g).float()
    w = torch.randn(G, D, generator=g)

    def today(x):
        return x.new_full((G, D), float("-inf")).scatter_reduce(0, batch.view(-1, 1).expand_as(x), x, reduce="amax")

    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got, want = body.global_max_pool(a, batch, G), today(b)
    assert torch.equal(got, want) and bool(torch.isinf(got[9]).all())
    (got * w).sum().backward()
    (want * w).sum().backward()
    assert torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))
    # the even split is kept here: two tied rows of one graph get half the gradient each
    t = torch.tensor([[2.0], [2.0], [1.0]], requires_grad=True)
    body.global_max_pool(t, torch.zeros(3, dtype=torch.long), 1).sum().backward()
    assert t.grad.reshape(-1).tolist() == [0.5, 0.5, 0.0]
    assert body.make_pool("max", D) is body.global_max_pool
