"""CPU: the C ABI of the bodies' rd projection (include/kpgnn.h kpgnn_rd_proj_fwd / _bwd, csrc/rd_proj.hip) - declaration,
export, binding, descriptor layout and the argument checks that run before any device call - and the CPU route of the
bodies' _inputs, which stays the framework expression x + rd_projection(rd).squeeze() bit for bit."""
import argparse
import ctypes
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kpgnn_rd_proj_fwd", "kpgnn_rd_proj_bwd")
FIELDS = ["N", "H", "reserved", "x", "x_stride", "rd", "w", "b", "out", "out_stride", "dy", "dy_stride", "dw", "db",
          "workspace", "workspace_bytes", "n_dyn"]


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
        assert re.search(r"\bint\s+%s\s*\(\s*const\s+kpgnn_rd_proj_desc\s*\*" % n, txt), n
        assert hasattr(lib, n), n
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is ctypes.c_int and argtypes[0] is ctypes.POINTER(_lib.RdProjDesc) and len(argtypes) == 2
    assert re.search(r"\bsize_t\s+kpgnn_rd_proj_workspace_bytes\s*\(\s*int64_t\s+N\s*,\s*int32_t\s+H\s*\)", txt)
    assert _lib.SIGNATURES["kpgnn_rd_proj_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.RD_PROJ_MAX_H == 256


def test_descriptor_layout_matches_the_header():
    from kp_gnn_amd import _lib
    body = re.search(r"typedef struct kpgnn_rd_proj_desc \{(.*?)\} kpgnn_rd_proj_desc;", _header(), flags=re.S).group(1)
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
    assert [f[0] for f in _lib.RdProjDesc._fields_] == names
    for name in names:                                   # laid out by hand: no field needs padding in this order
        field = getattr(_lib.RdProjDesc, name)
        assert (field.offset, field.size) == (total, want[name]), name
        total += want[name]
    assert total == 8 + 4 + 4 + 14 * 8 == 128
    assert ctypes.sizeof(_lib.RdProjDesc) == total


def _desc(N=8, H=4, **kw):
    from kp_gnn_amd import _lib
    a = 0x10000                                          # dummy, non-NULL, 16-B aligned: never dereferenced
    d = _lib.RdProjDesc()
    d.N, d.H = N, H
    for f in ("x", "rd", "w", "b", "out", "dy", "dw", "db", "workspace"):
        setattr(d, f, a)
    d.x_stride = d.out_stride = d.dy_stride = max(H, 1)
    d.workspace_bytes = 1 << 22
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_argument_validation_without_gpu(built):
    from kp_gnn_amd import _lib
    lib = _lib.load()
    for fn in (lib.kpgnn_rd_proj_fwd, lib.kpgnn_rd_proj_bwd):
        assert fn(None, None) == -1
        for bad in (dict(H=0), dict(N=-1), dict(rd=None)):
            assert fn(ctypes.byref(_desc(**bad)), None) == -1, bad
            assert b"rd_proj" in lib.kpgnn_last_error(), bad
        assert fn(ctypes.byref(_desc(H=257)), None) == _lib.ELIMIT == -3
        assert b"H=257" in lib.kpgnn_last_error()
    assert lib.kpgnn_rd_proj_fwd(ctypes.byref(_desc(N=0)), None) == 0           # no rows: no launch
    for fn, fields in ((lib.kpgnn_rd_proj_fwd, ("x", "w", "b", "out")), (lib.kpgnn_rd_proj_bwd, ("dy", "dw", "db", "workspace"))):
        for f in fields:
            assert fn(ctypes.byref(_desc(**{f: None})), None) == -1, f
            assert b"rd_proj" in lib.kpgnn_last_error()
    for f in ("x_stride", "out_stride"):
        assert lib.kpgnn_rd_proj_fwd(ctypes.byref(_desc(**{f: 3})), None) == -1, f
    assert lib.kpgnn_rd_proj_bwd(ctypes.byref(_desc(dy_stride=3)), None) == -1
    assert lib.kpgnn_rd_proj_bwd(ctypes.byref(_desc(workspace=0x10004)), None) == -1        # 8-byte alignment
    # the workspace: at most 256 partials of 2 H doubles, fewer for fewer rows; 0 = the shape is not covered
    wb = lib.kpgnn_rd_proj_workspace_bytes
    assert wb(1000, 120) == 256 * 2 * 120 * 8 and wb(3, 120) == 3 * 2 * 120 * 8 and wb(0, 1) == 16
    assert wb(-1, 4) == 0 and wb(4, 0) == 0 and wb(4, 257) == 0
    assert lib.kpgnn_rd_proj_bwd(ctypes.byref(_desc(N=1000, H=120, workspace_bytes=wb(1000, 120) - 1)), None) == -1
    assert b"workspace" in lib.kpgnn_last_error()


def _body(H, use_rd=True):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name="KPGIN", hidden_size=H, K=3, num_layer=2, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    return B.make_GNN(ns)(num_layer=2, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                          init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=use_rd,
                          num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)


def test_cpu_route_of_inputs_is_the_framework_expression_bit_for_bit():
    from kp_gnn_amd import ops
    H, N = 18, 9            # (KP-GIN splits H over its K = 3 hops)
    gnn = _body(H)
    g = torch.Generator().manual_seed(1)
    data = types.SimpleNamespace(x=torch.randint(0, 21, (N, 1), generator=g), rd=torch.rand(N, 1, generator=g))
    lin = gnn.rd_projection
    assert not ops.rd_project_applies(gnn.init_proj(data).squeeze(), data.rd, lin.weight, lin.bias)
    got = gnn._inputs(data)
    want = gnn.init_proj(data).squeeze() + lin(data.rd).squeeze()
    assert torch.equal(got, want)
    got.sum().backward()
    gw, gb = lin.weight.grad.clone(), lin.bias.grad.clone()
    gnn.zero_grad()
    want.sum().backward()
    assert torch.equal(gw, lin.weight.grad) and torch.equal(gb, lin.bias.grad)
    assert torch.equal(ops.rd_project(want.detach(), data.rd, lin.weight, lin.bias), want.detach() + lin(data.rd).squeeze())
    # without the feature on the batch, or without use_rd, nothing is added
    assert torch.equal(gnn._inputs(types.SimpleNamespace(x=data.x)), gnn.init_proj(data).squeeze())
    plain = _body(H, use_rd=False)
    assert not hasattr(plain, "rd_projection") and torch.equal(plain._inputs(data), plain.init_proj(data).squeeze())


def test_reference_expression_is_float64_and_the_switch_returns_the_previous_setting():
    from kp_gnn_amd import ops
    g = torch.Generator().manual_seed(2)
    x, rd, w, b = torch.randn(5, 3, generator=g), torch.rand(5, 1, generator=g), torch.randn(3, 1, generator=g), torch.randn(3, generator=g)
    ref = ops.rd_project_reference(x, rd, w, b)
    assert ref.dtype == torch.float64
    assert torch.allclose(ref, x.double() + rd.double() * w.double().t() + b.double(), rtol=1e-14, atol=1e-14)
    prev = ops.set_native_rd_proj(False)
    try:
        assert ops.native_rd_proj() is False and ops.set_native_rd_proj(True) is False and ops.native_rd_proj() is True
    finally:
        ops.set_native_rd_proj(prev)
