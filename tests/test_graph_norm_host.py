"""The host side of the per-graph norms (no GPU): ops.body_norm_reference with a batch vector against tests/graph_norm_ref.py
in float64, the unchanged whole-batch expression, norm_scope validation, BatchNorm ignoring the keywords, and the binding
against the header (the descriptor checks, which need no device either, are in tests/test_graph_norm_cabi.py)."""
import argparse
import ctypes
import os
import re

import pytest
import torch

import graph_norm_cases as GC
import graph_norm_ref as GR
import norm_ref as NR

FWD, BWD = "kpgnn_graph_norm_fwd", "kpgnn_graph_norm_bwd"


def _T():
    from kp_gnn_amd import _lib
    return _lib.GRAPH_NORM_BLOCK_ROWS


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _close_every_graph(got, ref, ptr, name, rel=1e-12):
    """|got - ref| <= rel * max|ref|, graph by graph, the maximum taken over the tensor (Layer on a constant block included:
    torch.std's gradient at 0 is 0, and so is the expression's).  Not over the graph's own block: two float64 evaluation
    orders cannot agree to 1e-12 of a two-row graph's gradient, which is eps / var ~ 1e-5 of the terms it is the difference of
    (Instance: s e (1 - a^2)), so they differ by 1e-16 / 1e-5 = 1e-11 of it; test_graph_norm_cabi.py holds the kernels to
    the per-block bound at the tolerance fp32 allows."""
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(got).all()), name
    scale = float(ref.abs().max())
    for g, r0, r1 in GR.blocks(ptr):
        a, b = got[r0:r1], ref[r0:r1]
        assert float((a - b).abs().max()) <= rel * scale, (name, g, r1 - r0, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("kind", NR.KINDS)
@pytest.mark.parametrize("case", ["sizes", "shuffled", "empty-first-middle-last", "one-graph", "one-small-graph", "200-tiny"])
def test_the_framework_expression_with_batch_is_the_reference_per_block(kind, case):
    from kp_gnn_amd import ops
    sizes = GC.cases(_T())[case]
    ptr = GC.ptr_of(sizes)
    N, G = ptr[-1], len(sizes)
    batch = GR.batch_of(ptr)
    for C in GC.WIDTHS:
        x, gout, res, w, b = (t.double() for t in GC.inputs(N, C, seed=3))
        outs = []
        for f in (lambda x_, p_, r_: ops.body_norm_reference(x_, kind, *p_, residual=r_, batch=batch, num_graphs=G),
                  lambda x_, p_, r_: GR.norm(kind, x_, ptr, *p_, residual=r_)):
            x_ = x.clone().requires_grad_(True)
            p_ = [w.clone().requires_grad_(True), b.clone().requires_grad_(True)] if kind == "Layer" else []
            r_ = res.clone().requires_grad_(True)
            y = f(x_, p_, r_)
            outs.append([y.detach()] + list(torch.autograd.grad(y, [x_, r_] + p_, gout)))
        (y, dx, dr, *dp), (ry, rdx, rdr, *rdp) = outs
        tag = f"{kind} {case} C={C}"
        _close_every_graph(y, ry, ptr, tag + " y")
        _close_every_graph(dx, rdx, ptr, tag + " dx")
        assert torch.equal(dr, rdr), tag
        for a, r in zip(dp, rdp):
            assert float((a - r).abs().max()) <= 1e-12 * float(r.abs().max()), tag


@pytest.mark.parametrize("kind", NR.KINDS)
def test_without_batch_the_expression_is_the_old_one_bit_for_bit(kind):
    from kp_gnn_amd import ops
    g = torch.Generator().manual_seed(5)
    for dtype in (torch.float32, torch.float64):
        x = (0.5 + torch.randn(37, 12, generator=g)).to(dtype).requires_grad_(True)
        res = torch.randn(37, 12, generator=g).to(dtype)
        p = [(1 + torch.randn(12, generator=g)).to(dtype), torch.randn(12, generator=g).to(dtype)] if kind == "Layer" else []
        for fn in (ops.body_norm_reference, ops.body_norm):
            got = fn(x, kind, *p, residual=res)
            want = NR.norm(kind, x, *p, residual=res)
            assert torch.equal(got, want), (kind, dtype, fn.__name__)
            assert torch.equal(torch.autograd.grad(got, x, res)[0], torch.autograd.grad(want, x, res)[0])
    with pytest.raises(ValueError):
        ops.body_norm_reference(torch.zeros(3, 4), "Batch", batch=torch.zeros(3, dtype=torch.int64), num_graphs=1)
    with pytest.raises(ValueError):
        ops.body_norm(torch.zeros(3, 4), "Pair", batch=torch.zeros(3, dtype=torch.int64))      # a batch vector needs num_graphs


def test_cpu_tensors_through_the_modules_take_the_per_graph_expression():
    from kp_gnn_amd import body as B
    ptr = GC.ptr_of([3, 0, 5, 1])
    batch = GR.batch_of(ptr)
    x, _, res, w, b = GC.inputs(9, 6, seed=1)
    mods = {"Layer": B.LayerNorm(6), "Instance": B.InstanceNorm(6), "GraphSize": B.GraphSizeNorm(), "Pair": B.PairNorm()}
    with torch.no_grad():
        mods["Layer"].weight.copy_(w)
        mods["Layer"].bias.copy_(b)
    for kind, m in mods.items():
        got = m(x, residual=res, batch=batch, num_graphs=4).detach()
        want = GR.norm(kind, x, ptr, *m.parameters(), residual=res).detach()
        assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), kind
        assert not torch.allclose(got, m(x, residual=res)), kind            # (and it is not the whole-batch result)


def test_batchnorm_accepts_and_ignores_the_keywords():
    from kp_gnn_amd import body as B
    torch.manual_seed(0)
    bn = B.BatchNorm(6)
    x = torch.randn(9, 6)
    batch = GR.batch_of(GC.ptr_of([4, 5]))
    a = bn(x)
    bn.module.reset_running_stats()
    b = bn(x, batch=batch, num_graphs=2)
    assert torch.equal(a, b)


def _body(model_name, norm_type, **kw):
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=24, K=3, num_layer=3, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    return B.make_GNN(ns)(num_layer=3, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type=norm_type,
                          init_emb=B.EmbeddingEncoder(21, 24), residual=True, virtual_node=False, use_rd=False,
                          num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0, **kw)


@pytest.mark.parametrize("model_name", ["KPGIN", "KPGINPlus", "KPGINPrime"])
def test_norm_scope_is_validated_and_not_saved(model_name):
    assert _body(model_name, "Layer").norm_scope == "batch"
    g = _body(model_name, "Layer", norm_scope="graph")
    assert g.norm_scope == "graph"
    assert sorted(g.state_dict()) == sorted(_body(model_name, "Layer").state_dict())
    _body(model_name, "Layer").load_state_dict(g.state_dict())
    for bad in ("Graph", "node", None, 1):
        with pytest.raises(ValueError, match="norm_scope"):
            _body(model_name, "Layer", norm_scope=bad)


def test_the_binding_matches_the_header(lib):
    from kp_gnn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "kpgnn.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.search(r"(\w+)\s*$", part).group(1) for stmt in body.split(";") if stmt.strip() for part in stmt.split(",")]

    names = fields("kpgnn_graph_norm_desc")
    assert names == [f[0] for f in _lib.GraphNormDesc._fields_], names
    assert names == fields("kpgnn_norm_desc") + ["graph_ptr", "G"]
    f = dict(_lib.GraphNormDesc._fields_)
    assert f["eps"] is ctypes.c_float and f["N"] is ctypes.c_int64 and f["G"] is ctypes.c_int32
    for name in (FWD, BWD):
        assert getattr(lib, name).argtypes[0] == ctypes.POINTER(_lib.GraphNormDesc)
    assert lib.kpgnn_graph_norm_workspace_bytes.restype is ctypes.c_size_t
    assert lib.kpgnn_graph_norm_saved_floats.restype is ctypes.c_size_t
    assert len(lib.kpgnn_graph_norm_workspace_bytes.argtypes) == 4 and len(lib.kpgnn_graph_norm_saved_floats.argtypes) == 3
    assert int(re.search(r"#define KPGNN_GRAPH_NORM_BLOCK_ROWS (\d+)", text).group(1)) == _lib.GRAPH_NORM_BLOCK_ROWS
