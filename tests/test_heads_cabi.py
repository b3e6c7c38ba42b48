"""CPU: the task-head entries kpgnn_attn_pool_* / kpgnn_head_linear_* / kpgnn_nll_loss reject malformed descriptors before any
device call (every pointer is a dummy that is never dereferenced, the stream is NULL), the head modules of kp_gnn_amd.body
have the reference's constructors and state_dict keys, and on CPU tensors (the framework formulation) they equal a float64
restatement of the formulas to fp32 rounding: |got - ref| <= ATOL * max|ref| + RTOL * |ref| (tests/parity_f64.py)."""
import ctypes
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import parity_f64 as PF

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
EINVAL, ELIMIT = -1, -3


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _attn_desc(N=100, G=4, D=32):
    from kp_gnn_amd import _lib
    d = _lib.AttnPoolDesc()
    d.N, d.G, d.D = N, G, D
    d.graph_ptr, d.x, d.x_stride, d.w, d.bias, d.alpha, d.out = A, A, D, A, A, A, A
    d.gout, d.gx, d.gx_stride, d.dw, d.db, d.workspace, d.workspace_bytes = A, A, D, A, A, A, 1 << 20
    return d


def _lin_desc(M=100, O=4, I=32):
    from kp_gnn_amd import _lib
    d = _lib.HeadLinearDesc()
    d.M, d.O, d.I = M, O, I
    d.x, d.x_stride, d.w, d.bias, d.y, d.y_stride = A, I, A, A, A, O
    d.dy, d.dy_stride, d.dx, d.dx_stride, d.dw, d.db, d.workspace, d.workspace_bytes = A, O, A, I, A, A, A, 1 << 20
    return d


def _loss_desc(M=100, C=10):
    from kp_gnn_amd import _lib
    d = _lib.NllLossDesc()
    d.M, d.C, d.reduction = M, C, 0
    d.logits, d.logits_stride, d.y, d.loss, d.dlogits, d.dlogits_stride, d.correct = A, C, A, A, A, C, A
    return d


ENTRIES = [("kpgnn_attn_pool_fwd", "attn_pool_fwd", _attn_desc), ("kpgnn_attn_pool_bwd", "attn_pool_bwd", _attn_desc),
           ("kpgnn_head_linear_fwd", "head_linear_fwd", _lin_desc), ("kpgnn_head_linear_bwd", "head_linear_bwd", _lin_desc),
           ("kpgnn_nll_loss", "nll_loss", _loss_desc)]


@pytest.mark.parametrize("entry,who,make", ENTRIES)
def test_null_descriptors_are_rejected(lib, entry, who, make):
    assert getattr(lib, entry)(None, None) == EINVAL
    assert (who + ": NULL descriptor").encode() in lib.kpgnn_last_error()


@pytest.mark.parametrize("entry,who,make", ENTRIES)
def test_bad_sizes_are_rejected(lib, entry, who, make):
    fn = getattr(lib, entry)
    if make is _attn_desc:
        bad = [dict(N=-1), dict(D=0), dict(G=-2)]
    elif make is _lin_desc:
        bad = [dict(M=-1), dict(O=0), dict(O=-4), dict(I=0)]
    else:
        bad = [dict(M=-5), dict(C=0)]                # (M = 0 is an empty batch, accepted like the other entries' zero rows)
    for kw in bad:
        assert fn(ctypes.byref(make(**kw)), None) == EINVAL, kw
        assert (who + ": bad ").encode() in lib.kpgnn_last_error(), (kw, lib.kpgnn_last_error())


@pytest.mark.parametrize("entry,who,make,fields", [
    ("kpgnn_attn_pool_fwd", "attn_pool_fwd", _attn_desc, ["graph_ptr", "x", "w", "alpha", "out"]),
    ("kpgnn_attn_pool_bwd", "attn_pool_bwd", _attn_desc, ["graph_ptr", "x", "w", "alpha", "out", "gout", "dw"]),
    ("kpgnn_head_linear_fwd", "head_linear_fwd", _lin_desc, ["x", "w", "y"]),
    ("kpgnn_head_linear_bwd", "head_linear_bwd", _lin_desc, ["x", "w", "dy", "dw"]),
    ("kpgnn_nll_loss", "nll_loss", _loss_desc, ["logits", "y", "loss"]),
])
def test_null_pointers_are_rejected(lib, entry, who, make, fields):
    fn = getattr(lib, entry)
    for f in fields:
        d = make()
        setattr(d, f, None)
        assert fn(ctypes.byref(d), None) == EINVAL, f
        assert who.encode() in lib.kpgnn_last_error() and b"NULL" in lib.kpgnn_last_error(), (f, lib.kpgnn_last_error())


def test_short_strides_and_bad_reduction_are_rejected(lib):
    d = _attn_desc()
    d.x_stride = 31
    assert lib.kpgnn_attn_pool_fwd(ctypes.byref(d), None) == EINVAL
    d = _lin_desc()
    d.y_stride = 3
    assert lib.kpgnn_head_linear_fwd(ctypes.byref(d), None) == EINVAL
    d = _lin_desc()
    d.dy_stride = 3
    assert lib.kpgnn_head_linear_bwd(ctypes.byref(d), None) == EINVAL
    d = _loss_desc()
    d.reduction = 2
    assert lib.kpgnn_nll_loss(ctypes.byref(d), None) == EINVAL
    assert b"nll_loss: reduction" in lib.kpgnn_last_error()
    d = _loss_desc()
    d.logits_stride = 9
    assert lib.kpgnn_nll_loss(ctypes.byref(d), None) == EINVAL


def test_shapes_the_kernels_do_not_instantiate_answer_elimit(lib):
    """Python keeps the framework formulation for these (ops.attention_pool, ops_dense.head_linear)."""
    for fn in (lib.kpgnn_head_linear_fwd, lib.kpgnn_head_linear_bwd):
        assert fn(ctypes.byref(_lin_desc(O=33)), None) == ELIMIT
        assert b"O=33" in lib.kpgnn_last_error()
        assert fn(ctypes.byref(_lin_desc(I=1025)), None) == ELIMIT
        assert b"I=1025" in lib.kpgnn_last_error()
    for fn in (lib.kpgnn_attn_pool_fwd, lib.kpgnn_attn_pool_bwd):
        assert fn(ctypes.byref(_attn_desc(D=260)), None) == ELIMIT
        assert b"attn_pool: D=260" in lib.kpgnn_last_error()
    assert lib.kpgnn_nll_loss(ctypes.byref(_loss_desc(C=1025)), None) == ELIMIT
    assert b"nll_loss: C=1025" in lib.kpgnn_last_error()


def test_workspace_queries(lib):
    assert lib.kpgnn_attn_pool_workspace_bytes(0, 32) == 0 and lib.kpgnn_attn_pool_workspace_bytes(8, 260) == 0
    # D = 33: one column per lane, 64 lanes per graph, 4 graphs per block -> 75 blocks of D + 1 floats for 300 graphs
    assert lib.kpgnn_attn_pool_workspace_bytes(300, 33) == 75 * 34 * 4
    assert lib.kpgnn_head_linear_workspace_bytes(128, 4, 32) == 0          # one block covers 128 rows: no slabs
    assert lib.kpgnn_head_linear_workspace_bytes(5000, 10, 48) == 40 * (10 * 48 + 10) * 4      # 128-row tiles
    assert lib.kpgnn_head_linear_workspace_bytes(5000, 33, 48) == 0


# ------------------------------------------------------------------------------------------------ modules
class StubBody(nn.Module):
    """An embedding model that returns a fixed leaf tensor: hidden_size, JK and num_layer are all the heads read."""

    def __init__(self, x, JK="last", num_layer=3):
        super().__init__()
        self.hidden_size, self.JK, self.num_layer = x.shape[1], JK, num_layer
        self.x = x
        self.resets = 0

    def reset_parameters(self):
        self.resets += 1

    def forward(self, data):
        return self.x


def _graphs(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _data(batch, G):
    return types.SimpleNamespace(batch=batch, num_graphs=G)


def test_constructors_and_state_dict_keys():
    from kp_gnn_amd import body as B
    x = torch.zeros(5, 16)
    for pooling in ("sum", "mean", "max"):
        m = B.GraphClassification(StubBody(x), pooling, 7)
        assert sorted(m.state_dict()) == ["classifier.bias", "classifier.weight"]
        assert m.classifier.weight.shape == (7, 16) and m.pooling_method == pooling and (m.JK, m.num_layer) == ("last", 3)
        assert sorted(B.GraphRegression(StubBody(x), pooling).state_dict()) == ["regressor.bias", "regressor.weight"]
    m = B.GraphClassification(StubBody(x), "attention", 7)
    assert sorted(m.state_dict()) == ["classifier.bias", "classifier.weight", "pool.gate_nn.bias", "pool.gate_nn.weight"]
    assert m.pool.gate_nn.weight.shape == (1, 16) and m.embedding_model.resets == 1
    before = m.pool.gate_nn.weight.detach().clone()
    m.reset_parameters()
    assert not torch.equal(before, m.pool.gate_nn.weight) and m.embedding_model.resets == 2
    with pytest.raises(ValueError, match="pooling method not implemented"):
        B.GraphClassification(StubBody(x), "median", 7)
    m = B.NodeClassification(StubBody(x), 4)
    assert sorted(m.state_dict()) == ["classifier.bias", "classifier.weight"] and m.classifier.weight.shape == (4, 16)
    m = B.NodeClassification(StubBody(x, JK="concat", num_layer=3), 4)
    assert m.classifier.weight.shape == (4, 16 * 4)                # the reference's width under JK == "concat"
    m = B.NodeRegression(StubBody(x))
    assert sorted(m.state_dict()) == ["regressor.bias", "regressor.weight"] and m.regressor.weight.shape == (1, 16)
    assert (m.JK, m.num_layer) == ("last", 3)


def test_graph_regression_takes_attention_pooling():
    from kp_gnn_amd import body as B
    m = B.GraphRegression(StubBody(torch.zeros(5, 16)), "attention")
    assert sorted(m.state_dict()) == ["pool.gate_nn.bias", "pool.gate_nn.weight", "regressor.bias", "regressor.weight"]
    assert isinstance(m.pool, B.AttentionalAggregation) and isinstance(m.pool.gate_nn, nn.Linear)


def _close(got, ref, name):
    got, ref = got.detach().double(), ref.detach()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = PF.ATOL * float(ref.abs().max()) + PF.RTOL * ref.abs()
    assert bool((err <= bound).all()), (name, float(err.max()))


def _pool64(x, batch, G, method, gate=None):
    x = x.double()
    if method == "attention":
        g = F.linear(x, gate.weight.double(), gate.bias.double()).reshape(-1)
        alpha = torch.zeros_like(g)
        for k in range(G):
            sel = batch == k
            if bool(sel.any()):
                e = (g[sel] - g[sel].max()).exp()
                alpha[sel] = e / (e.sum() + 1e-16)
        return torch.zeros(G, x.shape[1], dtype=torch.float64).index_add_(0, batch, alpha.unsqueeze(-1) * x)
    out = torch.zeros(G, x.shape[1], dtype=torch.float64).index_add_(0, batch, x)
    if method == "mean":
        out = out / torch.bincount(batch, minlength=G).clamp(min=1).unsqueeze(-1)
    return out


def _lin64(lin, v):
    return F.linear(v, lin.weight.double(), lin.bias.double())


@pytest.mark.parametrize("pooling", ["sum", "mean", "attention"])
def test_cpu_graph_heads_equal_the_float64_restatement(pooling):
    from kp_gnn_amd import body as B
    torch.manual_seed(11)
    sizes = [1, 0, 7, 64, 65, 3, 0]
    batch, G = _graphs(sizes), len(sizes)
    x = torch.relu(torch.randn(int(batch.numel()), 48)).requires_grad_(True)
    clf = B.GraphClassification(StubBody(x), pooling, 10)
    logits = clf(_data(batch, G))
    ref = _lin64(clf.classifier, _pool64(x.detach(), batch, G, pooling, getattr(clf.pool, "gate_nn", None)))
    assert logits.shape == (G, 10)
    _close(logits, ref, f"GraphClassification {pooling}")
    reg = B.GraphRegression(StubBody(x), pooling)
    score = reg(_data(batch, G))
    ref = _lin64(reg.regressor, _pool64(x.detach(), batch, G, pooling, getattr(reg.pool, "gate_nn", None))).squeeze()
    assert score.shape == (G,)
    _close(score, ref, f"GraphRegression {pooling}")
    logits.sum().backward()                      # the framework formulation differentiates on the CPU
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def test_cpu_node_heads_equal_the_float64_restatement():
    from kp_gnn_amd import body as B
    torch.manual_seed(12)
    x = torch.relu(torch.randn(77, 33))
    data = _data(torch.zeros(77, dtype=torch.long), 1)
    nc = B.NodeClassification(StubBody(x), 4)
    _close(nc(data), _lin64(nc.classifier, x.double()), "NodeClassification")
    nr = B.NodeRegression(StubBody(x))
    out = nr(data)
    assert out.shape == (77,)
    _close(out, _lin64(nr.regressor, x.double()).squeeze(), "NodeRegression")


def test_a_width_mismatch_raises_the_framework_shape_error():
    """The reference sizes NodeClassification's classifier for hidden_size * (num_layer + 1) inputs under JK == "concat" while its
    bodies return hidden_size columns: the forward raises there, and here (tests/test_heads.py: on the device too)."""
    from kp_gnn_amd import body as B, ops, ops_dense
    x = torch.randn(9, 16)
    data = _data(torch.zeros(9, dtype=torch.long), 1)
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        B.NodeClassification(StubBody(x, JK="concat", num_layer=3), 4)(data)
    for width in (8, 24):
        with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
            ops_dense.head_linear(x, nn.Linear(width, 4))
        with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
            ops.attention_pool(x, data.batch, 1, nn.Linear(width, 1))


@pytest.mark.parametrize("reduction", ["mean", "sum"])
def test_cpu_classification_loss_equals_the_float64_restatement(reduction):
    from kp_gnn_amd import ops_dense
    torch.manual_seed(13)
    logits = (3.0 * torch.randn(128, 15)).requires_grad_(True)
    y = torch.randint(0, 15, (128,))
    y[5] = -100
    l64 = logits.detach().double().requires_grad_(True)
    ref = F.nll_loss(F.log_softmax(l64, -1), y, reduction=reduction)
    ref.backward()
    loss = ops_dense.classification_loss(logits, y, reduction)
    loss.backward()
    _close(loss, ref.detach(), "loss")
    _close(logits.grad, l64.grad, "dlogits")
    lsum, correct = ops_dense.classification_eval(logits.detach(), y)
    _close(lsum, F.nll_loss(F.log_softmax(l64.detach(), -1), y, reduction="sum"), "loss sum")
    assert int(correct) == int((logits.argmax(1) == y).sum()) and correct.dtype == torch.int32
