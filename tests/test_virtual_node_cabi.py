"""CPU: kpgnn_vn_add_pool (csrc/virtual_node.hip) is exported and bound, and rejects malformed descriptors before any device
call (every pointer is a dummy that is never dereferenced, the stream is NULL; no case here reaches a launch).  The virtual-node
helpers of kp_gnn_amd.body take the graph count from the batch when it carries one and keep the framework expression on CPU
tensors, which equals a float64 restatement to the golden tolerances.

The bodies themselves have no CPU path (their layers refuse CPU tensors: "there is no CPU fallback"), so the comparison of a
whole virtual-node body with and without `num_graphs` against the float64 oracle lives in tests/test_virtual_node.py
(test_bodies_with_and_without_num_graphs_vs_float64), on the device."""
import ctypes
import types

import pytest
import torch

import parity_f64 as PF

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
OK, EINVAL, ELIMIT = 0, -1, -3
WHO = b"kpgnn_vn_add_pool"


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _desc(N=100, G=4, D=32, **kw):
    from kp_gnn_amd import _lib
    d = _lib.VnDesc()
    d.N, d.G, d.D = N, G, D
    d.graph_ptr, d.x, d.x_stride, d.v, d.v_stride, d.out, d.out_stride, d.pooled = A, A, D, A, D, A, D, A
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_the_entry_is_exported_and_bound(lib):
    from kp_gnn_amd import _lib
    assert hasattr(lib, "kpgnn_vn_add_pool")
    fn = lib.kpgnn_vn_add_pool
    assert fn.restype is ctypes.c_int and fn.argtypes[0] == ctypes.POINTER(_lib.VnDesc)
    names = [f[0] for f in _lib.VnDesc._fields_]
    assert names == ["N", "G", "D", "graph_ptr", "x", "x_stride", "v", "v_stride", "out", "out_stride", "pooled", "n_dyn"]


def test_null_descriptor_is_rejected(lib):
    assert lib.kpgnn_vn_add_pool(None, None) == EINVAL
    assert WHO + b": NULL descriptor" in lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", [dict(D=0), dict(D=-3), dict(N=-1), dict(G=-2)])
def test_bad_sizes_are_rejected(lib, kw):
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(**kw)), None) == EINVAL, kw
    assert WHO + b": bad " in lib.kpgnn_last_error(), lib.kpgnn_last_error()


@pytest.mark.parametrize("field", ["graph_ptr", "x", "v", "out"])
def test_null_pointers_are_rejected(lib, field):
    d = _desc()
    setattr(d, field, None)
    assert lib.kpgnn_vn_add_pool(ctypes.byref(d), None) == EINVAL, field
    assert WHO in lib.kpgnn_last_error() and b"NULL" in lib.kpgnn_last_error(), (field, lib.kpgnn_last_error())


@pytest.mark.parametrize("field", ["x_stride", "out_stride"])
def test_short_row_strides_are_rejected(lib, field):
    d = _desc()
    setattr(d, field, 31)
    assert lib.kpgnn_vn_add_pool(ctypes.byref(d), None) == EINVAL, field
    assert WHO in lib.kpgnn_last_error() and b"stride" in lib.kpgnn_last_error()


def test_a_zero_v_stride_is_accepted_and_a_short_one_is_not(lib):
    """G = 0: every check runs, nothing is launched.  Stride 0 is layer 0's virtual node, one embedding row for all graphs."""
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(G=0, v_stride=0)), None) == OK
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(G=0, v_stride=32)), None) == OK
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(G=0, v_stride=31)), None) == EINVAL
    assert WHO in lib.kpgnn_last_error() and b"v row stride" in lib.kpgnn_last_error()
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(G=0, v_stride=-32)), None) == EINVAL


def test_rows_wider_than_the_kernel_answer_elimit(lib):
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(D=1028, x_stride=1028, v_stride=1028, out_stride=1028)), None) == ELIMIT
    assert WHO + b": D=1028" in lib.kpgnn_last_error()
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(D=260, x_stride=260, v_stride=0, out_stride=260)), None) == ELIMIT


def test_no_graphs_is_ok_without_a_launch(lib):
    """(a launch with these dummy pointers and a NULL stream could not succeed)"""
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(G=0, graph_ptr=None, v=None)), None) == OK
    assert lib.kpgnn_vn_add_pool(ctypes.byref(_desc(N=0, G=0, graph_ptr=None, x=None, v=None, out=None, pooled=None)), None) == OK


# ------------------------------------------------------------------------------------------------ the Python side on the CPU
def _close(got, ref, name):
    got, ref = got.detach().double(), ref.detach()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    bound = PF.ATOL * float(ref.abs().max()) + PF.RTOL * ref.abs()
    assert bool((err <= bound).all()), (name, float(err.max()))


@pytest.mark.parametrize("expanded", [False, True])
@pytest.mark.parametrize("want_pool", [False, True])
def test_cpu_tensors_keep_the_framework_expression(expanded, want_pool):
    from kp_gnn_amd import ops
    torch.manual_seed(5)
    sizes = [0, 1, 3, 4, 5, 9, 67, 0, 2]
    G, D = len(sizes), 24
    batch = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))
    x = torch.randn(int(batch.numel()), D, requires_grad=True)
    row = torch.randn(1 if expanded else G, D, requires_grad=True)
    vn = row.expand(G, -1) if expanded else row
    out, pooled = ops.virtual_node_add(x, vn, batch, G, want_pool)
    x64, r64 = x.detach().double().requires_grad_(True), row.detach().double().requires_grad_(True)
    v64 = r64.expand(G, -1)
    o64 = x64 + v64[batch]
    p64 = torch.zeros(G, D, dtype=torch.float64).index_add_(0, batch, o64) + v64
    _close(out, o64, "out")
    go, gp = torch.randn(out.shape), torch.randn(G, D)
    if want_pool:
        _close(pooled, p64, "pooled")
        ((out * go).sum() + (pooled * gp).sum()).backward()
        ((o64 * go.double()).sum() + (p64 * gp.double()).sum()).backward()
    else:
        assert pooled is None
        (out * go).sum().backward()
        (o64 * go.double()).sum().backward()
    _close(x.grad, x64.grad, "gx")
    _close(row.grad, r64.grad, "gv")


def _vn_body(L=3, H=16):
    import argparse
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name="KPGINPlus", hidden_size=H, K=3, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine="geometric", eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    return B.GNNPlus(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch", init_emb=B.EmbeddingEncoder(21, H),
                     residual=True, virtual_node=True, use_rd=False, num_hop1_edge=3, max_edge_count=50, max_hop_num=6,
                     max_distance_count=50, drop_prob=0.0)


def test_vn_init_takes_the_graph_count_from_the_batch_and_expands_one_row():
    gnn = _vn_body()
    with torch.no_grad():
        gnn.virtualnode_embedding.weight.normal_()

    class NoItem(torch.Tensor):
        """A batch vector whose read-back raises: what a stream capture does to .item()."""
        @staticmethod
        def __new__(cls, t):
            return torch.Tensor._make_subclass(cls, t)

        def item(self):
            raise AssertionError("host read-back of the batch vector")

    batch = torch.tensor([0, 0, 1, 3, 3, 3])
    vn = gnn._vn_init(types.SimpleNamespace(num_graphs=4), NoItem(batch))
    assert tuple(vn.shape) == (4, 16) and vn.stride(0) == 0
    assert vn.data_ptr() == gnn.virtualnode_embedding.weight.data_ptr()
    vn2 = gnn._vn_init(types.SimpleNamespace(), batch)          # no num_graphs: the one read-back, as the readouts do
    assert torch.equal(vn, vn2) and vn2.stride(0) == 0
    vn2.sum().backward()
    assert torch.equal(gnn.virtualnode_embedding.weight.grad, torch.full((1, 16), 4.0))


def test_vn_update_on_cpu_equals_the_float64_restatement_and_keeps_the_batchnorm_error():
    """The pooled sum + vn through the virtual-node MLP (+ residual) on CPU tensors: the framework modules, one by one."""
    import torch.nn.functional as F
    gnn = _vn_body().train()
    torch.manual_seed(9)
    G, H = 7, 16
    tmp, vn = torch.randn(G, H), torch.randn(G, H)
    got = gnn._vn_update(1, vn, tmp)
    m = gnn.mlp_virtualnode_list[1]
    z = tmp.double()
    for lin, bn in ((m[0], m[1]), (m[3], m[4])):
        z = F.linear(z, lin.weight.double(), lin.bias.double())
        z = F.relu(F.batch_norm(z, None, None, bn.weight.double(), bn.bias.double(), True, 0.1, bn.eps))
    _close(got, vn.double() + z, "vn update")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        gnn._vn_update(0, vn[:1], tmp[:1])
    gnn.eval()
    assert tuple(gnn._vn_update(0, vn[:1], tmp[:1]).shape) == (1, H)      # G == 1 is fine on running statistics
