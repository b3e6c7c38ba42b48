"""kpgnn_dropout_fwd / _bwd / _mask (csrc/dropout.hip) through the C ABI.

CPU: the numpy restatement of the mask definition (tests/dropout_ref.py) reproduces the Philox4x32-10 known-answer vectors, and
the three entries reject malformed descriptors before any device call.  GPU: the exported mask equals the restatement bit for
bit, the forward and the backward are held to that mask, call ids advance on the device, and rows beyond *n_dyn are left alone
while the live rows do not depend on the capacity."""
import ctypes

import numpy as np
import pytest
import torch

import dropout_ref as DR

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
OK, EINVAL = 0, -1
ENTRIES = ("kpgnn_dropout_fwd", "kpgnn_dropout_bwd")
SHAPES = [(1, 104), (257, 6), (257, 33), (5000, 104), (300, 256)]   # one row; rows that straddle the groups of four; > 1 block
PS = (0.1, 0.5)
CALLS = (0, 1, 2 ** 32 + 5)
SEEDS = (0, 0x1234567890ABCDEF)


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _desc(N=100, C=32, **kw):
    from kp_gnn_amd import _lib
    d = _lib.DropoutDesc()
    d.N, d.C = N, C
    d.x, d.x_stride, d.out, d.out_stride, d.residual, d.r_stride = A, C, A, C, A, C
    d.thr, d.scale = DR.threshold(0.5), 2.0
    d.state, d.call_io, d.ticket = A, A, A
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _mask_desc(N=100, C=32, **kw):
    from kp_gnn_amd import _lib
    d = _lib.DropoutMaskDesc()
    d.seed, d.call, d.N, d.C, d.thr, d.mask = 1, 2, N, C, DR.threshold(0.5), A
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------ CPU
def test_numpy_philox_reproduces_the_known_answer_vectors():
    f = 0xFFFFFFFF
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for counter, key, want in kat:
        got = tuple(int(w) for w in DR.philox4x32_10(counter, key))
        assert got == want, (counter, key, [hex(g) for g in got])
    assert DR.threshold(0.5) == 2 ** 31 and DR.threshold(0.1) == 429496729 and DR.threshold(1.0) == 4294967295


def test_null_descriptors_and_empty_widths_are_rejected(lib):
    """-1 with a message, before any device call (the stream is NULL and every pointer a dummy)."""
    for name in ENTRIES + ("kpgnn_dropout_mask",):
        fn = getattr(lib, name)
        assert fn(None, None) == EINVAL, name
        assert name.encode() + b": NULL descriptor" in lib.kpgnn_last_error()
        d = _mask_desc(C=0) if name.endswith("mask") else _desc(C=0)
        assert fn(ctypes.byref(d), None) == EINVAL, name
        assert name.encode() + b": bad N=" in lib.kpgnn_last_error(), lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", [dict(N=-1), dict(C=-4), dict(x=None), dict(out=None), dict(state=None), dict(call_io=None),
                                dict(x_stride=-32), dict(out_stride=-32), dict(x_stride=31)])
def test_malformed_descriptors_are_rejected(lib, kw):
    for name in ENTRIES:
        assert getattr(lib, name)(ctypes.byref(_desc(**kw)), None) == EINVAL, (name, kw)
        assert name.encode() in lib.kpgnn_last_error()
    assert lib.kpgnn_dropout_fwd(ctypes.byref(_desc(r_stride=-32)), None) == EINVAL
    assert lib.kpgnn_dropout_fwd(ctypes.byref(_desc(ticket=None)), None) == EINVAL
    assert lib.kpgnn_dropout_mask(ctypes.byref(_mask_desc(mask=None)), None) == EINVAL
    assert lib.kpgnn_dropout_mask(ctypes.byref(_mask_desc(N=-2)), None) == EINVAL


def test_empty_row_counts_launch_nothing(lib):
    for name in ENTRIES:
        assert getattr(lib, name)(ctypes.byref(_desc(N=0)), None) == OK, name
    assert lib.kpgnn_dropout_mask(ctypes.byref(_mask_desc(N=0)), None) == OK


def test_the_entries_are_bound(lib):
    from kp_gnn_amd import _lib
    names = [f[0] for f in _lib.DropoutDesc._fields_]
    assert names == ["N", "C", "x", "x_stride", "out", "out_stride", "residual", "r_stride", "thr", "scale", "state", "call_io",
                     "ticket", "n_dyn"]
    for name in ENTRIES:
        assert getattr(lib, name).argtypes[0] == ctypes.POINTER(_lib.DropoutDesc)
    assert lib.kpgnn_dropout_mask.argtypes[0] == ctypes.POINTER(_lib.DropoutMaskDesc)


def test_the_switch_is_off_by_default_and_cpu_tensors_keep_the_framework_expression():
    from kp_gnn_amd import ops
    assert ops.native_dropout() is False
    prev = ops.set_native_dropout(True)
    try:
        assert prev is False and ops.native_dropout() is True
        x, r = torch.randn(5, 8), torch.randn(5, 8)
        assert not ops.native_dropout_applies(x, 0.5, True)
        assert torch.equal(ops.dropout_add(x, 0.5, False, r), x + r) and torch.equal(ops.dropout_add(x, 0.0, True), x)
        torch.manual_seed(1)
        got = ops.dropout_add(x, 0.5, True, r)
        torch.manual_seed(1)
        assert torch.equal(got, torch.nn.functional.dropout(x, 0.5, True) + r)
    finally:
        ops.set_native_dropout(prev)
    assert ops.native_dropout() is False


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda:0")


def _state(seed, calls=0):
    """(int64[2] {seed, calls}, int64[1] ticket) of the test's own: the ABI, not the package's state tensor."""
    from kp_gnn_amd import ops
    dev = _dev()
    return torch.tensor([ops._signed64(seed), calls], dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)


def _launch(name, x, out, p, state, ticket, cell, residual=None, N=None, n_dyn=None):
    from kp_gnn_amd import _lib
    C = x.shape[1]
    assert x.stride(1) == 1 and out.stride(1) == 1
    d = _lib.DropoutDesc()
    d.N, d.C = x.shape[0] if N is None else N, C
    d.x, d.x_stride, d.out, d.out_stride = x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0)
    if residual is not None:
        d.residual, d.r_stride = residual.data_ptr(), residual.stride(0)
    d.thr, d.scale = DR.threshold(p), DR.scale64(p)
    d.state, d.call_io, d.ticket = state.data_ptr(), cell.data_ptr(), ticket.data_ptr()
    d.n_dyn = None if n_dyn is None else n_dyn.data_ptr()
    _lib.launch(name, x.device, ctypes.byref(d))


def _exported_mask(N, C, p, seed, call):
    from kp_gnn_amd import ops
    return ops.dropout_mask((N, C), p, seed, call, _dev())


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_mask_equals_the_numpy_restatement(N, C):
    for p in PS:
        for call in CALLS:
            for seed in SEEDS:
                got = _exported_mask(N, C, p, seed, call)
                assert got.dtype == torch.bool and tuple(got.shape) == (N, C)
                ref = DR.keep_mask(N, C, p, seed, call)
                assert np.array_equal(got.cpu().numpy(), ref), (N, C, p, call, hex(seed))


@pytest.mark.gpu
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("with_residual", [True, False])
@pytest.mark.parametrize("N,C", SHAPES)
def test_forward_given_the_exported_mask(N, C, with_residual, strided):
    """Dropped elements are the residual's bits (0.0 without one); kept ones are within 2^-22 (|x| scale + |residual|) of the
    float64 expression: the rounding of scale to fp32 (2^-24 relative) and one fused rounding (2^-24 of the result).  strided:
    x and the residual are column views of wider tensors (row stride C + 8) and are read in place."""
    dev = _dev()
    p, seed, call = (0.1, SEEDS[1], CALLS[2]) if C in (33, 256) else (0.5, SEEDS[1], 7)
    g = torch.Generator().manual_seed(N * 1000 + C)
    wide = torch.randn(N, C + 8, generator=g).to(dev)
    rwide = torch.randn(N, C + 8, generator=g).to(dev)
    x = wide[:, 4:4 + C] if strided else wide[:, :C].contiguous()
    res = (rwide[:, 4:4 + C] if strided else rwide[:, :C].contiguous()) if with_residual else None
    if strided:
        assert x.stride(0) == C + 8 and x.data_ptr() == wide.data_ptr() + 16      # a view: nothing was copied
    state, ticket = _state(seed, call)
    cell = torch.full((1,), -1, dtype=torch.int64, device=dev)
    out = torch.full((N, C), float("nan"), device=dev)
    _launch("kpgnn_dropout_fwd", x, out, p, state, ticket, cell, residual=res)
    torch.cuda.synchronize()
    assert int(cell) == call and state.tolist() == [seed, call + 1] and int(ticket) == 0
    keep = _exported_mask(N, C, p, seed, call)
    r = res if with_residual else torch.zeros_like(x)
    assert torch.equal(out[~keep].view(torch.int32), r[~keep].contiguous().view(torch.int32)), "a dropped element is not the residual"
    scale = DR.scale64(p)
    ref64 = x.double() * scale + r.double()
    bound = 2.0 ** -22 * (x.double().abs() * scale + r.double().abs())
    err = (out.double() - ref64).abs()
    print(f"N{N} C{C} residual{with_residual} strided{strided}: max err / bound = {float((err[keep] / bound[keep]).max()):.3f}")
    assert bool((err[keep] <= bound[keep]).all())
    frac = 1.0 - float(keep.float().mean())
    assert N * C < 1000 or abs(frac - p) < 5 * (p * (1 - p) / (N * C)) ** 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_backward_recomputes_the_mask(N, C):
    """dx = dout * scale (the fp32 product, bitwise) where kept and 0.0 where dropped, from the seed and the call cell alone;
    `calls` is not touched."""
    dev = _dev()
    p, seed, call = 0.5, SEEDS[1], CALLS[2]
    dout = torch.randn(N, C, generator=torch.Generator().manual_seed(C)).to(dev)
    state, ticket = _state(seed, 11)
    cell = torch.tensor([call], dtype=torch.int64, device=dev)
    dx = torch.full((N, C), float("nan"), device=dev)
    _launch("kpgnn_dropout_bwd", dout, dx, p, state, ticket, cell)
    torch.cuda.synchronize()
    assert state.tolist()[1] == 11 and int(cell) == call and int(ticket) == 0
    keep = _exported_mask(N, C, p, seed, call)
    want = torch.where(keep, dout * torch.tensor(DR.scale64(p), dtype=torch.float32, device=dev), torch.zeros_like(dout))
    assert torch.equal(dx.view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
def test_call_ids_advance_on_the_device():
    """After dropout_seed(s): three forward launches on (5000, 104) leave 0, 1 and 2 in their call cells and calls == 3, with
    three different masks; a backward launch leaves calls alone."""
    from kp_gnn_amd import ops
    dev = _dev()
    N, C, p, s = 5000, 104, 0.5, 1234
    ops.dropout_seed(s, dev)
    st = ops.dropout_state(dev)
    assert st.tolist() == [s, 0, 0]
    x = torch.ones(N, C, device=dev)
    cells = [torch.full((1,), -1, dtype=torch.int64, device=dev) for _ in range(3)]
    outs = [torch.empty(N, C, device=dev) for _ in range(3)]
    for cell, out in zip(cells, outs):
        _launch("kpgnn_dropout_fwd", x, out, p, st[:2], st[2:], cell)
    torch.cuda.synchronize()
    assert [int(c) for c in cells] == [0, 1, 2] and st.tolist() == [s, 3, 0]
    masks = [o != 0 for o in outs]
    for i, m in enumerate(masks):
        assert torch.equal(m, _exported_mask(N, C, p, s, i))
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2]) and not torch.equal(masks[0], masks[2])
    dx = torch.empty(N, C, device=dev)
    _launch("kpgnn_dropout_bwd", x, dx, p, st[:2], st[2:], cells[1])
    torch.cuda.synchronize()
    assert st.tolist() == [s, 3, 0] and torch.equal(dx != 0, masks[1])


@pytest.mark.gpu
@pytest.mark.parametrize("C", [104, 33])
@pytest.mark.parametrize("strided", [False, True])
def test_rows_beyond_n_dyn_are_left_alone(C, strided):
    """Capacity 257, *n_dyn = 180, `out` pre-filled with a sentinel and the dead rows of x and the residual holding NaN: rows
    >= 180 keep the sentinel bitwise and rows < 180 equal bitwise an N = 180 launch with the same seed and call id - the mask
    does not depend on the capacity."""
    dev = _dev()
    cap, live, p, seed, call = 257, 180, 0.5, 99, 4
    g = torch.Generator().manual_seed(C)
    wide, rwide = torch.randn(cap, C + 8, generator=g).to(dev), torch.randn(cap, C + 8, generator=g).to(dev)
    wide[live:], rwide[live:] = float("nan"), float("nan")
    x = wide[:, 4:4 + C] if strided else wide[:, :C].contiguous()
    res = rwide[:, 4:4 + C] if strided else rwide[:, :C].contiguous()
    cnt = torch.tensor([live], dtype=torch.int32, device=dev)
    for name in ENTRIES:
        r = res if name == "kpgnn_dropout_fwd" else None
        out = torch.full((cap, C), -7.0, device=dev)
        state, ticket = _state(seed, call)
        cell = torch.tensor([call], dtype=torch.int64, device=dev)
        _launch(name, x, out, p, state, ticket, cell, residual=r, n_dyn=cnt)
        exact = torch.full((live, C), -7.0, device=dev)
        state, ticket = _state(seed, call)
        _launch(name, x[:live], exact, p, state, ticket, cell, residual=None if r is None else r[:live])
        torch.cuda.synchronize()
        assert bool((out[live:] == -7.0).all()), name
        assert torch.equal(out[:live].view(torch.int32), exact.view(torch.int32)), name
        assert not bool(torch.isnan(exact).any())
