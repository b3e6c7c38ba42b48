"""kpgnn_jk_reduce_fwd / _bwd (csrc/jk_reduce.hip) through the C ABI.

CPU: both entries reject malformed descriptors before any device call, N == 0 launches nothing, the binding matches the header,
and CPU tensors keep today's torch.stack expressions bit for bit.  GPU: MAX is bitwise the framework's max with the documented
tie rule (lowest slot) and NaN propagation, SUM is deterministic and independent of the launch geometry, SOFTMAX is held to the
float64 framework expression and its autograd with the fp32 CPU evaluation as the yardstick, and rows beyond *n_dyn are left
alone in every output of both directions."""
import ctypes

import pytest
import torch

import parity_f64 as PF

A = 0x10000                                       # dummy, non-NULL, 16-B aligned: never dereferenced
OK, EINVAL = 0, -1
SUM, MAX, SOFTMAX = 0, 1, 2
FWD, BWD = "kpgnn_jk_reduce_fwd", "kpgnn_jk_reduce_bwd"
RTOL, ATOL = PF.RTOL, PF.ATOL
M_F64 = 3
# one row; the scalar path with rows that straddle the lane groups; a width that is no multiple of 4; 64 lanes of 16 B; more than
# one block; S beyond 16; the maximal S - and two shapes whose rows are wider than 64 lanes reach in one pass (the column loop:
# 65 scalar columns, 260 = 65 x 4 vector columns)
SHAPES = [(1, 104, 9), (257, 6, 2), (257, 33, 3), (300, 256, 2), (5000, 104, 9), (129, 96, 18), (65, 32, 32),
          (70, 65, 3), (40, 260, 2)]


@pytest.fixture(scope="module")
def lib():
    from kp_gnn_amd import _lib, build
    build.build_all()
    return _lib.load()


def _desc(N=100, H=32, S=3, mode=MAX, **kw):
    """A descriptor that passes every check of both entries (all pointers dummies); kw overrides, x={l: pointer} per slot."""
    from kp_gnn_amd import _lib
    d = _lib.JkDesc()
    d.N, d.H, d.S, d.mode = N, H, S, mode
    for l in range(min(max(S, 0), 32)):
        d.x[l] = A
    d.x_stride, d.out, d.out_stride, d.score, d.arg, d.w = H, A, H, A, A, A
    d.gout, d.gout_stride, d.gx, d.gscore = A, H, A, A
    for k, v in kw.items():
        if k == "x":
            for l, q in v.items():
                d.x[l] = q
        else:
            setattr(d, k, v)
    return d


# ------------------------------------------------------------------------------------------------ CPU
COMMON_BAD = [dict(S=0), dict(S=-1), dict(S=33), dict(H=0), dict(H=-8), dict(N=-1), dict(mode=3), dict(mode=-1)]
FWD_BAD = COMMON_BAD + [dict(x={0: None}), dict(x={2: None}), dict(out=None), dict(x_stride=31), dict(out_stride=31),
                        dict(out_stride=-32), dict(mode=SOFTMAX, score=None), dict(mode=SUM, x={1: None})]
BWD_BAD = COMMON_BAD + [dict(gout=None), dict(gx=None), dict(gout_stride=31), dict(mode=MAX, arg=None), dict(mode=SOFTMAX, w=None),
                        dict(mode=SOFTMAX, gscore=None), dict(mode=SOFTMAX, x={1: None}), dict(mode=SOFTMAX, x_stride=31),
                        dict(mode=SUM)]


def test_null_descriptors_are_rejected(lib):
    for name in (FWD, BWD):
        assert getattr(lib, name)(None, None) == EINVAL, name
        assert name.encode() + b": NULL descriptor" in lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", FWD_BAD, ids=repr)
def test_malformed_forward_descriptors_are_rejected(lib, kw):
    """-1 with a message naming the entry, before any device call (the stream is NULL and every pointer a dummy)."""
    assert lib.kpgnn_jk_reduce_fwd(ctypes.byref(_desc(**kw)), None) == EINVAL, kw
    assert FWD.encode() in lib.kpgnn_last_error(), lib.kpgnn_last_error()


@pytest.mark.parametrize("kw", BWD_BAD, ids=repr)
def test_malformed_backward_descriptors_are_rejected(lib, kw):
    assert lib.kpgnn_jk_reduce_bwd(ctypes.byref(_desc(**kw)), None) == EINVAL, kw
    assert BWD.encode() in lib.kpgnn_last_error(), lib.kpgnn_last_error()
    if kw == dict(mode=SUM):
        assert b"SUM has no backward kernel" in lib.kpgnn_last_error()


def test_what_an_entry_does_not_use_may_be_null(lib):
    """With N == 0 nothing is launched, so a descriptor that passes validation returns 0: the forward needs no arg / w / gout,
    a MAX backward no states, out or score."""
    for mode in (SUM, MAX, SOFTMAX):
        assert lib.kpgnn_jk_reduce_fwd(ctypes.byref(_desc(N=0, mode=mode)), None) == OK, mode
        d = _desc(N=0, mode=mode, arg=None, w=None, gout=None, gx=None, gscore=None, score=A if mode == SOFTMAX else None)
        assert lib.kpgnn_jk_reduce_fwd(ctypes.byref(d), None) == OK, mode
    assert lib.kpgnn_jk_reduce_bwd(ctypes.byref(_desc(N=0, mode=MAX)), None) == OK
    assert lib.kpgnn_jk_reduce_bwd(ctypes.byref(_desc(N=0, mode=SOFTMAX)), None) == OK
    d = _desc(N=0, mode=MAX, x={0: None, 1: None, 2: None}, out=None, score=None, w=None, gscore=None)
    assert lib.kpgnn_jk_reduce_bwd(ctypes.byref(d), None) == OK
    assert lib.kpgnn_jk_reduce_fwd(ctypes.byref(_desc(N=0, S=32)), None) == OK       # the maximal S is accepted


def test_the_entries_are_bound(lib):
    from kp_gnn_amd import _lib
    names = [f[0] for f in _lib.JkDesc._fields_]
    assert names == ["N", "H", "S", "mode", "x", "x_stride", "score", "out", "out_stride", "arg", "w", "gout", "gout_stride",
                     "gx", "gscore", "n_dyn"]
    assert _lib.JkDesc.x.size == 32 * ctypes.sizeof(ctypes.c_void_p) and _lib.JK_MAX_STATES == 32
    assert (_lib.JK_SUM, _lib.JK_MAX, _lib.JK_SOFTMAX) == (SUM, MAX, SOFTMAX)
    for name in (FWD, BWD):
        assert getattr(lib, name).argtypes[0] == ctypes.POINTER(_lib.JkDesc)


def test_the_switch_is_on_by_default_and_cpu_tensors_keep_the_framework_expression():
    from kp_gnn_amd import ops
    assert ops.native_jk() is True and all(ops.native_jk(m) for m in ("sum", "max", "softmax"))
    g = torch.Generator().manual_seed(5)
    states = [torch.randn(7, 12, generator=g, requires_grad=True) for _ in range(4)]
    score = torch.randn(7, 4, generator=g, requires_grad=True)
    assert not ops.jk_native_applies(states) and not ops.jk_native_applies([])
    exprs = {"sum": lambda: torch.stack(states, dim=0).sum(dim=0),
             "max": lambda: torch.stack(states, dim=-1).max(dim=-1).values,
             "softmax": lambda: (torch.stack(states, dim=1) * torch.softmax(score, dim=1).unsqueeze(-1)).sum(1)}
    go = torch.randn(7, 12, generator=g)
    for mode, expr in exprs.items():
        got = ops.jk_reduce(states, mode, score if mode == "softmax" else None)
        want = expr()
        assert torch.equal(got, want), mode
        ga = torch.autograd.grad(got, states, go)
        gw = torch.autograd.grad(want, states, go)
        assert all(torch.equal(a, b) for a, b in zip(ga, gw)), mode
    with pytest.raises(ValueError):
        ops.jk_reduce(states, "mean")
    with pytest.raises(ValueError):
        ops.jk_reduce(states, "softmax")
    with pytest.raises(ValueError):
        ops.jk_reduce(states, "sum", score)
    prev = ops.set_native_jk(False, "max")
    try:
        assert prev is True and ops.native_jk("max") is False and ops.native_jk("sum") is True and ops.native_jk() is False
    finally:
        ops.set_native_jk(True)
    assert ops.native_jk() is True


# ------------------------------------------------------------------------------------------------ GPU
def _dev():
    return torch.device("cuda:0")


def _launch(name, mode, N, H, S, states=None, score=None, out=None, arg=None, w=None, gout=None, gx=None, gscore=None,
            n_dyn=None):
    from kp_gnn_amd import _lib
    d = _lib.JkDesc()
    d.N, d.H, d.S, d.mode = N, H, S, mode
    if states is not None:
        assert len(states) == S
        for l, t in enumerate(states):
            assert t.stride(1) == 1 and t.stride(0) == states[0].stride(0) and t.shape[0] >= N and t.shape[1] == H
            d.x[l] = t.data_ptr()
        d.x_stride = states[0].stride(0)
    for k, t in (("score", score), ("out", out), ("arg", arg), ("w", w), ("gout", gout), ("gx", gx), ("gscore", gscore),
                 ("n_dyn", n_dyn)):
        if t is not None:
            setattr(d, k, t.data_ptr())
    if out is not None:
        d.out_stride = out.stride(0)
    if gout is not None:
        d.gout_stride = gout.stride(0)
    _lib.launch(name, _dev(), ctypes.byref(d))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _routed(gout, idx, S):
    """[S,N,H]: gout in block idx[n,c], 0.0 elsewhere."""
    return torch.stack([torch.where(idx == l, gout, torch.zeros_like(gout)) for l in range(S)])


def _max_roundtrip(states, gout):
    """(out, arg, gx) of a MAX forward + backward on the device, every output pre-filled with a sentinel."""
    dev = _dev()
    S, (N, H) = len(states), states[0].shape
    xs = [t.to(dev) for t in states]
    out = torch.full((N, H), -7.0, device=dev)
    arg = torch.full((N, H), 255, dtype=torch.uint8, device=dev)
    gx = torch.full((S, N, H), -7.0, device=dev)
    _launch(FWD, MAX, N, H, S, states=xs, out=out, arg=arg)
    _launch(BWD, MAX, N, H, S, arg=arg, gout=gout.to(dev), gx=gx)
    torch.cuda.synchronize()
    return out.cpu(), arg.cpu().long(), gx.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,S", SHAPES)
def test_max_is_the_frameworks_max_bit_for_bit(N, H, S):
    """Random normal states without a tie for the top (asserted on the host): out is bitwise torch.stack(states, -1).max(-1)
    on the CPU, arg its argmax, gx the gradient routed by that arg (bitwise: copies of gout and zeros)."""
    g = torch.Generator().manual_seed(1000 * S + H)
    states = [torch.randn(N, H, generator=g) for _ in range(S)]
    gout = torch.randn(N, H, generator=g)
    stack = torch.stack(states, -1)
    if S > 1:
        top2 = stack.topk(2, dim=-1).values
        assert bool((top2[..., 0] > top2[..., 1]).all()), "the inputs hold a tie for the top"
    out, arg, gx = _max_roundtrip(states, gout)
    ref = stack.max(-1)
    assert torch.equal(_bits(out), _bits(ref.values))
    assert torch.equal(arg, ref.indices)
    assert torch.equal(_bits(gx), _bits(_routed(gout, ref.indices, S)))


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,S", SHAPES)
def test_max_gives_a_tie_to_the_lowest_slot_and_propagates_nan(N, H, S):
    """States from randint(-2, 3) * 0.5 (five values: ties everywhere), the last row all-equal, and a NaN in a middle slot of
    one element.  Reference: the first slot that equals the maximum (torch.argmax returns the first occurrence).  arg equals
    it and the gradient goes to that slot only; the element with the NaN gives NaN (its arg is unspecified and not compared)."""
    g = torch.Generator().manual_seed(1000 * S + H + 1)
    states = [torch.randint(-2, 3, (N, H), generator=g).float() * 0.5 for _ in range(S)]
    for t in states:
        t[N - 1] = 0.5
    gout = torch.randn(N, H, generator=g)
    clean = torch.stack(states, -1)
    idx = (clean == clean.max(-1, keepdim=True).values).int().argmax(-1)
    assert bool((idx[N - 1] == 0).all())
    if S > 1:
        assert N * H < 64 or int((clean == clean.max(-1, keepdim=True).values).sum(-1).max()) > 1, "the inputs hold no tie"
    nr, nc, nl = 0, H // 2, S // 2
    states[nl][nr, nc] = float("nan")
    out, arg, gx = _max_roundtrip(states, gout)
    assert bool(torch.isnan(out[nr, nc])), float(out[nr, nc])
    keep = torch.ones(N, H, dtype=torch.bool)
    keep[nr, nc] = False
    assert int(torch.isnan(out).sum()) == 1
    assert torch.equal(out[keep], clean.max(-1).values[keep])
    assert torch.equal(arg[keep], idx[keep])
    want = _routed(gout, idx, S)
    assert torch.equal(_bits(gx[:, keep]), _bits(want[:, keep]))
    assert int((gx[:, keep] != 0).sum(0).max()) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,S", SHAPES)
def test_sum_is_deterministic_and_independent_of_the_capacity(N, H, S):
    """Against the float64 sum at the golden tolerances; a second launch gives the same bits; the same rows at the head of a
    larger buffer (another grid, other rows per block in flight) give the same bits in the live rows."""
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * S + H + 2)
    cap = N + 43
    big = [torch.randn(cap, H, generator=g) for _ in range(S)]
    states = [t[:N].contiguous().to(dev) for t in big]
    outs = [torch.full((N, H), -7.0, device=dev) for _ in range(2)]
    for o in outs:
        _launch(FWD, SUM, N, H, S, states=states, out=o)
    wide = torch.full((cap, H), -7.0, device=dev)
    _launch(FWD, SUM, cap, H, S, states=[t.to(dev) for t in big], out=wide)
    torch.cuda.synchronize()
    ref = torch.stack([t[:N].double() for t in big]).sum(0)
    err = (outs[0].cpu().double() - ref).abs()
    bound = ATOL * float(ref.abs().max()) + RTOL * ref.abs()
    print(f"sum N{N} H{H} S{S}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.equal(_bits(wide[:N]), _bits(outs[0]))


def _softmax_reference(score, states, gout, dtype):
    xs = [t.to(dtype).requires_grad_(True) for t in states]
    sc = score.to(dtype).requires_grad_(True)
    w = torch.softmax(sc, dim=1)
    out = (torch.stack(xs, dim=1) * w.unsqueeze(-1)).sum(1)
    grads = torch.autograd.grad(out, [sc] + xs, gout.to(dtype))
    res = {"out": out.detach(), "w": w.detach(), "gscore": grads[0]}
    res.update({f"d{l}": gl for l, gl in enumerate(grads[1:])})
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("N,H,S", SHAPES)
def test_softmax_vs_float64(N, H, S):
    """score = 2 randn, states = randn, gout = randn (generator seeded 1000 S + H).  out, w, every gx[l] (d0 ..) and gscore
    through close_to_f64 with M = 3: ref64 is the framework expression (stack * softmax(score)[..., None]).sum(1) and its
    autograd in float64 on the CPU, the yardstick the same in fp32 on the CPU.  Measured on the MI355X (E32 / gscale; the largest
    |ours - float64| / max(e32_k, 0.1 E32) and its tensor), every tensor inside the bound - where the ratio exceeds M the
    golden floor ATOL * max(|ref_k|, 0.1 gscale) + RTOL |ref_k| is the larger term, the fp32 yardstick being ~1e-7 of the scale:
        (1,104,9) 1.0e-7 1.00    (257,6,2) 1.3e-7 1.00    (257,33,3) 2.4e-7 1.00    (300,256,2) 1.4e-7 1.79 gscore
        (5000,104,9) 5.2e-7 1.00    (129,96,18) 1.4e-7 5.18 d2    (65,32,32) 2.2e-7 7.06 gscore
        (70,65,3) 1.4e-7 1.00    (40,260,2) 1.5e-7 2.36 gscore"""
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * S + H)
    score = 2.0 * torch.randn(N, S, generator=g)
    states = [torch.randn(N, H, generator=g) for _ in range(S)]
    gout = torch.randn(N, H, generator=g)
    ref64 = _softmax_reference(score, states, gout, torch.float64)
    ref32 = _softmax_reference(score, states, gout, torch.float32)
    xs = [t.to(dev) for t in states]
    out, w = torch.full((N, H), -7.0, device=dev), torch.full((N, S), -7.0, device=dev)
    gx, gscore = torch.full((S, N, H), -7.0, device=dev), torch.full((N, S), -7.0, device=dev)
    _launch(FWD, SOFTMAX, N, H, S, states=xs, score=score.to(dev), out=out, w=w)
    _launch(BWD, SOFTMAX, N, H, S, states=xs, w=w, gout=gout.to(dev), gx=gx, gscore=gscore)
    torch.cuda.synchronize()
    got = {"out": out, "w": w, "gscore": gscore}
    got.update({f"d{l}": gx[l] for l in range(S)})
    PF.print_ratios(f"jk softmax N{N} H{H} S{S}", PF.close_to_f64(got, ref64, [ref32], f"jk softmax N{N} H{H} S{S}", M_F64))
    # without w the forward gives the same bits (nothing is saved when no backward follows)
    out2 = torch.full((N, H), -7.0, device=dev)
    _launch(FWD, SOFTMAX, N, H, S, states=xs, score=score.to(dev), out=out2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(out2))


@pytest.mark.gpu
@pytest.mark.parametrize("H", [33, 104])
@pytest.mark.parametrize("mode", [SUM, MAX, SOFTMAX])
def test_rows_beyond_n_dyn_are_left_alone(mode, H):
    """Capacity 300, *n_dyn = 257, every output of both directions pre-filled with a sentinel, the dead rows of every input
    holding NaN: rows >= 257 keep the sentinel and rows < 257 equal bitwise the exact-shape launch (H = 33: the scalar path by
    rows; 104: 16-byte accesses, and for SUM / MAX the rows as one run)."""
    dev = _dev()
    cap, live, S = 300, 257, 3
    g = torch.Generator().manual_seed(100 * mode + H)
    states = [torch.randn(cap, H, generator=g).to(dev) for _ in range(S)]
    score, gout = torch.randn(cap, S, generator=g).to(dev), torch.randn(cap, H, generator=g).to(dev)
    for t in states + [score, gout]:
        t[live:] = float("nan")
    cnt = torch.tensor([live], dtype=torch.int32, device=dev)

    def run(N, n_dyn):
        o = dict(out=torch.full((N, H), -7.0, device=dev), gx=torch.full((S, N, H), -7.0, device=dev))
        if mode == MAX:
            o["arg"] = torch.full((N, H), 99, dtype=torch.uint8, device=dev)
        if mode == SOFTMAX:
            o["w"], o["gscore"] = torch.full((N, S), -7.0, device=dev), torch.full((N, S), -7.0, device=dev)
        xs = [t[:N] for t in states]
        _launch(FWD, mode, N, H, S, states=xs, score=score[:N] if mode == SOFTMAX else None, out=o["out"], arg=o.get("arg"),
                w=o.get("w"), n_dyn=n_dyn)
        if mode != SUM:
            _launch(BWD, mode, N, H, S, states=xs if mode == SOFTMAX else None, arg=o.get("arg"), w=o.get("w"), gout=gout[:N],
                    gx=o["gx"], gscore=o.get("gscore"), n_dyn=n_dyn)
        torch.cuda.synchronize()
        return o

    got, exact = run(cap, cnt), run(live, None)
    for k, t in got.items():
        sentinel = 99 if k == "arg" else -7.0
        rows = t[:, :live] if k == "gx" else t[:live]
        dead = t[:, live:] if k == "gx" else t[live:]
        assert bool((dead == sentinel).all()), (k, "a dead row was written")
        if mode == SUM and k == "gx":
            assert bool((t == sentinel).all())          # (SUM has no backward launch)
            continue
        assert not bool(torch.isnan(exact[k].float()).any()), k
        assert torch.equal(rows.contiguous().view(torch.uint8), exact[k].view(torch.uint8)), (k, "the live rows depend on the capacity")
        assert not bool((rows == sentinel).all()), k
