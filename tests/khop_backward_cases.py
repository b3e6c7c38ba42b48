"""The routes of KHopAggregate.backward (kp_gnn_amd/ops.py), one named case each, at the smallest shapes that take them.

A case builds its inputs from fixed seeds on cuda:0, runs forward and backward and returns (trace, grads):
  trace  the ordered kp_gnn_amd._lib.launch calls made DURING the backward call - the entry point and, for the launches of the
         aggregate backward, the descriptor fields that tell its routes apart (FIELDS below; a pointer is recorded as set / not
         set, never as an address);
  grads  name -> tensor, every gradient of every input or parameter that requires one.

tests/test_khop_backward_stages.py holds each trace to tests/golden/khop_backward_traces.json.  Not a test module itself:

    python tests/khop_backward_cases.py --record tests/golden/khop_backward_traces.json     # (re)write the fixture
    python tests/khop_backward_cases.py --dump DIR                                          # torch.save every case's gradients
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(_HERE), _HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIXTURE = os.path.join(_HERE, "golden", "khop_backward_traces.json")
SECOND_PASS = "<second backward pass>"


def _set(v):
    return bool(v)


# entry point -> descriptor -> recorded fields
FIELDS = {
    "kpgnn_table_grad": lambda d: dict(
        fuse_pre=_set(d.fuse_pre), fuse_gtheta=_set(d.fuse_gtheta), fuse_galphas=_set(d.fuse_galphas), tables=d.n_code0 > 0,
        n_dict=d.n_dict, dict_src=d.dict_src, accumulate_dict=d.accumulate_dict, extra_out=_set(d.extra_out),
        pending=_set(d.pending), storage=d.storage),
    "kpgnn_aggregate_bwd": lambda d: dict(
        accumulate_mask=d.accumulate_mask, use_tables=d.use_tables, gx=_set(d.gx), gx_slots=sum(1 for p in d.gx_slot if p)),
    "kpgnn_khop_pull_gather": lambda d: dict(K=d.K, hinit=_set(d.hinit), hinit2=_set(d.hinit2)),
    "kpgnn_dict_grad": lambda d: dict(defer_reduce=d.defer_reduce, K=d.K),
    "kpgnn_dict_grad_multi": lambda d: dict(L=d.L),
    "kpgnn_combine_bwd": lambda d: dict(
        mode=d.mode, gv=_set(d.gv), gtheta=_set(d.gtheta), galphas=_set(d.galphas), gh=_set(d.gh), periph=_set(d.periph),
        storage=d.storage),
}


def _entry(name, args):
    f = FIELDS.get(name)
    return [name, f(args[1]._obj) if f else {}]      # (args = (device, ctypes.byref(descriptor), ...))


class traced:
    """with traced(trace): ... - every _lib.launch inside the block is appended to `trace` (and still runs)."""

    def __init__(self, trace):
        self.trace = trace

    def __enter__(self):
        from kp_gnn_amd import _lib
        self.real = real = _lib.launch
        trace = self.trace

        def spy(name, *a, **k):
            trace.append(_entry(name, a))
            return real(name, *a, **k)

        _lib.launch = spy
        return trace

    def __exit__(self, *exc):
        from kp_gnn_amd import _lib
        _lib.launch = self.real


def _dev():
    assert torch.cuda.is_available(), "the cases need the MI355X"
    return torch.device("cuda:0")


def _backward(loss, trace=None, **kw):
    trace = [] if trace is None else trace
    with traced(trace):
        loss.backward(**kw)
    torch.cuda.synchronize()
    return trace


def _leaf(t):
    return t.clone().to(_dev()).requires_grad_(True)


def _grads(named):
    out = {}
    for k, v in named.items():
        if isinstance(v, (list, tuple)):
            out.update({f"{k}[{i}]": t.grad for i, t in enumerate(v)})
        else:
            out[k] = v.grad
    assert all(g is not None for g in out.values()), [k for k, g in out.items() if g is None]
    return {k: g.detach().clone() for k, g in out.items()}


# ------------------------------------------------------------------------------------------------------- layer-level cases
def _fused_inputs(nk):
    """test_gpu_parity.py::test_fused_backward_path_equals_separate_path_end_to_end: N=700, E=9000, K=6, D=104, U=9."""
    from kp_gnn_amd.khop_csr import KHopCSR
    dev = _dev()
    N, E, K, D, U = 700, 9000, 6, 104, 9
    g0 = torch.Generator().manual_seed(nk)
    ei = torch.randint(0, N, (2, E), generator=g0)
    ea = torch.zeros(E, K, dtype=torch.long)
    act = torch.rand(E, K, generator=g0) < 0.4
    ea[:, 0] = torch.randint(1, 5, (E,), generator=g0) * act[:, 0]
    ea[:, 1:] = torch.randint(1, nk, (E, K - 1), generator=g0) * act[:, 1:]
    csr = KHopCSR.build(ei.to(dev), ea.to(dev), N)
    base = dict(xs=[torch.randn(N, D, generator=g0) for _ in range(K)], t0=torch.randn(5, D, generator=g0) * 0.3,
                tk=torch.randn(nk, D, generator=g0) * 0.3, ptab=torch.randn(U, D, generator=g0), alphas=torch.randn(D, generator=g0))
    uid = torch.randint(0, U, (N, K), generator=g0, dtype=torch.int32).to(dev)
    w = torch.randn(N, D, generator=g0).to(dev)
    base["theta"] = torch.softmax(torch.randn(K, D, generator=g0), 0)
    return csr, K, base, uid, w


def _fused(nk, theta_matrix=False):
    from kp_gnn_amd import ops
    csr, K, base, uid, w = _fused_inputs(nk)
    base.pop("alphas" if theta_matrix else "theta")
    t = {k: ([_leaf(x) for x in v] if isinstance(v, list) else _leaf(v)) for k, v in base.items()}
    out = ops.khop_aggregate(t["xs"], csr, K, ops.MODE_GINPLUS, t["t0"], t["tk"], ops.DictPeripheral(t["ptab"], uid),
                             theta=t["theta" if theta_matrix else "alphas"])
    return _backward((out * w).sum()), _grads(t)


def fused_inwalk():
    return _fused(12)


def separate_oversize_tables():
    return _fused(1002)


def fused_theta_matrix():
    return _fused(12, theta_matrix=True)


def _sum_shared_dict(D):
    """test_gpu_parity.py::test_shared_dictionary_gradient_cell_unfused_paths with the dictionary marked as shared."""
    from kp_gnn_amd import ops
    from kp_gnn_amd.khop_csr import KHopCSR
    dev = _dev()
    N, K, U = 900, 4, 9
    E = 10 * N
    g0 = torch.Generator().manual_seed(D)
    ei = torch.randint(0, N, (2, E), generator=g0)
    ea = torch.randint(1, 6, (E, K), generator=g0) * (torch.rand(E, K, generator=g0) < 0.5)
    csr = KHopCSR.build(ei.to(dev), ea.to(dev), N)
    base = dict(x=torch.randn(N, K, D, generator=g0), t0=torch.randn(6, D, generator=g0) * 0.3,
                tk=torch.randn(6, D, generator=g0) * 0.3, ptab=torch.randn(U, D, generator=g0))
    uid = torch.randint(0, U, (N, K), generator=g0, dtype=torch.int32).to(dev)
    w = torch.randn(N, K, D, generator=g0).to(dev)
    t = {k: _leaf(v) for k, v in base.items()}
    ptab = t["ptab"] * 1.0
    ptab._kp_shared_grad = True
    periph = ops.DictPeripheral(ptab, uid)
    h = t["x"]
    for _ in range(3):
        h = torch.tanh(ops.khop_aggregate(h, csr, K, ops.MODE_SUM, t["t0"], t["tk"], periph))
    trace = _backward((h * w).sum())
    assert ptab._kp_grad_cell.buf is None
    return trace, _grads(t)


def sum_shared_dict_d13():
    return _sum_shared_dict(13)


def sum_shared_dict_d104():
    return _sum_shared_dict(104)


def _random_khop(N, E, K, seed, n0=5, nk=12, density=0.3):
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, size=(2, E))
    ea = np.zeros((E, K), dtype=np.int64)
    act = rng.random((E, K)) < density
    ea[:, 0] = rng.integers(2, n0, size=E) * act[:, 0]
    if K > 1:
        ea[:, 1:] = rng.integers(2, nk, size=(E, K - 1)) * act[:, 1:]
    return torch.from_numpy(ei), torch.from_numpy(ea)


def _modes(mode, eps_grad=False, theta=False, periph="dense"):
    """test_gpu_parity.py::test_aggregate_modes_and_widths_vs_oracle at D = 104: N=61, E=700, K=5."""
    from kp_gnn_amd import _lib, ops
    from kp_gnn_amd.khop_csr import KHopCSR
    dev = _dev()
    N, E, K, D, U = 61, 700, 5, 104, 9
    ei, ea = _random_khop(N, E, K, seed=D)
    g = torch.Generator().manual_seed(D * 7 + len(mode))
    x = torch.randn(N, K, D, generator=g)
    t0 = torch.randn(5, D, generator=g)
    tk = torch.randn(12, D, generator=g)
    t0[0] = 0
    tk[0] = 0
    P = torch.randn(N, K, D, generator=g)
    w = torch.randn(N, K, D, generator=g).to(dev)
    csr = KHopCSR.build(ei.to(dev), ea.to(dev), N)
    t = dict(x=_leaf(x), t0=_leaf(t0), tk=_leaf(tk))
    eps = None
    if mode == "gin":
        eps = torch.tensor([0.3]).to(dev)
        if eps_grad:
            eps = t["eps"] = eps.requires_grad_(True)
    if periph == "dense":
        per = t["P"] = _leaf(P)
    else:
        t["ptab"] = _leaf(torch.randn(U, D, generator=g))
        per = ops.DictPeripheral(t["ptab"], torch.randint(0, U, (N, K), generator=g, dtype=torch.int32).to(dev))
    if theta:
        t["theta"] = _leaf(torch.softmax(torch.randn(K, D, generator=g), 0))
        w = w[:, 0]
    m = {"gin": _lib.MODE_GIN, "ginplus": _lib.MODE_GINPLUS, "gcn": _lib.MODE_GCN, "sum": _lib.MODE_SUM}[mode]
    out = ops.khop_aggregate(t["x"], csr, K, m, table0=t["t0"], tablek=t["tk"], periph=per, eps=eps, theta=t.get("theta"))
    return _backward((out * w).sum()), _grads(t)


def gin_eps():
    return _modes("gin", eps_grad=True)


def ginplus_dense():
    return _modes("ginplus")


def gcn():
    return _modes("gcn")


def sum_dense():
    return _modes("sum")


def ginplus_dense_theta():
    return _modes("ginplus", theta=True)


def ginplus_dict_no_theta():
    return _modes("ginplus", periph="dict")


# -------------------------------------------------------------------------------------------------------- body-level cases
def _body(model_name, combine, graphs, large=False, K=3, H=32):
    import parity_f64 as PF
    from kp_gnn_amd.batch import synthetic_zinc_batch
    dev = _dev()
    model = PF.small_body(model_name, combine, K, 4, H).to(dev).train()
    b = synthetic_zinc_batch(graphs, seed0=11, K=K).to(dev)
    b.build_csr()
    assert (b.num_nodes >= 4096) == large, b.num_nodes
    return model, b


def _loss(model, b):
    return (model(b).squeeze() - b.y.squeeze()).abs().mean()


def _param_grads(model):
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _body_case(model_name, combine, graphs, large=False, **kh):
    model, b = _body(model_name, combine, graphs, large, **kh)
    return _backward(_loss(model, b)), _param_grads(model)


def plus_small():
    return _body_case("KPGINPlus", "geometric", 40)


def plus_large():
    return _body_case("KPGINPlus", "geometric", 300, large=True)


def plus_large_push():
    from kp_gnn_amd import ops
    prev, ops.PULL_GATHER = ops.PULL_GATHER, False
    try:
        return plus_large()
    finally:
        ops.PULL_GATHER = prev


def plus_large_dict_per_layer():
    from kp_gnn_amd import ops
    prev, ops.DICT_MULTI = ops.DICT_MULTI, False
    try:
        return plus_large()
    finally:
        ops.DICT_MULTI = prev


def plus_large_bf16():
    from kp_gnn_amd import ops
    prev = ops.set_storage_dtype(torch.bfloat16)
    try:
        return plus_large()
    finally:
        ops.set_storage_dtype(prev)


def plus_attention_small():
    return _body_case("KPGINPlus", "attention", 40)


def kpgin_small():
    # K = 4: KP-GIN splits the width over the hops, and a share is parked in the x_state cell only by the jumping-knowledge
    # projection's grouped kernels, which take the widths 32, 64, 104 and 128 - none a multiple of 3
    return _body_case("KPGIN", "geometric", 40, K=4)


def kpgcn_small():     # (the width split over K = 3 hops: 24, not 32)
    return _body_case("KPGCN", "geometric", 40, H=24)


def plus_large_partial_then_full():
    """test_gpu_parity.py::test_gradient_cells_survive_a_partial_backward at 300 graphs: a backward towards the last layer's
    parameters only (it parks shares that nothing of its pass collects), then the full one over the retained graph."""
    model, b = _body("KPGINPlus", "geometric", 300, large=True)
    loss = _loss(model, b)
    last = [p for n, p in model.named_parameters() if ".gnns.3.mlp." in n and p.requires_grad]
    assert last
    trace = []
    with traced(trace):
        part = torch.autograd.grad(loss, last, retain_graph=True)
    trace.append([SECOND_PASS, {}])
    _backward(loss, trace)
    grads = _param_grads(model)
    grads.update({f"partial[{i}]": g.detach().clone() for i, g in enumerate(part)})
    return trace, grads


CASES = {f.__name__: f for f in (
    fused_inwalk, separate_oversize_tables, fused_theta_matrix, sum_shared_dict_d13, sum_shared_dict_d104,
    gin_eps, ginplus_dense, gcn, sum_dense, ginplus_dense_theta, ginplus_dict_no_theta,
    plus_small, plus_large, plus_large_push, plus_large_dict_per_layer, plus_large_bf16,
    plus_attention_small, kpgin_small, kpgcn_small, plus_large_partial_then_full)}


# ------------------------------------------------------------------------------------- the route each case is named after
def _any(trace, name, **fields):
    return any(n == name and all(f.get(k) == v for k, v in fields.items()) for n, f in trace)


def _none(trace, *names):
    return not any(n in names for n, _ in trace)


FUSED = dict(fuse_pre=True)
ROUTES = {
    # the fused kernel with the dictionary rows in its walk, d/dalphas from the same launch
    "fused_inwalk": lambda t: _any(t, "kpgnn_table_grad", n_dict=9, dict_src=1, fuse_galphas=True, **FUSED)
        and _none(t, "kpgnn_combine_bwd", "kpgnn_dict_grad", "kpgnn_geo_theta_bwd"),
    # no fused kernel and no table_grad plan either: combine_bwd, the tables inside the gather, the dictionary from rows of
    # gout * theta (the last fallback of the table stage)
    "separate_oversize_tables": lambda t: _any(t, "kpgnn_combine_bwd", gh=True, galphas=True)
        and [(f["tables"], f["dict_src"]) for n, f in t if n == "kpgnn_table_grad"] == [(False, 2)]
        and _any(t, "kpgnn_aggregate_bwd", use_tables=1) and _none(t, "kpgnn_dict_grad"),
    "fused_theta_matrix": lambda t: _any(t, "kpgnn_table_grad", fuse_gtheta=True, fuse_galphas=False, **FUSED)
        and _none(t, "kpgnn_geo_theta_bwd"),
    # table_grad's own dictionary rows (dict_src 2: rows of g), written by the first layer to run, added to by the others
    "sum_shared_dict_d13": lambda t: [f["accumulate_dict"] for n, f in t if n == "kpgnn_table_grad"] == [0, 1, 1],
    "sum_shared_dict_d104": lambda t: [f["accumulate_dict"] for n, f in t if n == "kpgnn_table_grad"] == [0, 1, 1],
    "gin_eps": lambda t: _none(t, "kpgnn_combine_bwd") and _any(t, "kpgnn_table_grad", fuse_pre=False, n_dict=0),
    "ginplus_dense": lambda t: _any(t, "kpgnn_combine_bwd", gh=False, gv=False),
    "gcn": lambda t: _any(t, "kpgnn_combine_bwd", gh=False) and _any(t, "kpgnn_aggregate_bwd", use_tables=1) and _none(t, "kpgnn_table_grad"),
    "sum_dense": lambda t: _none(t, "kpgnn_combine_bwd") and _any(t, "kpgnn_table_grad", fuse_pre=False),
    "ginplus_dense_theta": lambda t: _any(t, "kpgnn_combine_bwd", gh=True, gv=True, gtheta=True, periph=True),
    # dL/dP = gout: one table_grad for the tables (rows of g), one for the dictionary (rows of gout)
    "ginplus_dict_no_theta": lambda t: _any(t, "kpgnn_combine_bwd", gh=False)
        and [(f["tables"], f["n_dict"], f["dict_src"]) for n, f in t if n == "kpgnn_table_grad"] == [(True, 0, 0), (False, 9, 2)],
    # push form with slot cells, the dictionary in the walk, added to the cell's buffer by every layer but the first to run
    "plus_small": lambda t: _any(t, "kpgnn_table_grad", accumulate_dict=1, dict_src=1, **FUSED)
        and _any(t, "kpgnn_table_grad", accumulate_dict=0, dict_src=1, **FUSED) and _any(t, "kpgnn_aggregate_bwd", gx=False)
        and _none(t, "kpgnn_khop_pull_gather", "kpgnn_dict_grad", "kpgnn_dict_grad_multi"),
    "plus_large": lambda t: sum(n == "kpgnn_dict_grad_multi" for n, _ in t) == 1 and _any(t, "kpgnn_khop_pull_gather", hinit2=True)
        and _any(t, "kpgnn_table_grad", n_dict=0, **FUSED) and _none(t, "kpgnn_dict_grad"),
    "plus_large_push": lambda t: _none(t, "kpgnn_khop_pull_gather") and _any(t, "kpgnn_dict_grad_multi"),
    "plus_large_dict_per_layer": lambda t: _none(t, "kpgnn_dict_grad_multi") and _any(t, "kpgnn_dict_grad", defer_reduce=1)
        and _any(t, "kpgnn_table_grad", extra_out=True, **FUSED),
    "plus_large_bf16": lambda t: _any(t, "kpgnn_table_grad", storage=1, **FUSED) and _any(t, "kpgnn_aggregate_bwd"),
    # unfused epilogue: the attention combine hands back a node-major [N,k,D] gradient
    "plus_attention_small": lambda t: _any(t, "kpgnn_combine_bwd", gh=False) and _none(t, "kpgnn_khop_pull_gather"),
    # the x_state cell: the gather adds into the state's buffer
    "kpgin_small": lambda t: _any(t, "kpgnn_aggregate_bwd", gx=True, accumulate_mask=15),
    "kpgcn_small": lambda t: _any(t, "kpgnn_aggregate_bwd", use_tables=1),
    "plus_large_partial_then_full": lambda t: [SECOND_PASS, {}] in t and _any(t[t.index([SECOND_PASS, {}]):], "kpgnn_dict_grad_multi", L=4),
}
assert ROUTES.keys() == CASES.keys()


def main(argv):
    import json
    import time
    mode, target = argv
    assert mode in ("--record", "--dump"), __doc__
    traces, off_route = {}, []
    if mode == "--dump":
        os.makedirs(target, exist_ok=True)
    for name, case in CASES.items():
        t0 = time.perf_counter()
        trace, grads = case()
        print(f"{name}: {len(trace)} launches, {len(grads)} gradients, {time.perf_counter() - t0:.2f} s", flush=True)
        if not ROUTES[name](trace):
            off_route.append(name)
        traces[name] = trace
        if mode == "--dump":
            torch.save({k: v.cpu() for k, v in grads.items()}, os.path.join(target, name + ".pt"))
    if mode == "--record":
        with open(target, "w") as f:
            f.write("{\n" + ",\n".join(f' "{n}": [\n' + ",\n".join("  " + json.dumps(e) for e in t) + "\n ]" for n, t in traces.items())
                    + "\n}\n")
    assert not off_route, ("not on the route they are named after", off_route)


if __name__ == "__main__":
    main(sys.argv[1:])
