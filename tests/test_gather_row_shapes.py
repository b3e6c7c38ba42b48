"""GPU (-m gpu): every kernel behind kpgnn_aggregate_fwd / kpgnn_aggregate_bwd, and every row shape of the sub-group kernels,
against float64 on the hard K-hop CSRs of tests/gather_cases.py (empty node, empty hops, one-pair hops, hops that end exactly
at a chunk end, a hop that starts one pair before a chunk end and spans three chunks, G + 1 pairs in every hop, self and
repeated pairs; the last node of the batch is such a long one).  Launches go through _lib.AggFwdDesc / _lib.AggBwdDesc and
_lib.launch; the kernel that served a launch is read off kpgnn_agg_launch_counts and asserted for EVERY launch.

Bounds: test_gpu_parity._close with TOL["aggregate"] (out / grad_x / grad_table0 / grad_tablek), no new tolerance; mode SUM
without tables, bias or P is additionally held per element to 2 n 2^-24 sum|addends| (test_pull_gather_kernel.py's bound).

Cases, the instantiation each is meant to reach and the line of csrc/aggregate.hip that sends it there
(kpgnn_aggregate_fwd: narrow / small are skipped with n_dyn at :773-775, the LDS kernel refuses n_dyn, aggregate_lds.hip:106;
kpgnn_aggregate_bwd: :895 and :921; row shape by dispatch_row_shape<64> at :830 / :930 from row_vec / row_lanes):

SHAPES (VEC, G) <- D [, floats x / g sits off a 16-byte boundary]:
  (4,4) 16   (4,8) 20   (4,16) 40   (4,32) 104   (4,64) 256      (2,4) 6   (2,8) 10   (2,16) 18   (2,32) 34   (2,64) 66
  (1,4) 3    (1,8) 5    (1,16) 13   (1,32) 17    (1,64) 33       (2,8) 16 off 2   (1,16) 16 off 1

test_subgroup_forward[shape], n_dyn = N, one launch per named case (TAB by :763, GCN / TAB / FAST by launch_fwd_mode :681-686):
  gin_plain                agg_fwd_kernel<VEC,G,false,0>  K = G - 1 (lane_meta, :191), chunked loop, GIN self term, `out`
  gin_tabL_dense_xbias     <VEC,G,false,1>  K = G (lane_meta false), tables in LDS, dense periph, xbias * seglen
  ginplus_fast_slots       <VEC,G,false,1,FAST> (:817: theta staged, K < G)  per-hop slots, dictionary, given theta, S saved
  ginplus_alphas_dictbig   <VEC,G,false,1> for G <= 16 (K = G), FAST for G >= 32 (K = 16); dictionary above the 36 KiB cap (:820),
                           theta from alphas (in LDS, or geo_theta_fwd_launch :826 where K * D floats miss the cap)
  ginplus_theta_dict_strided  <VEC,G,false,1>  no S saved: generic epilogue, dictionary staged in LDS, x a strided view
  ginplus_K1_alphas        <VEC,G,false,1,FAST>  K = 1
  sum_K1_of_3_strided      <VEC,G,false,0>  K = 1 < K_csr = 3
  sum_plain                <VEC,G,false,0>  K = G, plus the derived per-element bound
  sum_dict_notab_theta     <VEC,G,false,0>  dictionary and theta read from global memory
  gcn_plain                <VEC,G,true,0>   per-hop loop: dis weights, self term
  gcn_tabL_dense_xbias     <VEC,G,true,1>   K = G: wacc * xbias, self-loop code row 1
  gcn_tabL_theta           <VEC,G,true,1>   K = 16 where G <= 16 else G - 1, hout
  gin_tabG_dense / gcn_tabG / ginplus_tabG_dict_theta   <VEC,G,*,2> at D = 256, 104, 13: (n_code0 + n_codek) D 4 > 96 KiB (:763)
test_subgroup_backward[shape], n_dyn = N (launch_bwd_mode :711-718):
  sum_chunked              agg_bwd_kernel<VEC,G,false,0>  CHUNKED (:480), K = G - 1, derived bound
  gin_chunked_slots        <VEC,G,false,0>  nself one hop ahead, slot outputs
  ginplus_slots_acc        <VEC,G,false,0>  K = min(G, 16) (lane_meta false for G <= 16, :475), nold one hop ahead
  gin_stacked_gxacc        <VEC,G,false,0,false,GXACC> (:711)  K = min(G, 32)
  gin_tabL                 <VEC,G,false,1>  per-hop loop, table-gradient atomics in LDS
  sum_tabL_slots_acc       <VEC,G,false,1>  the per-hop loop's own accumulate
  gcn_plain                <VEC,G,true,0>
  gcn_tabL                 <VEC,G,true,1>   K = G, self-loop row of the table gradients
  sum_K1_of_3              <VEC,G,false,0>  K = 1 < K_csr = 3
  gin_tabG / gcn_tabG      <VEC,G,*,2> at D = 256, 104, 13: global atomics
test_tile_counts[N]: (4,4) at 1, 7, 8 and 9 tiles of 64 nodes (pick_grid :645 rounds the grid to a multiple of 8).
test_narrow_*: agg_narrow_kernel<TAB> (aggregate_narrow.hip:122-124, :145-146), D = 1, 6, 13, 32.
test_small_*:  agg_fwd_small_kernel / agg_bwd_small_kernel (aggregate_small.hip:203-209, :232-234), D = 4, 104, 128, K = 1, 8.
test_lds_forward: agg_lds_fwd_kernel<D / 4> (aggregate_lds.hip:103-113), D = 4, 16, 64; a one-node graph, a three-node graph
  (fewer nodes than the CH = 8 destination chunks), graphs of 9 and N - 13 nodes that hold the special nodes.
Each of the three is also compared bit for bit with the sub-group kernel on the same descriptor with n_dyn = N, and launched
twice (identical bits).  Where the headers do not promise equal bits the pair is held to float64 alone (SAME_SUMS_ONLY)."""
import ctypes
import functools

import pytest
import torch

import gather_cases as GC
from gather_cases import MODE_GCN, MODE_GIN, MODE_GINPLUS, MODE_SUM
from test_gpu_parity import TOL, _close, _dev

pytestmark = pytest.mark.gpu

SUB, NARROW, SMALL, LDS = 0, 1, 2, 3        # include/kpgnn.h KPGNN_AGG_ROUTE_*
N0 = 5                                      # rows of table0 everywhere
NK_LDS = 7                                  # rows of tablek where the tables fit LDS
MAX_LDS_TABLE_BYTES = 96 * 1024             # aggregate.hip kMaxLdsTableBytes
SIDE_TABLE_CAP = 36 * 1024                  # aggregate.hip: cap of tables + theta + dictionary in LDS

# (D, floats off a 16-byte boundary, VEC, G)
SHAPES = [(16, 0, 4, 4), (20, 0, 4, 8), (40, 0, 4, 16), (104, 0, 4, 32), (256, 0, 4, 64),
          (6, 0, 2, 4), (10, 0, 2, 8), (18, 0, 2, 16), (34, 0, 2, 32), (66, 0, 2, 64),
          (3, 0, 1, 4), (5, 0, 1, 8), (13, 0, 1, 16), (17, 0, 1, 32), (33, 0, 1, 64),
          (16, 2, 2, 8), (16, 1, 1, 16)]
SHAPE_IDS = [f"D{d}" + (f"off{o}" if o else "") + f"-v{v}g{g}" for d, o, v, g in SHAPES]


def _row_shape(D, off):
    """row_vec / row_lanes of kpgnn_common.h for a row of D floats whose least aligned operand sits `off` floats off 16 bytes"""
    v = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    while v > 1 and (off * 4) % (v * 4):
        v >>= 1
    g = 4
    while g * v < D:
        g <<= 1
    return v, g


def test_shape_table_is_the_dispatch_table():
    assert sorted({(v, g) for _, _, v, g in SHAPES}) == sorted((v, g) for v in (1, 2, 4) for g in (4, 8, 16, 32, 64))
    for D, off, v, g in SHAPES:
        assert _row_shape(D, off) == (v, g)


def _nk(tables, D):
    if tables != "global":
        return NK_LDS
    nk = MAX_LDS_TABLE_BYTES // (4 * D) - N0 + 1
    assert (N0 + nk) * D * 4 > MAX_LDS_TABLE_BYTES
    return nk


@functools.lru_cache(maxsize=None)
def _csr(N, K_csr, G, seed, nk=NK_LDS, graph_ptr=None):
    return GC.hard_csr(N, K_csr, G, GC.prefetch_depth(G), seed, n_code0=N0, n_codek=nk, graph_ptr=graph_ptr)


def _place(t, dev, off=0):
    """`t` on the device, its first element `off` floats behind a 256-byte aligned allocation"""
    if not off:
        return t.to(dev).contiguous()
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device=dev)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    return v


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


class _Routes:
    """asserts that a launch advanced exactly one counter of kpgnn_agg_launch_counts"""

    def __init__(self):
        from kp_gnn_amd import _lib
        self._lib = _lib
        self.before = _lib.agg_launch_counts()

    def expect(self, bwd, route, label):
        after = self._lib.agg_launch_counts()
        want = [list(self.before[0]), list(self.before[1])]
        want[bwd][route] += 1
        assert [list(after[0]), list(after[1])] == want, (label, "route counters (fwd, bwd)", self.before, after)
        assert self._lib.load().kpgnn_agg_lds_launch_count() == after[0][LDS]
        assert after[1][LDS] == 0
        self.before = after


# ------------------------------------------------------------------------------------------------------------ forward
def _fwd_case(mode, K, K_csr=None, tables=None, P=None, outform="out", xbias=False, xform="stacked", pre=False):
    return dict(mode=mode, K=K, K_csr=K_csr or K, tables=tables, P=P, outform=outform, xbias=xbias, xform=xform, pre=pre)


def _fwd_inputs(c, D, case, seed):
    """CPU fp32 inputs of one case and its float64 reference"""
    N, K = c.N, case["K"]
    g = torch.Generator().manual_seed(77 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    i = dict(x=r(N, K, D))
    nk = _nk(case["tables"], D)
    if case["tables"]:
        i["t0"], i["tk"] = r(N0, D) * 0.3, (r(nk, D) * 0.3 if K > 1 else None)
    if case["xbias"]:
        i["xbias"] = r(D) * 0.5
    if case["mode"] == MODE_GIN:
        i["eps"] = 0.3
    if case["mode"] == MODE_GCN:
        i["dis"] = GC.degree_dis(c).float()
    if case["P"] == "dense":
        i["periph"] = r(N, K, D)
    elif case["P"]:
        n_dict = 3 if case["P"] == "dict" else SIDE_TABLE_CAP // (4 * D) + 1
        i["ptab"] = r(n_dict, D)
        ii, kk = torch.arange(N).unsqueeze(1), torch.arange(K + 1).unsqueeze(0)     # (uid_stride = K + 1)
        i["uid"] = torch.where(ii % 2 == 0, (ii % n_dict).expand(N, K + 1), (ii + kk) % n_dict).to(torch.int32).contiguous()
    theta64 = None
    if case["outform"] == "theta":
        i["theta"] = torch.softmax(r(K, D), 0)
        theta64 = i["theta"]
    elif case["outform"] == "alphas":
        i["alphas"] = r(D)
        theta64 = GC.theta_ref(i["alphas"], K)
    ref = GC.fwd_reference(c, K, case["mode"], i["x"], t0=i.get("t0"), tk=i.get("tk"), xbias=i.get("xbias"), dis=i.get("dis"),
                           periph=i.get("periph"), ptab=i.get("ptab"), uid=i.get("uid"), eps=i.get("eps"), theta=theta64)
    ref["theta"] = theta64
    return i, ref


def _launch_fwd(c, D, case, i, force_subgroup, off=0, graph_ptr=None):
    """one kpgnn_aggregate_fwd launch on fresh device copies; returns the outputs on the CPU"""
    from kp_gnn_amd import _lib
    dev = _dev()
    N, K, Kc = c.N, case["K"], case["K_csr"]
    keep = []                                                   # device tensors the launch reads or writes

    def dv(t, o=0):
        keep.append(_place(t, dev, o) if t.dtype == torch.float32 else t.to(dev))
        return keep[-1]

    d = _lib.AggFwdDesc()
    d.N, d.K, d.D, d.K_csr, d.mode = N, K, D, Kc, case["mode"]
    d.rowptr, d.col, d.code = dv(c.rowptr).data_ptr(), dv(c.col).data_ptr(), dv(c.code).data_ptr()
    if case["xform"] == "stacked":
        x = dv(i["x"], off)
        d.x, d.x_sn, d.x_sk = x.data_ptr(), K * D, D
    elif case["xform"] == "strided":                            # hops 1 .. K of a [N, K + 3, D] history buffer
        hist = torch.zeros(N, K + 3, D)
        hist[:, 1:1 + K] = i["x"]
        x = dv(hist, off)[:, 1:1 + K]
        d.x, d.x_sn, d.x_sk = x.data_ptr(), (K + 3) * D, D
    else:
        assert K <= 16
        d.x, d.x_sn = None, D
        for k in range(K):
            d.x_slot[k] = dv(i["x"][:, k].contiguous(), off).data_ptr()
    if case["tables"]:
        d.use_tables, d.n_code0, d.table0 = 1, N0, dv(i["t0"]).data_ptr()
        if K > 1:
            d.n_codek, d.tablek = i["tk"].shape[0], dv(i["tk"]).data_ptr()
    if "dis" in i:
        d.dis = dv(i["dis"]).data_ptr()
    if "eps" in i:
        d.eps = dv(torch.tensor([i["eps"]])).data_ptr()
    if "xbias" in i:
        d.xbias = dv(i["xbias"]).data_ptr()
    if "periph" in i:
        d.periph, d.p_sn, d.p_sk = dv(i["periph"]).data_ptr(), K * D, D
    if "ptab" in i:
        d.ptab, d.uid, d.uid_stride, d.n_dict = dv(i["ptab"]).data_ptr(), dv(i["uid"]).data_ptr(), K + 1, i["ptab"].shape[0]
    out = hout = pre = theta = None
    if case["outform"] == "out":
        out = _nan(dev, N, K, D)
        d.out, d.o_sn, d.o_sk = out.data_ptr(), K * D, D
    else:
        hout = _nan(dev, N, D)
        d.hout = hout.data_ptr()
        if case["outform"] == "alphas":
            theta = _nan(dev, K, D)
            d.alphas = dv(i["alphas"]).data_ptr()
        else:
            theta = dv(i["theta"])
        d.theta = theta.data_ptr()
    if case["pre"]:
        pre = _nan(dev, N, K, D)
        d.pre = pre.data_ptr()
    if force_subgroup:
        d.n_dyn = dv(torch.tensor([N], dtype=torch.int32)).data_ptr()
    if graph_ptr is not None:
        gp = torch.tensor(graph_ptr, dtype=torch.int32)
        d.graph_ptr, d.num_graphs = dv(gp).data_ptr(), len(graph_ptr) - 1
        d.max_graph_nodes = int((gp[1:] - gp[:-1]).max())
    _lib.launch("kpgnn_aggregate_fwd", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(out=out, hout=hout, pre=pre, theta=theta).items() if v is not None}


def _try(errors, label, fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError as e:
        errors.append(f"{label}: {e}")


def _within(got, ref, bound, name):
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (name, "beyond 2 n 2^-24 sum|addends| by", float((err - bound).max()))


def _check_fwd(errors, label, case, got, ref):
    T = TOL["aggregate"]
    for k, v in got.items():
        assert not bool(torch.isnan(v).any()), (label, k, "elements left unwritten")
    if "out" in got:
        _try(errors, label, _close, got["out"], ref["out"], "out", **T["out"])
        if case["mode"] == MODE_SUM and not case["tables"] and not case["P"] and not case["xbias"]:
            _try(errors, label, _within, got["out"], ref["out"], ref["sum_bound"], "out")
    if "hout" in got:
        _try(errors, label, _close, got["hout"], ref["hout"], "hout", **T["out"])
        _try(errors, label, _close, got["theta"], ref["theta"], "theta", **T["out"])
    if "pre" in got:
        _try(errors, label, _close, got["pre"], ref["S"], "S", **T["out"])


def _same_bits(errors, label, a, b, keys=None):
    for k in (keys or a.keys()):
        if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)):
            errors.append(f"{label}: {k} not bit-identical, max |diff| {float((a[k] - b[k]).abs().max()):.3e}")


def _fwd_cases(D, G):
    cases = [
        ("gin_plain", _fwd_case(MODE_GIN, G - 1)),
        ("gin_tabL_dense_xbias", _fwd_case(MODE_GIN, G, tables="lds", P="dense", xbias=True)),
        ("ginplus_fast_slots", _fwd_case(MODE_GINPLUS, min(G - 1, 8), tables="lds", P="dict", outform="theta", xbias=True,
                                         xform="slots", pre=True)),
        ("ginplus_alphas_dictbig", _fwd_case(MODE_GINPLUS, min(G, 16), tables="lds", P="dict_big", outform="alphas",
                                             xform="slots", pre=True)),
        ("ginplus_theta_dict_strided", _fwd_case(MODE_GINPLUS, G - 1, tables="lds", P="dict", outform="theta", xform="strided")),
        ("ginplus_K1_alphas", _fwd_case(MODE_GINPLUS, 1, tables="lds", P="dict", outform="alphas", xform="slots", pre=True)),
        ("sum_K1_of_3_strided", _fwd_case(MODE_SUM, 1, K_csr=3, xform="strided")),
        ("sum_plain", _fwd_case(MODE_SUM, G)),
        ("sum_dict_notab_theta", _fwd_case(MODE_SUM, min(G - 1, 8), P="dict", outform="theta", xform="slots")),
        ("gcn_plain", _fwd_case(MODE_GCN, G - 1)),
        ("gcn_tabL_dense_xbias", _fwd_case(MODE_GCN, G, tables="lds", P="dense", xbias=True)),
        ("gcn_tabL_theta", _fwd_case(MODE_GCN, 16 if G <= 16 else G - 1, tables="lds", outform="theta", xbias=True)),
    ]
    if D in (256, 104, 13):
        Kg = min(G - 1, 8)
        cases += [("gin_tabG_dense", _fwd_case(MODE_GIN, Kg, tables="global", P="dense", xbias=True)),
                  ("gcn_tabG", _fwd_case(MODE_GCN, Kg, tables="global")),
                  ("ginplus_tabG_dict_theta", _fwd_case(MODE_GINPLUS, Kg, tables="global", P="dict", outform="theta",
                                                        xform="slots", pre=True))]
    return cases


@pytest.mark.parametrize("D,off,vec,G", SHAPES, ids=SHAPE_IDS)
def test_subgroup_forward(D, off, vec, G):
    assert _row_shape(D, off) == (vec, G)
    errors, routes = [], _Routes()
    for n, (name, case) in enumerate(_fwd_cases(D, G)):
        c = _csr(GC.case_nodes(G), case["K_csr"], G, seed=n, nk=_nk(case["tables"], D))
        i, ref = _fwd_inputs(c, D, case, seed=D * 31 + n)
        got = _launch_fwd(c, D, case, i, force_subgroup=True, off=off)
        routes.expect(0, SUB, name)
        _check_fwd(errors, name, case, got, ref)
        if n == 2:                                              # (one case per kernel: two launches, identical bits)
            _same_bits(errors, name + " second launch", got, _launch_fwd(c, D, case, i, force_subgroup=True, off=off))
            routes.expect(0, SUB, name)
    assert not errors, "\n".join(errors)


# ------------------------------------------------------------------------------------------------------------ backward
def _bwd_case(mode, K, K_csr=None, tables=None, gxform="stacked", acc=False):
    mask = sum(1 << k for k in range(K) if k % 3 != 1) if acc else 0
    return dict(mode=mode, K=K, K_csr=K_csr or K, tables=tables, gxform=gxform, acc_mask=mask)


def _bwd_inputs(c, D, case, seed):
    N, K = c.N, case["K"]
    g = torch.Generator().manual_seed(177 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    i = dict(g=r(N, K, D), old=r(N, K, D))
    if case["mode"] == MODE_GIN:
        i["eps"] = 0.3
    if case["mode"] == MODE_GCN:
        i["dis"] = GC.degree_dis(c).float()
    nk = _nk(case["tables"], D)
    ref = GC.bwd_reference(c, K, case["mode"], i["g"], dis=i.get("dis"), eps=i.get("eps"), old=i["old"],
                           acc_mask=case["acc_mask"], n_code0=N0 if case["tables"] else 0, n_codek=nk)
    return i, ref


def _launch_bwd(c, D, case, i, force_subgroup, off=0):
    from kp_gnn_amd import _lib
    dev = _dev()
    N, K, Kc = c.N, case["K"], case["K_csr"]
    keep = []

    def dv(t, o=0):
        keep.append(_place(t, dev, o) if t.dtype == torch.float32 else t.to(dev))
        return keep[-1]

    d = _lib.AggBwdDesc()
    d.N, d.K, d.D, d.K_csr, d.mode = N, K, D, Kc, case["mode"]
    d.rowptr_src, d.col_src, d.code_src = dv(c.rowptr).data_ptr(), dv(c.col).data_ptr(), dv(c.code).data_ptr()
    d.g, d.g_sn, d.g_sk = dv(i["g"], off).data_ptr(), K * D, D
    if "dis" in i:
        d.dis = dv(i["dis"]).data_ptr()
    if "eps" in i:
        d.eps = dv(torch.tensor([i["eps"]])).data_ptr()
    mask = case["acc_mask"]
    start = torch.full((N, K, D), float("nan"))                 # accumulating hops start from `old`, the others from NaN
    for k in range(K):
        if (mask >> k) & 1:
            start[:, k] = i["old"][:, k]
    if case["gxform"] == "stacked":
        gx = dv(start)
        d.gx, d.gx_sn, d.gx_sk = gx.data_ptr(), K * D, D
        slots = None
    else:
        assert K <= 16
        slots = [dv(start[:, k].contiguous()) for k in range(K)]
        d.gx, d.gx_sn = None, D
        for k in range(K):
            d.gx_slot[k] = slots[k].data_ptr()
    d.accumulate_mask = mask
    gt0 = gtk = None
    if case["tables"]:
        nk = _nk(case["tables"], D)
        gt0 = torch.zeros(N0, D, dtype=torch.float32, device=dev)
        d.use_tables, d.n_code0, d.gtable0 = 1, N0, gt0.data_ptr()
        if K > 1:
            gtk = torch.zeros(nk, D, dtype=torch.float32, device=dev)
            d.n_codek, d.gtablek = nk, gtk.data_ptr()
    if force_subgroup:
        d.n_dyn = dv(torch.tensor([N], dtype=torch.int32)).data_ptr()
    _lib.launch("kpgnn_aggregate_bwd", dev, ctypes.byref(d))
    torch.cuda.synchronize()
    res = dict(gx=(gx if slots is None else torch.stack(slots, 1)).cpu())
    if gt0 is not None:
        res["gtable0"] = gt0.cpu()
    if gtk is not None:
        res["gtablek"] = gtk.cpu()
    return res


def _check_bwd(errors, label, case, got, ref):
    T = TOL["aggregate"]
    assert not bool(torch.isnan(got["gx"]).any()), (label, "gx elements left unwritten")
    _try(errors, label, _close, got["gx"], ref["gx"], "gx", **T["grad_x"])
    if case["mode"] == MODE_SUM and not case["tables"] and not case["acc_mask"]:
        _try(errors, label, _within, got["gx"], ref["gx"], ref["sum_bound"], "gx")
    for k in ("gtable0", "gtablek"):
        if k in got:
            _try(errors, label, _close, got[k], ref[k], k, **T["grad_" + k[1:]])


def _bwd_cases(D, G):
    cases = [
        ("sum_chunked", _bwd_case(MODE_SUM, G - 1)),
        ("gin_chunked_slots", _bwd_case(MODE_GIN, min(G - 1, 16), gxform="slots")),
        ("ginplus_slots_acc", _bwd_case(MODE_GINPLUS, min(G, 16), gxform="slots", acc=True)),
        ("gin_stacked_gxacc", _bwd_case(MODE_GIN, min(G, 32), acc=True)),
        ("gin_tabL", _bwd_case(MODE_GIN, G - 1, tables="lds")),
        ("sum_tabL_slots_acc", _bwd_case(MODE_SUM, min(G, 16), tables="lds", gxform="slots", acc=True)),
        ("gcn_plain", _bwd_case(MODE_GCN, G - 1)),
        ("gcn_tabL", _bwd_case(MODE_GCN, G, tables="lds")),
        ("sum_K1_of_3", _bwd_case(MODE_SUM, 1, K_csr=3)),
    ]
    if D in (256, 104, 13):
        Kg = min(G - 1, 8)
        cases += [("gin_tabG", _bwd_case(MODE_GIN, Kg, tables="global")), ("gcn_tabG", _bwd_case(MODE_GCN, Kg, tables="global"))]
    return cases


@pytest.mark.parametrize("D,off,vec,G", SHAPES, ids=SHAPE_IDS)
def test_subgroup_backward(D, off, vec, G):
    assert _row_shape(D, off) == (vec, G)
    errors, routes = [], _Routes()
    for n, (name, case) in enumerate(_bwd_cases(D, G)):
        c = _csr(GC.case_nodes(G), case["K_csr"], G, seed=100 + n, nk=_nk(case["tables"], D))
        i, ref = _bwd_inputs(c, D, case, seed=D * 37 + n)
        got = _launch_bwd(c, D, case, i, force_subgroup=True, off=off)
        routes.expect(1, SUB, name)
        _check_bwd(errors, name, case, got, ref)
        if n in (2, 4):                                         # two launches: identical bits (table-gradient atomics excepted)
            _same_bits(errors, name + " second launch", got, _launch_bwd(c, D, case, i, force_subgroup=True, off=off), ["gx"])
            routes.expect(1, SUB, name)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("tiles", [1, 7, 8, 9])
def test_tile_counts(tiles):
    """D = 16 (G = 4, 64 nodes per tile): 1, 7, 8 and 9 tiles, the last one ragged - the grid is rounded down to a multiple of 8
    (pick_grid), so 9 tiles are walked by 8 blocks and 7 by 7."""
    D, G = 16, 4
    N = tiles * 64 - 23
    assert N >= GC.MIN_NODES and (N + 63) // 64 == tiles and N % 64
    errors, routes = [], _Routes()
    fc = _fwd_case(MODE_GIN, 3, tables="lds", P="dict", xbias=True)
    c = _csr(N, 3, G, seed=200 + tiles)
    i, ref = _fwd_inputs(c, D, fc, seed=tiles)
    got = _launch_fwd(c, D, fc, i, force_subgroup=True)
    routes.expect(0, SUB, "fwd")
    _check_fwd(errors, "fwd", fc, got, ref)
    for name, bc in (("bwd chunked", _bwd_case(MODE_GIN, 3, gxform="slots", acc=True)), ("bwd tables", _bwd_case(MODE_GCN, 3, tables="lds"))):
        i, ref = _bwd_inputs(c, D, bc, seed=tiles)
        got = _launch_bwd(c, D, bc, i, force_subgroup=True)
        routes.expect(1, SUB, name)
        _check_bwd(errors, name, bc, got, ref)
    assert not errors, "\n".join(errors)


# ------------------------------------------------------------------------------------------------------------ the other kernels
# Pairs of (kernel, output) whose bits the kernels' headers do not promise to be those of the sub-group kernel: the sums are
# the same, in another order (measured: 1 to 4 ulp apart).  They are held to float64 like everything else, and not bit for bit.
#   small forward, hout at K > 1: theta * v is rounded before the hop sum there and fused into it by the sub-group kernel
#     (aggregate_small.hip header); S, theta and hout at K = 1 are bit-identical.
#   narrow / small backward with a self term (GIN) or accumulate_mask: the sub-group kernel's chunked loop adds the self term
#     and the old value behind a hop's first PF pairs, where they arrive, and the remaining pairs after them; the narrow and
#     the small kernel add them after the last pair.
SAME_SUMS_ONLY = {("small_fwd", "hout"), ("narrow_bwd", "self_or_acc"), ("small_bwd", "acc")}


def _two_routes_fwd(errors, routes, label, c, D, case, seed, route, graph_ptr=None, bit_keys=None):
    """the case on its own kernel (twice: identical bits) and on the sub-group kernel (n_dyn = N): float64 for both, then bits"""
    i, ref = _fwd_inputs(c, D, case, seed)
    own = _launch_fwd(c, D, case, i, force_subgroup=False, graph_ptr=graph_ptr)
    routes.expect(0, route, label)
    again = _launch_fwd(c, D, case, i, force_subgroup=False, graph_ptr=graph_ptr)
    routes.expect(0, route, label)
    sub = _launch_fwd(c, D, case, i, force_subgroup=True)
    routes.expect(0, SUB, label)
    _check_fwd(errors, label, case, own, ref)
    _check_fwd(errors, label + " (sub-group)", case, sub, ref)
    _same_bits(errors, label + " second launch", own, again)
    _same_bits(errors, label + " vs sub-group", own, sub, bit_keys)


def _two_routes_bwd(errors, routes, label, c, D, case, seed, route, bits=True):
    i, ref = _bwd_inputs(c, D, case, seed)
    own = _launch_bwd(c, D, case, i, force_subgroup=False)
    routes.expect(1, route, label)
    again = _launch_bwd(c, D, case, i, force_subgroup=False)
    routes.expect(1, route, label)
    sub = _launch_bwd(c, D, case, i, force_subgroup=True)
    routes.expect(1, SUB, label)
    _check_bwd(errors, label, case, own, ref)
    _check_bwd(errors, label + " (sub-group)", case, sub, ref)
    _same_bits(errors, label + " second launch", own, again, ["gx"])
    if bits:
        _same_bits(errors, label + " vs sub-group", own, sub, ["gx"])


@pytest.mark.parametrize("D", [1, 6, 13, 32])
def test_narrow_forward(D):
    G = _row_shape(D, 0)[1]
    errors, routes = [], _Routes()
    cases = [("gin_tab_dense_xbias", _fwd_case(MODE_GIN, 5, tables="lds", P="dense", xbias=True)),
             ("ginplus_tab_dict_pre", _fwd_case(MODE_GINPLUS, G, tables="lds", P="dict", xbias=True, pre=True)),
             ("gin_plain", _fwd_case(MODE_GIN, G - 1)),
             ("sum_K1_of_3_strided", _fwd_case(MODE_SUM, 1, K_csr=3, xform="strided"))]
    for n, (name, case) in enumerate(cases):
        c = _csr(GC.case_nodes(G), case["K_csr"], G, seed=300 + n)
        _two_routes_fwd(errors, routes, name, c, D, case, D * 41 + n, NARROW)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("D", [1, 6, 13, 32])
def test_narrow_backward(D):
    G = _row_shape(D, 0)[1]
    errors, routes = [], _Routes()
    cases = [("sum_plain", _bwd_case(MODE_SUM, G - 1), True),
             ("ginplus_K1_of_3", _bwd_case(MODE_GINPLUS, 1, K_csr=3), True),
             ("gin_self_term", _bwd_case(MODE_GIN, 5), ("narrow_bwd", "self_or_acc") not in SAME_SUMS_ONLY),
             ("sum_acc_mask", _bwd_case(MODE_SUM, G, acc=True), ("narrow_bwd", "self_or_acc") not in SAME_SUMS_ONLY)]
    for n, (name, case, bits) in enumerate(cases):
        c = _csr(GC.case_nodes(G), case["K_csr"], G, seed=320 + n)
        _two_routes_bwd(errors, routes, name, c, D, case, D * 43 + n, NARROW, bits)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("D", [4, 104, 128])
def test_small_forward(D, K):
    """N = 41 <= 4096; the pair lists are built for the 32-pair chunk of the small kernel's units (and of G = 32)"""
    errors, routes = [], _Routes()
    keys = None if K == 1 or ("small_fwd", "hout") not in SAME_SUMS_ONLY else ["pre", "theta"]
    for n, outform in enumerate(("theta", "alphas")):
        case = _fwd_case(MODE_GINPLUS, K, tables="lds", P="dict", outform=outform, xbias=bool(n), xform="slots", pre=True)
        c = _csr(GC.case_nodes(32), K, 32, seed=340 + n)
        _two_routes_fwd(errors, routes, outform, c, D, case, D * 47 + K + n, SMALL, bit_keys=keys)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("D", [4, 104, 128])
def test_small_backward(D, K):
    errors, routes = [], _Routes()
    cases = [("sum_slots", _bwd_case(MODE_SUM, K, gxform="slots"), True),
             ("ginplus_slots_acc", _bwd_case(MODE_GINPLUS, K, gxform="slots", acc=True), ("small_bwd", "acc") not in SAME_SUMS_ONLY)]
    for n, (name, case, bits) in enumerate(cases):
        c = _csr(GC.case_nodes(32), K, 32, seed=360 + n)
        _two_routes_bwd(errors, routes, name, c, D, case, D * 53 + K + n, SMALL, bits)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("mode", [MODE_GIN, MODE_SUM], ids=["gin", "sum"])
@pytest.mark.parametrize("D", [4, 16, 64])
def test_lds_forward(D, mode):
    """graphs of 1, 3, 9 and N - 13 nodes; pairs drawn inside each graph; the pair lists are built for the 2 * D / 4 pairs the
    kernel fetches per trip"""
    G = max(4, 2 * (D // 4))
    N = GC.case_nodes(G)
    gp = (0, 1, 4, 13, N)
    errors, routes = [], _Routes()
    c = _csr(N, 3, G, seed=380, graph_ptr=gp)
    _two_routes_fwd(errors, routes, "lds", c, D, _fwd_case(mode, 3), D * 59 + mode, LDS, graph_ptr=gp)
    assert not errors, "\n".join(errors)
