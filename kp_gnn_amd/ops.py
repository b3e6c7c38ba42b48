"""Autograd operators over the C ABI (include/kpgnn.h).  Host-side plumbing only: tensors in, pointers
and strides out; every arithmetic step of the K-hop aggregation runs in the HIP kernels."""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import MODE_GCN, MODE_GIN, MODE_GINPLUS, MODE_SUM, LaunchTimer, set_launch_timer  # noqa: F401
from .ops_dataset import (COUNT_LABELS_AUTO, GRAPH_LABELS_AUTO, PROPERTY_GRAPHS_AUTO, PropertyGraphs, RegularGraphs,  # noqa: F401
                          count_labels, count_labels_launch, graph_labels_launch, graph_property_labels, khop_transform,
                          property_graphs, random_regular_graphs, resistance_distance)

_SQRT1_2 = 0.7071067811865476
_INV_SQRT_2PI = 0.3989422804014327


def algorithmic_bytes(csr, k_act, D, n_tensors, n_rows_tables, extra_nd=0, s=4):
    """s*N*k*D per streamed [N,k,D] tensor + (4+2) B per active pair + int32 row pointers
    + the tables once (+ 4*N*D per fp32 [N,D] tensor), s = 4 (fp32) or 2 (bf16 storage).  n_tensors may be fractional
    when the streams of one launch have different widths (it counts fp32-equivalents at s = 4)."""
    A = csr.active_pairs(k_act)
    return int(s * csr.N * k_act * D * n_tensors) + A * 6 + 4 * (csr.N * csr.K + 1) + 4 * D * n_rows_tables \
        + 4 * csr.N * D * extra_nd


# Storage of the big per-(node,hop) streams of the fused KP-GIN+ path (hop-slot rows, S saved for the backward, dL/dS):
# torch.float32 (default) or torch.bfloat16 (kpgnn.h KPGNN_STORE_BF16: 2-byte rows, fp32 sums).  Other paths ignore it.
_STORAGE = torch.float32


def set_storage_dtype(dtype):
    """torch.float32 / torch.bfloat16 (or "fp32" / "bf16"): see _STORAGE.  Returns the previous setting."""
    global _STORAGE
    prev = _STORAGE
    dtype = {"fp32": torch.float32, "f32": torch.float32, "bf16": torch.bfloat16}.get(dtype, dtype)
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"storage dtype must be float32 or bfloat16, got {dtype}")
    _STORAGE = dtype
    return prev


def bf16_shadow(t):
    """bf16 copy of a hop state [N,D] for the gathers of later layers (made once per state, kept on the tensor)."""
    rec = getattr(t, "_kp_bf16", None)
    if rec is None or rec[0] != t._version:      # (a state modified in place after its first reader gets a fresh shadow)
        rec = (t._version, t.detach().to(torch.bfloat16).contiguous())
        try:
            t._kp_bf16 = rec
        except AttributeError:
            pass
    return rec[1]


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------ dynamic row count (static-shape graphs)
# A hipGraph bakes every kernel argument in, the row count N of a batch included, and no two shuffled batches have the same
# N.  Under `dynamic_rows(count, capacity)` every launch that works on `capacity` rows is handed `count` (a device int32[1],
# e.g. the node count kpgnn_collate leaves in its header) as its descriptor's n_dyn: tensors are allocated for the capacity,
# kernels read, write and SUM only the live rows - so ONE captured graph serves every batch up to the capacity
# (dataset.StaticBatch, bench.py --fresh-batches).  Operators without an n_dyn field refuse to run in this mode.
_DYN = None     # (count tensor, capacity)


class dynamic_rows:
    def __init__(self, count, capacity):
        assert count.dtype == torch.int32 and count.numel() >= 1 and count.is_cuda
        self._new = (count, int(capacity))

    def __enter__(self):
        global _DYN
        self._old, _DYN = _DYN, self._new
        return self

    def __exit__(self, *exc):
        global _DYN
        _DYN = self._old
        return False


def dyn_ptr(rows):
    """n_dyn for a launch over `rows` rows: the live-count pointer when `rows` is the capacity of the active dynamic_rows
    block, else None (launches over other row counts - graphs, dictionary rows - are static)."""
    if _DYN is not None and int(rows) == _DYN[1]:
        return _DYN[0].data_ptr()
    return None


def refuse_dynamic_rows(what, rows):
    if _DYN is not None and int(rows) == _DYN[1]:
        raise _lib.KpgnnError(f"{what} has no dynamic row count (n_dyn): run this configuration on exact-shape batches")


def _last_contig(t):
    """[N,K,D] view with unit innermost stride (copy only if the caller handed something exotic)."""
    return t if t.stride(-1) == 1 else t.contiguous()


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.KpgnnError("kp_gnn_amd ops need CUDA/HIP tensors: there is no CPU fallback "
                                  "(the CPU restatement lives in oracle/ and is test-only)")


def _check_codes(csr, k_act, table0, tablek):
    if csr.A == 0:
        return
    if csr.max_code0 >= table0.shape[0]:
        raise IndexError(f"edge code {csr.max_code0} out of range for hop1_edge_emb with {table0.shape[0]} rows")
    if k_act > 1 and tablek is not None and csr.max_codek >= tablek.shape[0]:
        raise IndexError(f"edge code {csr.max_codek} out of range for hopk_edge_emb with {tablek.shape[0]} rows")


# ------------------------------------------------------------------------------------ deferred reductions
# A weight-gradient launch leaves per-block partial sums that a small second launch adds up.  Inside
# `deferred_reductions()` that second launch is not issued: the job (kpgnn_reduce_job) waits in this list and the next
# table-gradient call - which has a finishing launch of its own - takes it along (8 launches less per step at L = 8); what
# is left when the block ends is run then.  The gradient tensors such a backward returns are NOT valid until the block
# ends: only for callers that read gradients afterwards (torch.autograd.grad(...) inside the block, or .backward() into
# parameters whose .grad is None) - never with gradient accumulation into existing .grad tensors or backward hooks.
#
# The weight gradients of the fused MLPs go one step further: nothing reads them before the pass ends, so inside the block
# their PRODUCTS are not launched either.  Each MLP parks its pair of problems here, and up to WGRAD_MANY_PAIRS of one shape
# run as ONE kpgnn_linear_wgrad_many launch (per pair the sums of a launch of its own, bit for bit) followed by their
# reductions.  A parked pair keeps its operands alive until then (dy2, dy1, y1, h: 4 [N,h] tensors per layer).
_pending_reduce = None        # None: off; list of (ReduceJob, tensors kept alive)
_parked_wgrad = []            # (shape key, WgradDesc a, WgradDesc b, parameter keys, tensors kept alive), oldest first
WGRAD_MANY_PAIRS = 8          # csrc/wgrad.hip kW2MaxProb / 2


class deferred_reductions:
    def __enter__(self):
        global _pending_reduce
        self._outer = _pending_reduce
        if _pending_reduce is None:
            _pending_reduce = []
        return self

    def __exit__(self, *exc):
        global _pending_reduce
        if self._outer is None:
            if exc[0] is None:
                flush_parked_wgrad()
            del _parked_wgrad[:]
            jobs, _pending_reduce = _pending_reduce, None
            _deferred_owners.clear()
            if jobs and exc[0] is None:
                flush_reductions(jobs)
        return False


def flush_reductions(jobs):
    arr = (_lib.ReduceJob * len(jobs))(*[j for j, _ in jobs])
    _lib.launch("kpgnn_reduce_jobs", jobs[0][1][0].device, arr, len(jobs))


_deferred_owners = set()      # data_ptr of the parameters whose gradient a queued job will write


def defer_reduce_job(*params):
    """A fresh job slot when reductions are being deferred (the caller hands ctypes.byref(job) to a launch with a `defer`
    field, then calls queue_reduce_job), else None.
    `params`: the parameters whose gradients the job will write.  A parameter that feeds TWO nodes (shared MLP weights, a
    layer applied twice) has its two gradients summed by autograd as soon as both nodes have returned - before the block
    ends - so a second job for a parameter that already has one is refused (None: the caller reduces at once) and everything
    queued so far is run first: the sum then only ever reads finished gradients."""
    if _pending_reduce is None:
        return None
    keys = {p.data_ptr() for p in params if p is not None}
    if keys & _deferred_owners:
        flush_parked_wgrad()          # (the parked products first: their reductions must not run after the sum either)
        jobs = list(_pending_reduce)
        del _pending_reduce[:]
        _deferred_owners.clear()
        if jobs:
            flush_reductions(jobs)
        return None
    _deferred_owners.update(keys)
    return _lib.ReduceJob()


def park_wgrad_pair(a, b, params, keep_alive):
    """Inside deferred_reductions(): take the two weight-gradient problems of a fused MLP (filled kpgnn_wgrad_desc a, b with
    O == I, a.workspace set) instead of launching them - True - where the bf16-split kernel would run them.  False: the caller
    launches as usual.  `params` as in defer_reduce_job; keep_alive[0] is a tensor on the launch's device."""
    if _pending_reduce is None or a.math == _lib.MATH_F32 or a.O != a.I or a.O > 128 or a.O % 4:
        return False
    keys = {p.data_ptr() for p in params}
    if keys & _deferred_owners:       # a shared weight: defer_reduce_job runs what is parked and queued, the caller reduces at once
        return False
    shape = (a.N, a.O, a.I, a.n_dyn, keep_alive[0].device)
    if _parked_wgrad and _parked_wgrad[0][0] != shape:
        flush_parked_wgrad()
    _deferred_owners.update(keys)
    _parked_wgrad.append((shape, a, b, keys, keep_alive))
    if len(_parked_wgrad) == WGRAD_MANY_PAIRS:
        flush_parked_wgrad()
    return True


def flush_parked_wgrad():
    """Run the parked weight-gradient products in one launch, then their reductions."""
    parked = list(_parked_wgrad)
    del _parked_wgrad[:]
    if not parked:
        return
    dev = parked[0][0][-1]
    jobs = []
    for _, a, _, keys, keep_alive in parked:
        job = _lib.ReduceJob()
        a.defer = ctypes.cast(ctypes.pointer(job), ctypes.c_void_p)
        jobs.append((job, keep_alive))
        _deferred_owners.difference_update(keys)
    if len(parked) == 1:
        _lib.launch("kpgnn_linear_wgrad_pair", dev, ctypes.byref(parked[0][1]), ctypes.byref(parked[0][2]))
    else:
        ptrs = ctypes.POINTER(_lib.WgradDesc) * len(parked)
        _lib.launch("kpgnn_linear_wgrad_many", dev, ptrs(*[ctypes.pointer(e[1]) for e in parked]),
                    ptrs(*[ctypes.pointer(e[2]) for e in parked]), len(parked))
    flush_reductions(jobs)


def queue_reduce_job(job, keep_alive):
    _pending_reduce.append((job, keep_alive))


def take_reduce_job():
    """The oldest waiting job, or None: for a call whose finishing launch can take one along."""
    if _pending_reduce:
        return _pending_reduce.pop(0)
    return None


class DictPeripheral:
    """Dictionary form of the peripheral features: P[i,k,:] = table[uid[i,k], :].

    The (node,hop) peripheral-subgraph feature tuples repeat massively (25 distinct among 379,600 slots of a
    2048-molecule batch), so instead of a dense [N,K,D] tensor the callers may hand the layers this object
    as `peripheral_attr`: `table` [U,D] carries the gradient, `uid` [N,K] (int32) is static per batch.
    Supports the body's `peripheral_attr[:, :k]` hop-prefix slicing (models/GNNs.py:421-423)."""

    def __init__(self, table, uid):
        self.table, self.uid = table, uid

    @property
    def shape(self):
        return (self.uid.shape[0], self.uid.shape[1], self.table.shape[1])

    def __getitem__(self, idx):
        if (isinstance(idx, tuple) and len(idx) == 2 and idx[0] == slice(None) and isinstance(idx[1], slice)
                and idx[1].start in (None, 0) and idx[1].step in (None, 1)):
            v = self.uid[:, idx[1]]
            dom = getattr(self.uid, "_kp_dom", None)
            if dom is not None:                      # (per-hop hint for the dictionary gradient: follows the hop prefix)
                v._kp_dom = dom[idx[1]]
            return DictPeripheral(self.table, v)
        return self.dense()[idx]

    def dense(self):
        """Materialised [N,K,D] tensor (differentiable): for callers outside the fused kernels."""
        return DictRows.apply(self.table, self.uid)


def aggregate_fwd_raw(csr, k_act, mode, x, table0, tablek, periph, eps, theta, xbias, want_pre, ptab=None, uid=None,
                      xs=None, alphas=None, bf16=False):
    """Launch kpgnn_aggregate_fwd.  x is [N,k,D], or None with xs = k per-hop [N,D] tensors (row stride shared).
    bf16: xs are bf16 rows and `pre` is returned as bf16 (KPGNN_STORE_BF16).
    Returns (out or hout, pre or None)."""
    if x is not None:
        N, K, D = x.shape
    else:
        N, D = xs[0].shape
        K = len(xs)
    assert K == k_act and N == csr.N
    dev = (x if x is not None else xs[0]).device
    d = _lib.AggFwdDesc()
    d.N, d.K, d.D, d.K_csr, d.mode = N, K, D, csr.K, mode
    d.n_dyn = dyn_ptr(N)
    use_tables = table0 is not None
    d.use_tables = 1 if use_tables else 0
    d.n_code0 = table0.shape[0] if use_tables else 0
    d.n_codek = tablek.shape[0] if (use_tables and tablek is not None) else 0
    d.rowptr, d.col, d.code = csr.rowptr_dst.data_ptr(), csr.col_dst.data_ptr(), csr.code_dst.data_ptr()
    d.dis = csr.gcn_dis().data_ptr() if mode == MODE_GCN else None
    if x is not None:
        d.x, d.x_sn, d.x_sk = x.data_ptr(), x.stride(0), x.stride(1)
    else:
        d.x_sn = xs[0].stride(0)
        for k, t in enumerate(xs):
            assert t.shape == (N, D) and t.stride(1) == 1 and t.stride(0) == d.x_sn
            d.x_slot[k] = t.data_ptr()
    d.table0, d.tablek = _ptr(table0), _ptr(tablek)
    if periph is not None:
        d.periph, d.p_sn, d.p_sk = periph.data_ptr(), periph.stride(0), periph.stride(1)
    elif uid is not None:
        d.ptab, d.uid, d.uid_stride = ptab.data_ptr(), uid.data_ptr(), uid.stride(0)
        d.n_dict = ptab.shape[0]
    d.eps = _ptr(eps)
    d.xbias = _ptr(xbias)
    # dense K-hop neighbourhoods (>= 12 pairs per (node, hop) on average) of a batch whose graph boundaries are known: the
    # library may gather from an LDS-staged hop slab (mask-only aggregations; it checks the shape itself)
    gp = getattr(csr, "graph_ptr", None)
    if gp is not None and x is not None and not use_tables and csr.A >= 12 * max(csr.N * csr.K, 1) and d.n_dyn is None:
        d.graph_ptr, d.num_graphs, d.max_graph_nodes = gp.data_ptr(), gp.numel() - 1, csr.max_graph_nodes
    pre = torch.empty((N, K, D), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev) if want_pre else None
    d.pre = _ptr(pre)
    d.storage = 1 if bf16 else 0
    if theta is not None:
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
        d.theta, d.hout = theta.data_ptr(), out.data_ptr()
        d.alphas = _ptr(alphas)     # geometric combine: the launch fills `theta` itself
    else:
        out = torch.empty((N, K, D), dtype=torch.float32, device=dev)
        d.out, d.o_sn, d.o_sk = out.data_ptr(), out.stride(0), out.stride(1)

    def nbytes():
        n_t = 1 + (periph is not None) + (pre is not None) + (theta is None)  # x, dense P, pre, out
        extra = 4 * N * K if uid is not None else 0                           # int32 uid per (node,hop)
        return extra + algorithmic_bytes(csr, K, D, n_t, d.n_code0 + d.n_codek, extra_nd=1 if theta is not None else 0,
                                         s=2 if bf16 else 4)
    _lib.launch("kpgnn_aggregate_fwd", dev, ctypes.byref(d), timed=("agg_fwd", nbytes))
    return out, pre


PULL_GATHER = True      # (tests switch it off to compare with the read-modify-write form of the backward gather)


def pull_applies(N, D, dtype=torch.float32):
    """Whether KHopAggregate.backward takes the pull form for a [N, k, D] gradient of this dtype (the KP-GIN+ history pattern
    is the caller's business): producers of other shares of a state's gradient use it to decide how to hand theirs over."""
    return PULL_GATHER and dtype == torch.float32 and N >= 4096 and D % 4 == 0


def khop_pull_gather(csr, slabs, hinit, hinit2=None):
    """A state's whole K-hop gradient in ONE launch (kpgnn_khop_pull_gather over the (source, hop)-keyed CSR):
    out[i] = hinit[i] + sum_k sum_{j in N_k(i)} slabs[k][j], where slabs[k] is hop k's [N,D] slab of dL/dS of the
    layer that read the state at hop slot k.  Replaces one read-modify-write of the state's gradient per reader (36 per step
    at K = L = 8: agg_bwd moved 273 MB per launch for 183 MB of gathered rows) by one write per state."""
    K = len(slabs)
    N, D = slabs[0].shape
    dev = slabs[0].device
    out = hinit if hinit is not None else torch.empty((N, D), dtype=torch.float32, device=dev)
    d = _lib.PullGatherDesc()
    d.N, d.K, d.D, d.K_csr = N, K, D, csr.K
    d.n_dyn = dyn_ptr(N)
    d.rowptr, d.col = csr.rowptr_src.data_ptr(), csr.col_src.data_ptr()
    d.slab_sn = D
    for k, t in enumerate(slabs):
        assert t.shape == (N, D) and t.is_contiguous() and t.dtype == torch.float32
        d.slab[k] = t.data_ptr()
    d.hout, d.hinit, d.hinit2 = out.data_ptr(), _ptr(hinit), _ptr(hinit2)
    _lib.launch("kpgnn_khop_pull_gather", dev, ctypes.byref(d), timed=("agg_bwd", lambda: algorithmic_bytes(
        csr, K, D, 1, 0, extra_nd=1 + (hinit is not None) + (hinit2 is not None))))
    return out


def aggregate_bwd_raw(csr, k_act, mode, g, eps, n_code0, n_codek, want_tables, slots=False, slot_bufs=None, gx_accum=None):
    """Launch kpgnn_aggregate_bwd on g = dL/dS.  Returns (gx, gtable0, gtablek); with slots=True gx is a list of
    k contiguous [N,D] tensors (one per hop slot) instead of one [N,k,D] tensor; slot_bufs[k] (a [N,D] tensor or None)
    makes the kernel ADD slot k's gradient into that buffer instead of writing a fresh one."""
    N, K, D = g.shape
    dev = g.device
    bf16 = g.dtype == torch.bfloat16      # KPGNN_STORE_BF16: g rows are bf16, gx stays fp32
    d = _lib.AggBwdDesc()
    d.N, d.K, d.D, d.K_csr, d.mode = N, K, D, csr.K, mode
    d.n_dyn = dyn_ptr(N)
    d.storage = 1 if bf16 else 0
    d.use_tables = 1 if want_tables else 0
    d.n_code0, d.n_codek = n_code0, n_codek
    d.rowptr_src, d.col_src, d.code_src = csr.rowptr_src.data_ptr(), csr.col_src.data_ptr(), csr.code_src.data_ptr()
    d.dis = csr.gcn_dis().data_ptr() if mode == MODE_GCN else None
    d.g, d.g_sn, d.g_sk = g.data_ptr(), g.stride(0), g.stride(1)
    d.eps = _ptr(eps)
    late_adds = []
    if slots:
        # The kernel writes every hop slot with ONE row stride.  Parked gradient buffers (slot_bufs) may be strided
        # views (slices of the jumping-knowledge gradient, body.py): when all K slots are parked with the same stride
        # the kernel accumulates into them where they are; otherwise parked buffers whose stride differs from the fresh
        # contiguous outputs are added afterwards by the framework (rare path).
        bufs = list(slot_bufs) if slot_bufs is not None else [None] * K
        strides = {b.stride(0) for b in bufs if b is not None}
        sn = D
        if len(strides) == 1 and all(b is not None for b in bufs):
            sn = strides.pop()
        gx, mask = [], 0
        for k in range(K):
            b = bufs[k]
            if b is not None and b.stride(0) == sn and b.stride(1) == 1:
                gx.append(b)
                mask |= 1 << k
            else:
                t = torch.empty((N, D), dtype=torch.float32, device=dev)
                gx.append(t)
                if b is not None:
                    late_adds.append((k, b))
            d.gx_slot[k] = gx[k].data_ptr()
        d.gx_sn = sn
        d.accumulate_mask = mask
    elif gx_accum is not None:     # the state's gradient cell ([N, K*D] contiguous): the kernel adds into it
        gx = gx_accum.view(N, K, D)
        d.gx, d.gx_sn, d.gx_sk = gx.data_ptr(), gx.stride(0), gx.stride(1)
        d.accumulate_mask = (1 << K) - 1
    else:
        gx = torch.empty((N, K, D), dtype=torch.float32, device=dev)
        d.gx, d.gx_sn, d.gx_sk = gx.data_ptr(), gx.stride(0), gx.stride(1)
    gt0 = gtk = None
    if want_tables:
        gt0 = torch.zeros((n_code0, D), dtype=torch.float32, device=dev)
        d.gtable0 = gt0.data_ptr()
        if K > 1 and n_codek > 0:
            gtk = torch.zeros((n_codek, D), dtype=torch.float32, device=dev)
            d.gtablek = gtk.data_ptr()
    # g read (2 or 4 bytes per element) + gx written (fp32)
    _lib.launch("kpgnn_aggregate_bwd", dev, ctypes.byref(d), timed=("agg_bwd", lambda: algorithmic_bytes(
        csr, K, D, 1.5 if bf16 else 2, (n_code0 + n_codek) if want_tables else 0)))
    for k, b in late_adds:
        gx[k] = b.add_(gx[k])
    return gx, gt0, gtk


def dict_tile_pack(csr, uid):
    """The (node, hop) dictionary entries of every tile of `csr`, sorted by dictionary row (kpgnn_dict_tile_pack): static
    per batch, built on first use and kept on the csr.  `uid` may be a hop-prefix view uid_full[:, :k]: the list is built
    over the full row (the kernel skips hops >= k).  Returns (pack, K_built) or (None, 0) when the shape has no pack."""
    kf = uid.stride(0) if uid.dim() == 2 and uid.shape[0] > 1 else uid.shape[1]
    if uid.stride(1) != 1 or kf > 8 or kf < uid.shape[1] or csr.nodes_per_tile * kf > 64:
        return None, 0
    cache = csr._dict_packs
    N = uid.shape[0]
    dyn = dyn_ptr(N)
    # (a StaticBatch refills `uid` in place: under dynamic_rows the list is rebuilt by every call - into the same buffer, so a
    #  captured graph refreshes it at every replay - and holds the live nodes' entries only: the walk takes every entry it finds.
    #  Such a list is kept under a key of its own: a launch over all N rows of the same csr and uid never walks it.)
    key = (uid.data_ptr(), kf, N, dyn)
    hit = cache.get(key)
    if hit is None or dyn is not None:
        tiles = (N + csr.nodes_per_tile - 1) // csr.nodes_per_tile
        pack = hit[0] if hit is not None else torch.empty((tiles, 64), dtype=torch.int32, device=uid.device)
        _lib.launch("kpgnn_dict_tile_pack_dyn", uid.device, uid.data_ptr(), kf, N, dyn, kf, csr.nodes_per_tile, pack.data_ptr())
        hit = cache[key] = (pack, kf, uid)     # (uid kept alive: the key is its address)
    return hit[0], hit[1]


def dict_grad_raw(uid, n_dict, theta, gh, defer=False):
    """Launch kpgnn_dict_grad: gdict[u] = sum_k theta[k] * sum_{i: uid[i,k]==u} gh[i].  uid [N,k] (may be a hop-prefix
    view), theta [k,D], gh [N,D].  Returns gdict [n_dict,D], or None when the shape does not fit the kernel.
    defer=True: returns (gdict, slab, nslab) with gdict still UNWRITTEN - the per-block partial sums wait in `slab` for a
    later finishing launch (table_grad_raw(extra=...) adds them up along with its own)."""
    lib = _lib.load()
    N, K = uid.shape
    D = gh.shape[1]
    ws_bytes = lib.kpgnn_dict_grad_workspace_bytes(N, K, D, n_dict)
    if ws_bytes == 0 or uid.stride(1) != 1:
        return None
    dev = gh.device
    dom = getattr(uid, "_kp_dom", None)          # [K] int32: the designated (most frequent) id per hop, if the caller has it
    has_dom = dom is not None and dom.numel() == K and dom.dtype == torch.int32 and dom.is_contiguous() and dom.device == dev
    if not has_dom and 4 * (n_dict * K * D + 2 * 64 * D) > 160 * 1024:
        return None        # (without the hint the kernel stages gh in LDS next to the accumulator rows: this dictionary does not fit)
    gh = gh.contiguous()
    theta = theta.contiguous()
    d = _lib.DictGradDesc()
    d.N, d.K, d.D, d.n_dict = N, K, D, n_dict
    d.n_dyn = dyn_ptr(N)
    d.uid, d.uid_stride, d.theta, d.gh = uid.data_ptr(), uid.stride(0), theta.data_ptr(), gh.data_ptr()
    if has_dom:
        d.dominant = dom.data_ptr()
    gd = torch.empty((n_dict, D), dtype=torch.float32, device=dev)
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    d.gdict, d.workspace, d.workspace_bytes = gd.data_ptr(), ws.data_ptr(), int(ws_bytes)
    d.defer_reduce = 1 if defer else 0
    _lib.launch("kpgnn_dict_grad", dev, ctypes.byref(d), timed=("dict_grad", lambda: 4 * N * D + 4 * N * K + 4 * D * (n_dict + K)))
    if defer:
        return gd, ws, int(lib.kpgnn_dict_grad_slabs(N))
    return gd


DICT_MULTI = True      # one dictionary-gradient launch per backward pass instead of one per layer (where the layers qualify)


def dict_multi_ok(uid, n_dict, theta, gh):
    """Whether a layer's dictionary share can wait for the one launch of dict_grad_multi_raw."""
    if not DICT_MULTI or uid is None or theta is None:
        return False
    N, K = uid.shape
    D = gh.shape[1]
    dom = getattr(uid, "_kp_dom", None)
    return (dom is not None and dom.numel() == K and dom.dtype == torch.int32 and dom.is_contiguous() and dom.device == gh.device
            and uid.stride(1) == 1 and uid.dtype == torch.int32 and K <= 8 and D % 2 == 0 and D <= 128 and gh.dtype == torch.float32
            and theta.dtype == torch.float32 and tuple(theta.shape) == (K, D) and 4 * (n_dict * 8 + 9) * D <= 160 * 1024)


def dict_grad_multi_raw(items, n_dict):
    """kpgnn_dict_grad_multi over the parked (uid view, theta, gh) of the layers that read one dictionary:
    gdict[u] = sum_l sum_k theta_l[k] * sum_{i: uid[i,k]==u} gh_l[i].  The uid views are hop prefixes of ONE id matrix."""
    lib = _lib.load()
    uid = max((it[0] for it in items), key=lambda u: u.shape[1])
    N, K = uid.shape
    D = items[0][2].shape[1]
    dev = items[0][2].device
    base = uid.data_ptr()
    one = all(it[0].data_ptr() == base and it[0].stride(0) == uid.stride(0) and it[0].shape[0] == N for it in items)
    if not one or len(items) > 16 or 4 * (n_dict * K + 9 * len(items)) * D > 160 * 1024:
        # (different id matrices, more layers than the kernel takes, or a table + per-layer totals beyond the LDS: one launch per layer)
        total = None
        for u, th, gh in items:
            g = dict_grad_raw(u, n_dict, th, gh)
            if g is None:
                raise _lib.KpgnnError("kpgnn_dict_grad refused a share that was parked for kpgnn_dict_grad_multi")
            total = g if total is None else total + g
        return total
    keep = []
    d = _lib.DictGradMultiDesc()
    d.N, d.D, d.n_dict, d.L = N, D, n_dict, len(items)
    d.uid, d.uid_stride = base, uid.stride(0)
    for l, (u, th, gh) in enumerate(items):
        th, gh = th.contiguous(), gh.contiguous()
        keep += [th, gh]
        d.theta[l], d.gh[l], d.K[l] = th.data_ptr(), gh.data_ptr(), u.shape[1]
    d.dominant = uid._kp_dom.data_ptr()
    d.n_dyn = dyn_ptr(N)
    ws_bytes = int(lib.kpgnn_dict_grad_workspace_bytes(N, K, D, n_dict))
    gd = torch.empty((n_dict, D), dtype=torch.float32, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    d.gdict, d.workspace, d.workspace_bytes = gd.data_ptr(), ws.data_ptr(), ws_bytes
    _lib.launch("kpgnn_dict_grad_multi", dev, ctypes.byref(d),
                timed=("dict_grad", lambda: len(items) * 4 * N * D + 4 * N * K + 4 * D * n_dict))
    return gd


def table_grad_raw(csr, g, n_code0, n_codek, edges=True, uid=None, n_dict=0, theta=None, gh=None, kernel=0, extra=None,
                   gdict_acc=None):
    """Launch kpgnn_table_grad on g = dL/dS [N,k,D]: edge-code table gradients (no per-edge atomics) and /
    or the peripheral-dictionary gradient (theta/gh given: sum theta[k]*gh[i]; else: sum of g rows).
    kernel: 0 automatic, 1 register walk, 2 count-matrix product (parity tests).
    Returns (gtable0, gtablek, gdict), or None when the shape fits neither kernel."""
    lib = _lib.load()
    g = g.contiguous()
    N, K, D = g.shape
    dev = g.device
    n0 = n_code0 if edges else 0
    nk = n_codek if (edges and K > 1) else 0
    ws_bytes = lib.kpgnn_table_grad_workspace_bytes(N, K, D, csr.nodes_per_tile, max(n0, 1) if edges else 0, nk, n_dict)
    if ws_bytes == 0:
        return None
    d = _lib.TableGradDesc()
    d.N, d.K, d.D, d.nodes_per_tile, d.n_code0, d.n_codek = N, K, D, csr.nodes_per_tile, n0, nk
    d.n_dyn = dyn_ptr(N)
    d.n_dict = n_dict
    d.dict_src = 0 if n_dict == 0 else (1 if theta is not None else 2)
    d.kernel = kernel
    d.storage = 1 if g.dtype == torch.bfloat16 else 0
    if edges:
        tptr, tpack = csr.tile_list(K)          # (hop-prefix copy of the entry list when this layer sees K < csr.K hops)
        d.tile_ptr, d.tile_pack = tptr.data_ptr(), tpack.data_ptr()
    d.g = g.data_ptr()
    d.g_sn, d.g_sk = K * D, D  # (contiguous; size-1 dims carry arbitrary strides)
    gt0 = gtk = gd = None
    if edges:
        gt0 = torch.empty((n0, D), dtype=torch.float32, device=dev)
        gtk = torch.empty((nk, D), dtype=torch.float32, device=dev) if nk > 0 else None
        d.gtable0, d.gtablek = gt0.data_ptr(), _ptr(gtk)
    if n_dict > 0:
        gd = torch.empty((n_dict, D), dtype=torch.float32, device=dev) if gdict_acc is None else gdict_acc
        d.uid, d.uid_stride, d.gdict = uid.data_ptr(), uid.stride(0), gd.data_ptr()
        if gdict_acc is not None:     # (a dictionary read by several layers: the gradient is added in place, see KHopAggregate)
            assert gdict_acc.is_contiguous() and gdict_acc.dtype == torch.float32 and tuple(gdict_acc.shape) == (n_dict, D)
            d.accumulate_dict = 1
        d.theta, d.gh = _ptr(theta), _ptr(gh)
        if K <= 8 and csr.nodes_per_tile * K <= 64:
            pack, kf = dict_tile_pack(csr, uid)
            d.dict_pack, d.dict_pack_K = _ptr(pack), kf
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), int(ws_bytes)
    if extra is not None:       # (out, slab, nslab) of dict_grad_raw(defer=True): added up by this call's finishing launch
        d.extra_out, d.extra_slab, d.extra_nslab, d.extra_elems = extra[0].data_ptr(), extra[1].data_ptr(), extra[2], extra[0].numel()
    _lib.launch("kpgnn_table_grad", dev, ctypes.byref(d), timed=("table_grad", lambda: (
        g.element_size() * N * K * D + (4 * csr.active_pairs(K) if edges else 0) + 4 * D * (n0 + nk + n_dict)
        + (4 * N * K if n_dict else 0))))
    return gt0, gtk, gd


def _combine_table_grad_ok(csr, pre, table_rows=0, dict_rows=0):
    """Shapes the fused combine + table-gradient kernel takes (kpgnn_table_grad with fuse_pre): fp32, K <= 8, even D <= 128,
    tiles of 8 nodes, and an LDS plan that fits - tile + (table rows + dictionary rows + 40 service rows) * D floats
    <= 160 KB (e.g. train_SR.py's max_pe_num = 1000 does not: those layers keep the separate kernels)."""
    N, K, D = pre.shape
    lds = 4 * (8 * K * D + (table_rows + 2 * dict_rows + 40) * D) + 64
    ok = (K <= 8 and D % 2 == 0 and D <= 128 and csr.nodes_per_tile == 8
          and getattr(csr, "tile_ptr", None) is not None and pre.is_contiguous() and N > 0 and lds <= 160 * 1024)
    if pre.dtype == torch.bfloat16:
        # bf16 S / dL/dS (KPGNN_STORE_BF16): the matrix-core variant only - no dictionary rows riding along (large batches, where
        # kpgnn_dict_grad takes them), <= 64 table rows, every entry multiplicity known to be below 64
        return ok and N >= 4096 and table_rows <= 64 and 1 <= csr.max_multiplicity() < 64
    return ok and pre.dtype == torch.float32


def combine_table_grad_raw(csr, pre, gh, theta, ptab, uid, n_code0, n_codek, want_gtheta, alphas=None, extra=None,
                           dict_rows=0, gdict_acc=None):
    """kpgnn_table_grad with the combine backward fused in (KP-GIN+ epilogue, fp32): computes g = theta[k]*gh[i]*gelu'(S[i,k]),
    the edge-code table gradients from it and (want_gtheta) the theta gradient / d/dalphas - `g` is written once and never read
    back for the tables.  Returns (g, gtheta or (gtheta, galphas) or None, gtable0, gtablek), or None when the shape has no
    fused kernel (the caller then runs combine_bwd_raw + table_grad_raw).
    dict_rows > 0: the dictionary gradient (theta[k]*gh[i] per (node, hop) id) rides along the walk and is returned as a
    fifth value (small batches, where a separate dict_grad launch costs more than it saves).
    gdict_acc: a [n_dict, D] buffer the dictionary gradient (in-walk or `extra`) is ADDED to instead of being written."""
    lib = _lib.load()
    N, K, D = pre.shape
    dev = pre.device
    nk = n_codek if K > 1 else 0
    if not _combine_table_grad_ok(csr, pre, n_code0 + nk, ptab.shape[0] if (ptab is not None and uid is not None) else 0):
        return None
    gd = None
    if dict_rows > 0 and pre.dtype == torch.bfloat16:
        return None                     # (bf16 storage: the matrix-core variant carries no dictionary rows)
    if dict_rows > 0:
        pack, kf = dict_tile_pack(csr, uid)
        if pack is None:
            return None
    ws_bytes = lib.kpgnn_table_grad_workspace_bytes(N, K, D, csr.nodes_per_tile, max(n_code0, 1), nk, dict_rows)
    if ws_bytes == 0:
        return None
    d = _lib.TableGradDesc()
    d.N, d.K, d.D, d.nodes_per_tile, d.n_code0, d.n_codek = N, K, D, csr.nodes_per_tile, n_code0, nk
    d.n_dyn = dyn_ptr(N)
    if dict_rows > 0:
        gd = torch.empty((dict_rows, D), dtype=torch.float32, device=dev) if gdict_acc is None else gdict_acc
        d.n_dict, d.dict_src, d.uid, d.uid_stride, d.gdict = dict_rows, 1, uid.data_ptr(), uid.stride(0), gd.data_ptr()
        d.dict_pack, d.dict_pack_K = pack.data_ptr(), kf
    if gdict_acc is not None:
        assert gdict_acc.is_contiguous() and gdict_acc.dtype == torch.float32 and (dict_rows > 0 or extra is not None)
        d.accumulate_dict = 1
    tptr, tpack = csr.tile_list(K)
    d.tile_ptr, d.tile_pack = tptr.data_ptr(), tpack.data_ptr()
    d.max_multiplicity = csr.max_multiplicity()      # (< 64: the matrix-core kernel may take the table gradients)
    gh = gh.contiguous()
    theta = theta.contiguous()
    d.theta, d.gh = theta.data_ptr(), gh.data_ptr()
    gt0 = torch.empty((n_code0, D), dtype=torch.float32, device=dev)
    gtk = torch.empty((nk, D), dtype=torch.float32, device=dev) if nk > 0 else None
    d.gtable0, d.gtablek = gt0.data_ptr(), _ptr(gtk)
    ws = torch.empty(int(ws_bytes), dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), int(ws_bytes)
    # dL/dS leaves hop-major ([K][N][D]: the transposed gather of kpgnn_aggregate_bwd then reads one contiguous [N,D] slab
    # per hop, like the forward's hop slots, instead of rows K*D floats apart - 1.5x of its bytes reached HBM that way)
    g = torch.empty((K, N, D), dtype=pre.dtype, device=dev).permute(1, 0, 2)
    d.g_sn, d.g_sk = g.stride(0), g.stride(1)
    d.storage = 1 if pre.dtype == torch.bfloat16 else 0
    d.fuse_pre, d.fuse_g = pre.data_ptr(), g.data_ptr()
    if uid is not None and ptab is not None:
        d.fuse_ptab, d.fuse_uid, d.fuse_uid_stride, d.fuse_n_dict = ptab.data_ptr(), uid.data_ptr(), uid.stride(0), ptab.shape[0]
    gth = gal = fws = None
    if want_gtheta:
        gth = torch.empty((K, D), dtype=torch.float32, device=dev)
        nb = int(lib.kpgnn_table_grad_fuse_workspace_bytes(K, D))
        fws = torch.empty(nb, dtype=torch.uint8, device=dev)
        d.fuse_gtheta, d.fuse_workspace, d.fuse_workspace_bytes = gth.data_ptr(), fws.data_ptr(), nb
        if alphas is not None:
            gal = torch.empty_like(alphas)
            d.fuse_alphas, d.fuse_galphas = alphas.data_ptr(), gal.data_ptr()
    if extra is not None:
        eo = extra[0] if gdict_acc is None else gdict_acc
        assert eo.numel() == extra[0].numel()
        d.extra_out, d.extra_slab, d.extra_nslab, d.extra_elems = eo.data_ptr(), extra[1].data_ptr(), extra[2], extra[0].numel()
    waiting = take_reduce_job()        # (an earlier launch's deferred reduction rides along with the finishing launch)
    if waiting is not None:
        d.pending = ctypes.cast(ctypes.pointer(waiting[0]), ctypes.c_void_p)
    # bytes: S read, g written, gh read, pair list, tables
    _lib.launch("kpgnn_table_grad", dev, ctypes.byref(d), timed=("combine_table_grad", lambda: (
        8 * N * K * D + 4 * N * D + 4 * csr.active_pairs(K) + 4 * D * (n_code0 + nk))))
    if dict_rows > 0:
        return g, ((gth, gal) if gal is not None else gth), gt0, gtk, gd
    return g, ((gth, gal) if gal is not None else gth), gt0, gtk


def combine_bwd_raw(mode, pre, gout, theta, periph, ptab, uid, want_gtheta, want_gv, alphas=None):
    """Launch kpgnn_combine_bwd.  gout is gh [N,D] when theta is given, else dL/dout [N,K,D].
    Returns (g, gv or None, gtheta or None); with `alphas` (geometric combine) the third is (gtheta, galphas)."""
    lib = _lib.load()
    N, K, D = pre.shape
    dev = pre.device
    refuse_dynamic_rows("kpgnn_combine_bwd", N)
    d = _lib.CombineBwdDesc()
    d.N, d.K, d.D, d.mode = N, K, D, mode
    d.pre = pre.data_ptr()
    if theta is not None:
        d.gh, d.theta = gout.data_ptr(), theta.data_ptr()
    else:
        d.gout, d.go_sn, d.go_sk = gout.data_ptr(), gout.stride(0), gout.stride(1)
    if periph is not None:
        d.periph, d.p_sn, d.p_sk = periph.data_ptr(), periph.stride(0), periph.stride(1)
    elif uid is not None and ptab is not None:  # (P is only read for the theta gradient)
        d.ptab, d.uid, d.uid_stride = ptab.data_ptr(), uid.data_ptr(), uid.stride(0)
        d.n_dict = ptab.shape[0]
    bf16 = pre.dtype == torch.bfloat16    # KPGNN_STORE_BF16: S arrives and dL/dS leaves as bf16 rows
    d.storage = 1 if bf16 else 0
    g = torch.empty((N, K, D), dtype=pre.dtype, device=dev)
    gv = torch.empty((N, K, D), dtype=torch.float32, device=dev) if want_gv else None
    gth = torch.empty((K, D), dtype=torch.float32, device=dev) if want_gtheta else None
    d.g, d.gv, d.gtheta = g.data_ptr(), _ptr(gv), _ptr(gth)
    ws = gal = None
    if want_gtheta and alphas is not None:
        gal = torch.empty_like(alphas)
        d.alphas, d.galphas = alphas.data_ptr(), gal.data_ptr()
    if want_gtheta:
        nb = lib.kpgnn_combine_bwd_workspace_bytes(N, K, D)
        ws = torch.empty(int(nb), dtype=torch.uint8, device=dev)
        d.workspace, d.workspace_bytes = ws.data_ptr(), int(nb)
    _lib.launch("kpgnn_combine_bwd", dev, ctypes.byref(d), timed=("combine_bwd", lambda: (
        (2 if bf16 else 4) * N * K * D * (2 + (gv is not None) + (theta is None) + (periph is not None and want_gtheta))
        + (4 * N * D if theta is not None else 0))))
    if gal is not None:
        return g, gv, (gth, gal)
    return g, gv, gth


class KHopAggregate(torch.autograd.Function):
    """out[N,k,D] (or hout[N,D] with a fused geometric combine) = epilogue(K-hop segmented sum).

    Differentiable w.r.t. x, table0, tablek, periph (dense) or ptab (dictionary), eps, theta.  `xbias` (a
    detached constant row, see kpgnn.h) carries no gradient: it is the padding row of hopk_node_path_emb,
    whose grad the reference's nn.Embedding(padding_idx=0) discards as well.

    Backward = five stages, each a function below the class:
      1. epilogue    g = dL/dS, dL/dP, the theta / alphas gradient: the fused combine + table-gradient kernel (KP-GIN+ with a
                     fused combine, dictionary P and code tables: the table gradients and this layer's dictionary share come
                     with it), else kpgnn_combine_bwd (an activation or a fused combine), else g = dL/dout;
      2. tables      kpgnn_dict_grad / kpgnn_table_grad for the edge-code tables and the dictionary (no atomics) - or the
                     tables are left to the gather; skipped after the fused kernel;
      3. dictionary  the layer's share (_DictShare) settled against the cell of a dictionary several layers read;
      4. gather      dL/dx: the pull form (kpgnn_khop_pull_gather, one launch per state) or kpgnn_aggregate_bwd;
      5. tails       d/dalphas through theta where no finishing launch produced it, the eps gradient."""

    @staticmethod
    def forward(ctx, x, table0, tablek, periph, eps, theta, xbias, ptab, csr, k_act, mode, uid, cells, *xs):
        # cells: per-hop inputs -> list of the slots' gradient cells; one [N,K,D] input -> the gradient cell of the STATE that x
        # is a view of (or None): its other readers' gradients are then collected in one buffer (see khop_aggregate)
        ctx.cells = cells if xs else None
        ctx.x_cell = cells if (not xs and cells is not None) else None
        _require_cuda(x, table0, tablek, periph, eps, theta, xbias, ptab, uid, *xs)
        ctx.n_slots = len(xs)
        bf16 = False
        if xs:   # per-hop inputs: k separate [N,D] states instead of one stacked [N,k,D] tensor
            assert x is None and len(xs) == k_act
            # bf16 storage (set_storage_dtype): only the configuration the bf16 kernels exist for - the fused KP-GIN+
            # epilogue with a dictionary P and code tables; everything else stays fp32
            bf16 = (_STORAGE is torch.bfloat16 and mode == MODE_GINPLUS and theta is not None and ptab is not None
                    and periph is None and table0 is not None and xs[0].shape[1] % 8 == 0 and eps is None and k_act > 1)
            # (k_act > 1: the single-hop first layer reads the raw input embedding once - nothing to save, and its rounding
            #  is what the ill-conditioned gradients of the input encoders' scalar gates feel first)
            xs = [bf16_shadow(t) if bf16 else t.float() for t in xs]
            if ctx.cells:   # will this reader's backward be the pull form?  (not with the unfused epilogue - the attention combine hands
                            #  back a node-major [N,k,D] gradient - and not with bf16 storage, whose dL/dS is bf16)
                ctx.cells[0].pull_reader = bool(PULL_GATHER and mode == MODE_GINPLUS and theta is not None and eps is None and not bf16)
            # the kernel reads every hop slot with ONE row stride (x_sn): row-strided slots (column slices of the bodies'
            # jumping-knowledge buffer) are read where they are; only mixed layouts are copied
            if any(t.stride(1) != 1 for t in xs) or len({t.stride(0) for t in xs}) != 1:
                xs = [t.contiguous() for t in xs]
        else:
            x = _last_contig(x.float())
        if periph is not None:
            periph = _last_contig(periph.float())
            ptab = uid = None
        # a dictionary every layer of a sequential stack reads (the bodies mark it, body._peripheral): its gradient is collected
        # in ONE buffer.  The first reader in forward order is the last to run backward: it hands autograd the total.
        ctx.dict_cell, ctx.dict_first = None, False
        if ptab is not None and getattr(ptab, "_kp_shared_grad", False):
            c = getattr(ptab, "_kp_grad_cell", None)
            ctx.dict_first = c is None
            if c is None:
                c = ptab._kp_grad_cell = _SlotGradCell()
            ctx.dict_cell = c
        if table0 is not None:
            table0 = table0.contiguous()
            tablek = tablek.contiguous() if tablek is not None else None
            _check_codes(csr, k_act, table0, tablek)
        alphas = None
        if theta is not None and theta.dim() == 1:
            # GeometricCombine.alphas [D]: theta = softmax_k(a (1-a)^k) is computed by the aggregation launch itself
            alphas = theta.contiguous()
            theta = torch.empty((k_act, alphas.numel()), dtype=torch.float32, device=alphas.device)
        elif theta is not None:
            theta = theta.contiguous()
        if ptab is not None:
            ptab = ptab.contiguous()
        need_pre = mode in (MODE_GINPLUS, MODE_GCN) or theta is not None
        out, pre = aggregate_fwd_raw(csr, k_act, mode, x, table0, tablek, periph, eps, theta, xbias, need_pre,
                                     ptab=ptab, uid=uid, xs=list(xs) if xs else None, alphas=alphas, bf16=bf16)
        ctx.alphas = alphas
        ctx.csr, ctx.k_act, ctx.mode, ctx.uid = csr, k_act, mode, uid
        ctx.has_tables = table0 is not None
        ctx.n_code0 = table0.shape[0] if table0 is not None else 0
        ctx.n_codek = tablek.shape[0] if tablek is not None else 0
        ctx.has_periph = periph is not None
        ctx.n_dict = ptab.shape[0] if ptab is not None else 0
        eps_needs = eps is not None and eps.requires_grad
        if eps_needs and xs:
            x = torch.stack(list(xs), dim=1)
        ctx.save_for_backward(pre, eps, theta, periph if theta is not None else None,
                              x if eps_needs else None, xbias if eps_needs else None,
                              ptab if theta is not None else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        pre, eps, theta, periph, x_saved, xbias, ptab = ctx.saved_tensors
        gout = gout.contiguous() if theta is not None else _last_contig(gout)
        want_tables = ctx.has_tables and (_needs(ctx, "table0") or _needs(ctx, "tablek"))
        want_gdict = ctx.n_dict > 0 and _needs(ctx, "ptab")
        want_gperiph = ctx.has_periph and _needs(ctx, "periph")
        g, gperiph, gtheta, galphas, tables, share = _epilogue_bwd(ctx, pre, theta, periph, ptab, gout,
                                                                   want_tables, want_gdict, want_gperiph)
        tables_in_gather = False
        if tables is None:                # (only the fused epilogue brings the table gradients and a dictionary share along)
            tables, tables_in_gather, share = _table_stage(ctx, g, gout, theta, want_tables, want_gdict)
        gdict = _settle_dict_share(ctx.dict_cell, ctx.dict_first, share, ctx.n_dict) if want_gdict else None
        if _pull_form_applies(ctx, g, eps, tables_in_gather):
            slots = [_gather_pull(ctx, g)] + [None] * (ctx.k_act - 1)
            gtheta = _finish_gtheta(ctx, gtheta, galphas, theta)
            return _input_grads(table0=tables[0], tablek=tables[1], periph=gperiph, theta=gtheta, ptab=gdict, slots=slots)
        gx, gathered = _gather_push(ctx, g, eps, tables_in_gather)
        if tables_in_gather:
            tables = gathered
        gtheta = _finish_gtheta(ctx, gtheta, galphas, theta)
        geps = _eps_grad(ctx, g, eps, x_saved, xbias)
        # (row 0 of both table grads stays exactly zero: code 0 == "inactive" never enters the CSR, which
        #  is also what nn.Embedding(padding_idx=0) would do)
        if ctx.n_slots:
            return _input_grads(table0=tables[0], tablek=tables[1], periph=gperiph, eps=geps, theta=gtheta, ptab=gdict,
                                slots=_slot_grads(ctx, gx))
        return _input_grads(x=gx if _needs(ctx, "x") else None, table0=tables[0], tablek=tables[1], periph=gperiph, eps=geps,
                            theta=gtheta, ptab=gdict)


# The one place that knows where KHopAggregate.forward's inputs stand: the names of its arguments after ctx, in order (the
# per-hop slots `*xs` follow them).
_INPUTS = ("x", "table0", "tablek", "periph", "eps", "theta", "xbias", "ptab", "csr", "k_act", "mode", "uid", "cells")
_INPUT_POS = {n: i for i, n in enumerate(_INPUTS)}


def _needs(ctx, name):
    return ctx.needs_input_grad[_INPUT_POS[name]]


def _input_grads(slots=(), **named):
    """The tuple backward hands autograd: the named gradients at their inputs' positions, None elsewhere, then the slots'."""
    assert named.keys() <= _INPUT_POS.keys()
    return (*(named.get(n) for n in _INPUTS), *slots)


# This layer's share of the peripheral dictionary's gradient, and where it is:
#   grad           the tensor, or None (nothing asked, or the share waits elsewhere: `parked`);
#   includes_cell  a finishing launch has already ADDED the dictionary cell's buffer (the later layers' shares) into `grad`;
#   parked         the share waits in the cell's list (_SlotGradCell.park_dict) for the ONE kpgnn_dict_grad_multi launch of
#                  the pass: `grad` is None.
_DictShare = collections.namedtuple("_DictShare", "grad includes_cell parked", defaults=(None, False, False))


# ---- stage 1: the epilogue's backward - g = dL/dS from dL/dout
def _epilogue_bwd(ctx, pre, theta, periph, ptab, gout, want_tables, want_gdict, want_gperiph):
    """Returns (g, gperiph, gtheta, galphas, tables, share).  galphas: d/dalphas where the finishing launch produced it (gtheta
    is then None).  tables = (gtable0, gtablek) and share (a _DictShare) only from the fused route, else None: the table stage
    then follows."""
    if (theta is not None and ctx.mode == MODE_GINPLUS and want_tables and periph is None and not want_gperiph
            and _combine_table_grad_ok(ctx.csr, pre, ctx.n_code0 + (ctx.n_codek if ctx.k_act > 1 else 0), ctx.n_dict)):
        r = _epilogue_fused(ctx, pre, theta, ptab, gout, want_gdict)
        if r is not None:
            return r
    if theta is not None or ctx.mode in (MODE_GINPLUS, MODE_GCN):
        return _epilogue_combine_bwd(ctx, pre, theta, periph, ptab, gout, want_gperiph)
    return gout, (gout if want_gperiph else None), None, None, None, None            # identity: g = dL/dout = dL/dP


def _epilogue_fused(ctx, pre, theta, ptab, gout, want_gdict):
    """KP-GIN+ with the fused combine, dictionary P and edge-code tables: ONE kernel computes dL/dS from S and gh, writes it
    for the gather and takes the table gradients from the LDS copy of each tile.  The dictionary gradient comes from gh alone:
    large batches park it for the pass's one multi-layer launch or run kpgnn_dict_grad, whose partial sums the same finishing
    launch adds up; small ones let the dictionary rows ride along the walk.  None: no fused kernel for this shape after all."""
    csr, uid, cell = ctx.csr, ctx.uid, ctx.dict_cell
    acc = cell.buf if (want_gdict and cell is not None) else None     # later layers' share: the finishing launch adds to it
    dg, parked = None, False
    if want_gdict and pre.shape[0] >= 4096:
        if cell is not None and dict_multi_ok(uid, ctx.n_dict, theta, gout):
            cell.park_dict(uid, theta, gout)        # ONE launch for all the layers, run by the last of them
            parked, acc = True, None
        else:
            dg = dict_grad_raw(uid, ctx.n_dict, theta, gout, defer=True)
    in_walk = ctx.n_dict if (want_gdict and dg is None and not parked) else 0    # small batches: the dictionary rows ride along
    r = combine_table_grad_raw(csr, pre, gout, theta, ptab, uid, ctx.n_code0, ctx.n_codek, want_gtheta=_needs(ctx, "theta"),
                               alphas=ctx.alphas, extra=dg, dict_rows=in_walk, gdict_acc=acc)
    if r is None and in_walk:                       # the one retry: without dictionary rows (and without the cell's buffer)
        r = combine_table_grad_raw(csr, pre, gout, theta, ptab, uid, ctx.n_code0, ctx.n_codek, want_gtheta=_needs(ctx, "theta"),
                                   alphas=ctx.alphas)
        in_walk = 0
    if r is None:
        if parked:                                  # (the share goes the plain way, through the table stage)
            cell.unpark_dict()
        if dg is not None:
            raise _lib.KpgnnError("table_grad refused a shape after dict_grad deferred its reduction to it")
        return None
    g, gtheta, gt0, gtk = r[:4]
    gtheta, galphas = (None, gtheta[1]) if isinstance(gtheta, tuple) else (gtheta, None)
    if dg is not None:
        share = _DictShare(dg[0] if acc is None else acc, includes_cell=acc is not None)
    elif in_walk:
        share = _DictShare(r[4], includes_cell=acc is not None)
    elif want_gdict and not parked:
        share = _DictShare(table_grad_raw(csr, g, 0, 0, edges=False, uid=uid, n_dict=ctx.n_dict, theta=theta, gh=gout)[2])
    else:
        share = _DictShare(parked=parked)
    return g, None, gtheta, galphas, (gt0, gtk), share


def _epilogue_combine_bwd(ctx, pre, theta, periph, ptab, gout, want_gperiph):
    """kpgnn_combine_bwd: the activation's and / or the fused combine's backward (g, dL/dP as gv, theta gradient)."""
    fused = theta is not None
    g, gv, gtheta = combine_bwd_raw(ctx.mode, pre, gout, theta, periph, ptab, ctx.uid,
                                    want_gtheta=fused and _needs(ctx, "theta"),
                                    want_gv=fused and want_gperiph, alphas=ctx.alphas if fused else None)
    # (geometric combine: d/dalphas came with the same finishing launch)
    gtheta, galphas = (None, gtheta[1]) if isinstance(gtheta, tuple) else (gtheta, None)
    return g, (gv if fused else (gout if want_gperiph else None)), gtheta, galphas, None, None


# ---- stage 2: table gradients (edge codes + peripheral dictionary), column-private kernel; not after the fused epilogue
def _table_stage(ctx, g, gout, theta, want_tables, want_gdict):
    """Returns ((gtable0, gtablek), tables_in_gather, share): tables_in_gather = the gather computes the table gradients
    (GCN's per-edge weights, or a shape kpgnn_table_grad refuses) and the pair is still (None, None)."""
    gt0 = gtk = gdict = None
    if not (want_tables or want_gdict):
        return (gt0, gtk), False, _DictShare()
    csr, uid, cell = ctx.csr, ctx.uid, ctx.dict_cell
    fused = theta is not None
    need_act = ctx.mode in (MODE_GINPLUS, MODE_GCN)
    edges_here = want_tables and ctx.mode != MODE_GCN   # GCN weights its table grads per edge: fused atomics
    dict_here = want_gdict and (fused or not need_act)  # g == dL/dP only without an activation
    res = extra = acc = None
    # (below ~4K nodes the walk's own dictionary path is cheaper than a second kernel: 1.44 vs 1.52 ms per step at
    #  batch 64, where every launch is latency-bound)
    if dict_here and fused and (g.shape[0] >= 4096 or not edges_here):   # from gh alone (20 MB, not [N,K,D])
        # (its partial sums are added up by table_grad's finishing launch when one follows)
        dg = dict_grad_raw(uid, ctx.n_dict, theta, gout, defer=edges_here)
        if dg is not None:
            dict_here = False
            if edges_here:
                gdict, extra = dg[0], dg
            else:
                gdict = dg
    if edges_here or dict_here:
        if dict_here and cell is not None:
            acc = cell.buf                       # later layers' share: this call's finishing launch adds to it
        res = table_grad_raw(csr, g, ctx.n_code0, ctx.n_codek, edges=edges_here,
                             uid=uid if dict_here else None, n_dict=ctx.n_dict if dict_here else 0,
                             theta=theta if fused else None, gh=gout if fused else None, extra=extra, gdict_acc=acc)
        if res is None and extra is not None:
            raise _lib.KpgnnError("table_grad refused a shape after dict_grad deferred its reduction to it")
    if res is not None:
        gt0, gtk = res[0], res[1]
        gdict = res[2] if gdict is None else gdict
    if want_gdict and gdict is None:  # activation without fused combine (or oversize tables): dL/dP = gout
        r2 = table_grad_raw(csr, gout if not fused else (gout.unsqueeze(1) * theta.unsqueeze(0)),
                            0, 0, edges=False, uid=uid, n_dict=ctx.n_dict)
        if r2 is None:
            raise _lib.KpgnnError("peripheral dictionary too large for the LDS table-gradient kernel; "
                                  "pass a dense peripheral_attr instead")
        gdict = r2[2]
    return (gt0, gtk), want_tables and (res is None or not edges_here), _DictShare(gdict, res is not None and acc is not None)


# ---- stage 3: this layer's dictionary share against the cell of a dictionary that several layers read
def _settle_dict_share(cell, first, share, n_dict):
    """What this layer hands autograd for the dictionary: its own share without a cell; with one, None unless it is the
    FIRST reader in forward order - the last to run backward - which hands over the total and clears the cell.

      parked and not first         nothing: the share waits in the cell's list, a share in `cell.buf` stays where it is.
      otherwise                    total = share.grad
        first                        + the ONE multi-layer launch over what the layers parked (its own share included),
        not share.includes_cell      + cell.buf, if there is one                                    - in THIS order;
      first                        return the total, clear the cell;  else  cell.buf = total, return None.

    `cell.buf` is added here exactly when no finishing launch has added it already (the single-scope backward wrote this as
    "the buffer was not handed to a launch, and (not done or dict_parked)", done = the fused epilogue ran):
      fused epilogue, dict_grad deferred or rows in the walk   the launch was given cell.buf: includes_cell whenever there
                                                               was one, and nothing to add when there was none;
      fused epilogue, after the retry without dictionary rows  the share is a fresh tensor: added here;
      fused epilogue, parked (this is then the first reader)   the total starts from the multi launch's result: added here;
      table stage                                              includes_cell only if table_grad took the dictionary rows
                                                               itself and was given cell.buf; every other path (dict_grad,
                                                               the dL/dP = gout fallback): added here."""
    if cell is None:
        return share.grad
    if share.parked and not first:
        return None
    total = share.grad
    if first:
        items = cell.take_dicts()
        if items:
            gm = dict_grad_multi_raw(items, n_dict)
            total = gm if total is None else total + gm
    if not share.includes_cell and cell.buf is not None:
        total = total + cell.buf                     # (a path without the accumulating launch: add the parked share the plain way)
    cell.buf = None if first else total
    return total if first else None


# ---- stage 4: the transposed gather - dL/dx (or the hop slots' gradients) from g
def _pull_form_applies(ctx, g, eps, tables_in_gather):
    """Pull form (KP-GIN+ history pattern, large batches): this layer's hop slabs of g are parked with the states it read as
    slots >= 1; the state it read as slot 0 - whose last reader it is - gets its WHOLE gradient from one gather."""
    return (PULL_GATHER and ctx.n_slots > 0 and ctx.cells is not None and ctx.mode == MODE_GINPLUS and not tables_in_gather
            and eps is None and g.dtype == torch.float32 and g.shape[0] >= 4096 and g.shape[2] % 4 == 0 and ctx.k_act <= 16
            and all(g[:, k].is_contiguous() for k in range(ctx.k_act)))


def _gather_pull(ctx, g):
    """d/d(slot-0 state): one gather over the slabs later layers parked for it, this layer's hop-0 slab and whatever share
    the cell already holds.  Parks this layer's other slabs with the states it read them from."""
    for k in range(1, ctx.k_act):
        ctx.cells[k].park_slab(k, g[:, k])
    c0 = ctx.cells[0]
    pend = c0.take_slabs()
    top = max(pend) if pend else 0
    zeros = None
    slabs = [g[:, 0]]
    for h in range(1, top + 1):
        t = pend.get(h)
        if t is None:            # (a hop nobody parked - a pruned backward pass: gathered from zeros)
            zeros = torch.zeros_like(slabs[0]) if zeros is None else zeros
            t = zeros
        slabs.append(t)
    hb = c0.buf
    shape = tuple(slabs[0].shape)
    ok = lambda t: t is not None and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == shape
    hinit = hb if ok(hb) else None
    ext = c0.take_addend()
    hinit2 = ext if ok(ext) else None
    total = khop_pull_gather(ctx.csr, slabs[:16], hinit, hinit2)
    if hb is not None and hinit is None:
        total = total + hb.view_as(total)          # (odd layout: add the parked share the plain way)
    if ext is not None and hinit2 is None:
        total = total + ext.view_as(total)
    c0.buf = None
    return total


def _x_cell_accumulator(ctx, g, tables_in_gather):
    """The buffer of the state's cell (x_state) when kpgnn_aggregate_bwd can add dL/dx into it in place, else None."""
    if (ctx.x_cell is not None and ctx.x_cell.buf is not None and _needs(ctx, "x") and ctx.k_act <= 32
            and ctx.mode != MODE_GCN and not tables_in_gather):
        b = ctx.x_cell.buf
        if b.is_contiguous() and b.numel() == g.numel() and b.dtype == torch.float32:
            return b
    return None


def _gather_push(ctx, g, eps, tables_in_gather):
    """kpgnn_aggregate_bwd, adding into the cells' buffers where it can, and whatever was left for this layer's states by
    readers that counted on another form.  Returns (gx, (gtable0, gtablek) of the gather)."""
    xbuf = _x_cell_accumulator(ctx, g, tables_in_gather)
    gx, a0, ak = aggregate_bwd_raw(ctx.csr, ctx.k_act, ctx.mode, g, eps, ctx.n_code0, ctx.n_codek, tables_in_gather,
                                   slots=ctx.n_slots > 0, slot_bufs=_slot_bufs(ctx), gx_accum=xbuf)
    if ctx.n_slots > 0 and ctx.cells is not None:
        ext = ctx.cells[0].take_addend()      # (a share handed over for the pull form that this layer could not run)
        if ext is not None:
            gx = list(gx)
            gx[0] = gx[0] + ext.view_as(gx[0])
        pend = ctx.cells[0].take_slabs()      # (later layers ran the pull form, this one could not: their slabs for ITS slot-0 state)
        if pend:
            zeros = torch.zeros_like(next(iter(pend.values())))
            extra = khop_pull_gather(ctx.csr, [pend.get(h, zeros) for h in range(0, max(pend) + 1)], None)
            gx = list(gx)
            gx[0] = gx[0] + extra
    if ctx.x_cell is not None:
        if xbuf is None and ctx.x_cell.buf is not None and _needs(ctx, "x"):
            gx = gx + ctx.x_cell.buf.view_as(gx)     # (odd layout: add the parked share the plain way)
        ctx.x_cell.buf = None
    return gx, (a0, ak)


# ---- stage 5: the scalar tails
def _eps_grad(ctx, g, eps, x_saved, xbias):
    if eps is None or not _needs(ctx, "eps") or ctx.mode != MODE_GIN:
        return None
    refuse_dynamic_rows("the eps gradient (framework sum over rows)", g.shape[0])
    xe = x_saved
    if xbias is not None and xe.shape[1] > 1:
        xe = torch.cat([xe[:, :1], xe[:, 1:] + xbias], dim=1)
    return (g * xe).sum().reshape(eps.shape)


def _finish_gtheta(ctx, gtheta, galphas, theta):
    """What the `theta` input gets: d/dalphas - through theta (geo_theta.hip) when the finishing launch has not already
    produced it - where the input was a GeometricCombine's alphas, else the theta gradient."""
    if galphas is not None:
        return galphas
    if gtheta is not None and ctx.alphas is not None:
        galpha = torch.empty_like(ctx.alphas)
        _lib.launch("kpgnn_geo_theta_bwd", galpha.device,
                    ctx.alphas.data_ptr(), theta.data_ptr(), gtheta.data_ptr(), ctx.k_act, ctx.alphas.numel(), galpha.data_ptr())
        return galpha
    return gtheta


def _backward_pass_id():
    """Identity of the autograd backward pass that is executing (-1 outside one)."""
    try:
        return torch._C._current_graph_task_id()
    except AttributeError:  # pragma: no cover - older torch
        return -1


class _PassTagged:
    """A value and the backward pass that wrote it (torch._C._current_graph_task_id()): read from any other pass, it is gone."""
    __slots__ = ("v", "task")

    def __init__(self):
        self.v, self.task = None, -1

    def get(self):
        if self.v is not None and self.task != _backward_pass_id():
            self.v = None                # written by another backward pass: stale
        return self.v

    def set(self, v):
        self.v = v
        self.task = _backward_pass_id() if v is not None else -1

    def take(self):
        v = self.get()
        self.v, self.task = None, -1
        return v


class _SlotGradCell:
    """Gradient buffer of one state tensor that several layers read as a hop slot (see khop_aggregate).

    Cells carry part of d/dstate OUTSIDE autograd: a reader parks its share in `buf`, later readers (in backward order) add
    to it in place and the state's last reader hands autograd the total and clears the cell.  That is only sound within ONE
    backward pass.  A pruned or partial pass (`autograd.grad(score, some_params, retain_graph=True)`) may park a share that
    no reader of ITS pass ever collects; everything parked is therefore tagged with the pass that wrote it (_PassTagged) and
    reads from any other pass see an empty cell - a stale share is never added to a later pass's gradient
    (tests/test_gpu_parity.py::test_gradient_cells_survive_a_partial_backward)."""
    __slots__ = ("_share", "_slabs", "_addend", "_dicts", "pull_reader")

    def __init__(self):
        self._share = _PassTagged()             # `buf`
        self._slabs = _PassTagged()             # {hop: [N,D] slab} of the pull gather
        self._addend = _PassTagged()            # one more [N,D] addend of the pull gather (the residual branch's share)
        self._dicts = _PassTagged()             # dictionary cell: the (uid, theta, gh) of the layers whose share waits for ONE launch
        self.pull_reader = False                # set in forward by the state's slot-0 reader when its backward will be the pull
                                                # form (fused geometric combine): only then is an addend worth parking

    # what is held whatever pass wrote it (the tests look at a cell after the backward pass has ended)
    _buf = property(lambda self: self._share.v)
    _add = property(lambda self: self._addend.v)

    # One dictionary-gradient launch for all the layers that read the dictionary (dict_grad_multi_raw): every reader parks
    # (uid view, theta, gh); the first reader in forward order - the last to run backward - runs the launch.
    def park_dict(self, uid, theta, gh):
        if self._dicts.get() is None:
            self._dicts.set([])
        self._dicts.v.append((uid, theta, gh))

    def unpark_dict(self):
        """Takes back the share this pass parked last (its layer hands it over another way after all)."""
        self._dicts.get().pop()

    def take_dicts(self):
        return self._dicts.take() or []

    def park_addend(self, t):
        self._addend.set(t)

    def take_addend(self):
        return self._addend.take()

    # Pull form of the backward gather (khop_pull_gather): a later reader of the state does not add its share into `buf` -
    # it leaves the hop slab of ITS dL/dS here, keyed by the hop slot it read the state at, and the state's last reader
    # gathers from all of them in one launch.
    def park_slab(self, hop, slab):
        if self._slabs.get() is None:
            self._slabs.set({})
        self._slabs.v[hop] = slab

    def take_slabs(self):
        return self._slabs.take() or {}

    @property
    def buf(self):
        return self._share.get()

    @buf.setter
    def buf(self, v):
        self._share.set(v)


def state_cell(t):
    """The gradient cell of a state tensor (created on first use): whoever computes part of d/dt BEFORE the state's last
    reader runs its backward may add it to `cell.buf` instead of handing autograd a tensor to sum."""
    c = getattr(t, "_kp_slot_cell", None)
    if c is None:
        c = t._kp_slot_cell = _SlotGradCell()
    return c


def _slot_bufs(ctx):
    return [c.buf for c in ctx.cells] if ctx.cells else None


def _slot_grads(ctx, gx):
    """With shared cells: slots >= 1 park their gradient in the state's cell (the kernel has added to it) and hand
    autograd nothing; slot 0 - by construction the LAST of a state's readers to run backward - returns the total."""
    if not ctx.cells:
        return gx
    out = []
    for k, c in enumerate(ctx.cells):
        if k == 0:
            out.append(gx[0])
            c.buf = None
        else:
            c.buf = gx[k]
            out.append(None)
    return out


def khop_aggregate(x, csr, k_act, mode, table0=None, tablek=None, periph=None, eps=None, theta=None, xbias=None,
                   share_slot_grads=False, x_state=None):
    """x: [N,k,D] tensor, or a list/tuple of k per-hop [N,D] tensors (no stacking copy).
    periph: dense [N,k,D] tensor, a DictPeripheral, or None.
    theta: [k,D] hop weights of a fused combine, or the [D] `alphas` of a GeometricCombine (theta is then computed by the
    aggregation launch itself and differentiated back to alphas).
    share_slot_grads (per-hop list only): the caller guarantees the GNNPlus history pattern - slot k of layer m is the
    output of layer m-1-k, so every state is read as slot 0 by the layer right after it and as slots >= 1 only by LATER
    layers, whose backward autograd runs first.  The backward then accumulates a state's slot gradients in ONE buffer
    inside the gather kernel (kpgnn_agg_bwd_desc.accumulate_mask) instead of emitting one [N,D] tensor per reader
    for autograd to add up (36 adds of 19.7 MB per step at K = L = 8)."""
    ptab = uid = None
    if isinstance(periph, DictPeripheral):
        ptab, uid, periph = periph.table, periph.uid, None
    if isinstance(x, (list, tuple)):
        cells = None
        if share_slot_grads and torch.is_grad_enabled():
            cells = [state_cell(t) for t in x]
        return KHopAggregate.apply(None, table0, tablek, periph, eps, theta, xbias, ptab, csr, k_act, mode, uid, cells, *x)
    # x_state: the [N, K*D] state tensor that x is a view of, when the caller guarantees that this call is the LAST of the
    # state's readers to run backward (the bodies: the jumping-knowledge projection and the next norm's residual branch read
    # it too, both later in the forward).  Those readers park their share of d/dstate in the state's cell and the gather
    # kernel adds its own into the same buffer - no [N,H] tensors for autograd to sum.
    cell = None
    if x_state is not None and torch.is_grad_enabled() and x_state.requires_grad and x_state.is_cuda:
        cell = state_cell(x_state)
    return KHopAggregate.apply(x, table0, tablek, periph, eps, theta, xbias, ptab, csr, k_act, mode, uid, cell)


class DictRows(torch.autograd.Function):
    """out[i,k,:] = table[uid[i,k],:]; backward through kpgnn_table_grad (dictionary part, no atomics)."""

    @staticmethod
    def forward(ctx, table, uid):
        ctx.save_for_backward(uid)
        ctx.n = table.shape[0]
        return table.index_select(0, uid.reshape(-1).long()).view(uid.shape[0], uid.shape[1], table.shape[1])

    @staticmethod
    def backward(ctx, gout):
        (uid,) = ctx.saved_tensors
        gout = _last_contig(gout)

        class _C:  # table_grad_raw only needs the tile size from the CSR when there is no pair list
            nodes_per_tile = 8 if gout.shape[1] <= 8 else max(1, 64 // gout.shape[1])
        res = table_grad_raw(_C, gout, 0, 0, edges=False, uid=uid, n_dict=ctx.n)
        if res is None:
            g = torch.zeros((ctx.n, gout.shape[2]), dtype=gout.dtype, device=gout.device)
            return g.index_add_(0, uid.reshape(-1).long(), gout.reshape(-1, gout.shape[2])), None
        return res[2], None


# ------------------------------------------------------------------------------------------------ table gather-sum
class TableGatherSum(torch.autograd.Function):
    """out[m,:] = bias + sum_c table[col_offset[c] + idx[m,c], :]  (kpgnn_table_gather_sum_fwd/bwd)."""

    @staticmethod
    def forward(ctx, table, bias, idx, col_offset):
        _require_cuda(table, bias, idx, col_offset)
        table = table.contiguous()
        bias = bias.contiguous() if bias is not None else None
        M, C = idx.shape
        R, D = table.shape
        out = torch.empty((M, D), dtype=torch.float32, device=table.device)
        d = _lib.TgsDesc()
        d.M, d.C, d.D, d.R = M, C, D, R
        d.n_dyn = dyn_ptr(M)
        d.idx, d.col_offset, d.table, d.bias = idx.data_ptr(), col_offset.data_ptr(), table.data_ptr(), _ptr(bias)
        d.out, d.out_stride = out.data_ptr(), out.stride(0)
        _lib.launch("kpgnn_table_gather_sum_fwd", table.device, ctypes.byref(d))
        ctx.save_for_backward(idx, col_offset)
        ctx.shape = (R, D)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        idx, col_offset = ctx.saved_tensors
        lib = _lib.load()
        gout = _last_contig(gout)
        R, D = ctx.shape
        M, C = idx.shape
        gtable = torch.empty((R, D), dtype=torch.float32, device=gout.device)
        nb = int(lib.kpgnn_table_gather_sum_bwd_workspace_bytes(M, D, R))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=gout.device)
        d = _lib.TgsDesc()
        d.M, d.C, d.D, d.R = M, C, D, R
        d.n_dyn = dyn_ptr(M)
        d.idx, d.col_offset = idx.data_ptr(), col_offset.data_ptr()
        d.gout, d.gout_stride, d.gtable = gout.data_ptr(), gout.stride(0), gtable.data_ptr()
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        _lib.launch("kpgnn_table_gather_sum_bwd", gout.device, ctypes.byref(d))
        if ctx.has_bias:
            refuse_dynamic_rows("the bias gradient of a table gather-sum (framework row sum)", M)
        gbias = gout.sum(0) if ctx.has_bias else None
        return gtable, gbias, None, None


def table_gather_sum(table, bias, idx, col_offset):
    return TableGatherSum.apply(table, bias, idx, col_offset)


_I16 = "_kpgnn_idx16"
_ZERO_OFF = {}


def _zero_offset(dev):
    """One int32 zero per device: the column offset of a single-table gather-sum."""
    t = _ZERO_OFF.get(dev)
    if t is None:
        t = _ZERO_OFF[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


class _ZeroRowGrad(torch.autograd.Function):
    """Identity whose backward zeroes one row of the gradient: nn.Embedding(padding_idx=r) semantics for a table that
    is read through the gather-sum kernels."""

    @staticmethod
    def forward(ctx, weight, row):
        ctx.row = row
        return weight.view_as(weight)

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[ctx.row].zero_()
        return g, None


def embedding_rows(weight, idx, padding_idx=None):
    """weight[idx] for an integer index tensor of any shape (the bodies' input embedding, input_encoder.py:21-22; the
    layers' path encoding, KPGIN.py:92-93) through the gather-sum kernels: unlike the framework's embedding backward
    (sort + unique_by_key with a host read-back, which FAULTS when a captured hipGraph replays it) this is free of
    host synchronisation.  The 16-bit copy of the index is cached on the index tensor object; building it validates
    the range once (one sync per index tensor, outside any capture), as nn.Embedding's device assert would.
    padding_idx: that row receives no gradient (its forward value is whatever the table holds, zeros for nn.Embedding)."""
    if idx.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8):
        raise TypeError(f"embedding_rows: integer index expected, got {idx.dtype}")
    R = weight.shape[0]
    if R > 65536:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.KpgnnError(f"embedding table with {R} rows > 65536 falls back to the framework's embedding, whose "
                                  "backward cannot be captured in a hipGraph (host read-back); run eagerly")
        return torch.nn.functional.embedding(idx.long(), weight, padding_idx=padding_idx)
    rec = getattr(idx, _I16, None)
    if rec is None or rec[0] != (idx._version, R):
        # a batch collated from a resident dataset (dataset.KHopDataset.collate) carries int16 indices whose dataset-wide
        # maximum is known on the host: no device round trip for the range check
        pre = getattr(idx, "_kp_index_bound", None)
        if pre is not None and pre[0] == idx._version and idx.dtype == torch.int16 and idx.is_contiguous():
            if pre[1] >= R:
                raise IndexError(f"embedding index {pre[1]} out of range for a table with {R} rows")
            rec = ((idx._version, R), idx.reshape(-1, 1), _zero_offset(idx.device))
            try:
                setattr(idx, _I16, rec)
            except Exception:  # pragma: no cover
                pass
    if rec is None or rec[0] != (idx._version, R):
        if torch.cuda.is_current_stream_capturing():
            raise _lib.KpgnnError("embedding_rows: first use of an index tensor inside a hipGraph capture (its range "
                                  "check needs a host sync); run one eager step on the batch before capturing")
        flat = idx.reshape(-1, 1)
        if flat.numel() and bool(((flat < 0) | (flat >= R)).any().item()):
            raise IndexError(f"embedding index out of range for a table with {R} rows")
        i64 = flat.long()
        i16 = (i64 if R <= 32768 else i64 - 65536 * (i64 >= 32768)).to(torch.int16).contiguous()
        off = torch.zeros(1, dtype=torch.int32, device=idx.device)
        rec = ((idx._version, R), i16, off)
        try:
            setattr(idx, _I16, rec)
        except Exception:  # pragma: no cover
            pass
    if padding_idx is not None and weight.requires_grad:
        weight = _ZeroRowGrad.apply(weight, int(padding_idx))
    res = TableGatherSum.apply(weight, None, rec[1], rec[2])
    return res.view(*idx.shape, weight.shape[1])


# ------------------------------------------------------------------------------------------------ graph readout
_GPTR = "_kpgnn_graph_ptr"


def graph_ptr_of(batch, num_graphs):
    """int32 [G+1] node offsets of the graphs of a collated batch (nodes of a graph are contiguous, as PyG's collate
    lays them out), cached on the `batch` tensor; checks once that `batch` is sorted (one sync per batch object)."""
    rec = getattr(batch, _GPTR, None)
    if rec is not None and rec[0] == (batch._version, num_graphs):
        return rec[1]
    if torch.cuda.is_current_stream_capturing():
        raise _lib.KpgnnError("graph readout: first use of a batch vector inside a hipGraph capture (its order check needs a "
                              "host sync); run one eager step on the batch before capturing")
    if batch.numel() > 1 and bool((batch[1:] < batch[:-1]).any().item()):
        raise ValueError("graph readout needs the nodes of every graph to be contiguous (sorted `batch`)")
    if batch.numel() and (int(batch[-1].item()) >= num_graphs or int(batch[0].item()) < 0):
        raise IndexError(f"graph readout: batch holds graph ids outside [0, {num_graphs})")
    ptr = torch.searchsorted(batch, torch.arange(num_graphs + 1, device=batch.device, dtype=batch.dtype)).to(torch.int32)
    try:
        setattr(batch, _GPTR, ((batch._version, num_graphs), ptr))
    except Exception:  # pragma: no cover
        pass
    return ptr


def _rows_view(t, C):
    """[N,C] fp32 rows the kernels can walk: unit column stride, rows that do not overlap (a column slice stays a view)."""
    return t if t.stride(1) == 1 and t.stride(0) >= C else t.contiguous()


def _segment_pool_launch(x, ptr, num_graphs, mean=False):
    """[G,D] sum / mean of the rows of x [N,D] per graph: one kpgnn_segment_pool_fwd launch."""
    N, D = x.shape
    x = _rows_view(x, D)
    out = torch.empty((num_graphs, D), dtype=torch.float32, device=x.device)
    d = _lib.PoolDesc()
    d.N, d.G, d.D, d.mode = N, num_graphs, D, 1 if mean else 0
    d.n_dyn = dyn_ptr(N)
    d.graph_ptr, d.x, d.x_stride, d.out = ptr.data_ptr(), x.data_ptr(), x.stride(0), out.data_ptr()
    _lib.launch("kpgnn_segment_pool_fwd", x.device, ctypes.byref(d))
    return out


class SegmentPool(torch.autograd.Function):
    """out[g] = sum / mean of the rows of graph g (kpgnn_segment_pool_*): one launch per direction, no atomics."""

    @staticmethod
    def forward(ctx, x, batch, ptr, num_graphs, mean):
        N, D = x.shape
        out = _segment_pool_launch(x, ptr, num_graphs, mean)
        ctx.save_for_backward(batch, ptr)
        ctx.dims = (N, D, num_graphs, mean)
        return out

    @staticmethod
    def backward(ctx, gout):
        batch, ptr = ctx.saved_tensors
        N, D, G, mean = ctx.dims
        gout = gout.contiguous()
        gx = torch.empty((N, D), dtype=torch.float32, device=gout.device)
        d = _lib.PoolDesc()
        d.N, d.G, d.D, d.mode = N, G, D, 1 if mean else 0
        d.n_dyn = dyn_ptr(N)
        d.graph_ptr, d.batch, d.gout, d.gx, d.gx_stride = ptr.data_ptr(), batch.data_ptr(), gout.data_ptr(), gx.data_ptr(), D
        _lib.launch("kpgnn_segment_pool_bwd", gout.device, ctypes.byref(d))
        return gx, None, None, None, None


def segment_pool(x, batch, num_graphs, mean=False):
    """Sum / mean readout of [N,D] node rows per graph on the HIP kernels (fp32 device tensors, int64 sorted batch)."""
    _require_cuda(x, batch)
    if x.shape[1] > 256:       # (kpgnn_segment_pool_* instantiates row widths up to 256 floats: wider rows take the framework's scatter)
        refuse_dynamic_rows("graph readout of rows wider than 256", x.shape[0])
        out = x.new_zeros((num_graphs, x.shape[1])).index_add_(0, batch.long(), x)
        if mean:
            cnt = x.new_zeros(num_graphs).index_add_(0, batch.long(), x.new_ones(batch.numel()))
            out = out / cnt.clamp(min=1).unsqueeze(-1)
        return out
    return SegmentPool.apply(x, batch.long() if batch.dtype != torch.int64 else batch, graph_ptr_of(batch, num_graphs), num_graphs, mean)


def _segment_max_launch(x, ptr, num_graphs, keep_arg):
    """([G,D] column-wise max of the rows of x [N,D] per graph, int32 [G,D] winning rows or None): one kpgnn_segment_max_fwd
    launch.  A strided x with unit column stride is read in place."""
    N, D = x.shape
    x = _rows_view(x, D)
    out = torch.empty((num_graphs, D), dtype=torch.float32, device=x.device)
    arg = torch.empty((num_graphs, D), dtype=torch.int32, device=x.device) if keep_arg else None
    d = _lib.PoolMaxDesc()
    d.N, d.G, d.D = N, num_graphs, D
    d.n_dyn = dyn_ptr(N)
    d.graph_ptr, d.x, d.x_stride, d.out, d.arg = ptr.data_ptr(), x.data_ptr(), x.stride(0), out.data_ptr(), _ptr(arg)
    _lib.launch("kpgnn_segment_max_fwd", x.device, ctypes.byref(d))
    return out, arg


class SegmentMax(torch.autograd.Function):
    """out[g] = column-wise max of the rows of graph g (kpgnn_segment_max_*): the lowest row that attains a column's max is its
    one winner and takes the whole gradient (torch_scatter.scatter_max, not amax's even split).  One launch per direction;
    only `batch` and the int32 winners are kept for backward, neither x nor the result."""

    @staticmethod
    def forward(ctx, x, batch, ptr, num_graphs):
        out, arg = _segment_max_launch(x, ptr, num_graphs, True)
        ctx.save_for_backward(batch, arg)
        ctx.dims = (x.shape[0], x.shape[1], num_graphs)
        return out

    @staticmethod
    def backward(ctx, gout):
        batch, arg = ctx.saved_tensors
        N, D, G = ctx.dims
        gout = gout.contiguous()
        gx = torch.empty((N, D), dtype=torch.float32, device=gout.device)
        d = _lib.PoolMaxDesc()
        d.N, d.G, d.D = N, G, D
        d.n_dyn = dyn_ptr(N)
        d.batch, d.arg, d.gout, d.gx, d.gx_stride = batch.data_ptr(), arg.data_ptr(), gout.data_ptr(), gx.data_ptr(), D
        _lib.launch("kpgnn_segment_max_bwd", gout.device, ctypes.byref(d))
        return gx, None, None, None


def segment_max(x, batch, num_graphs):
    """Max readout of [N,D] node rows per graph on the HIP kernels (fp32 device tensors, int64 sorted batch); an empty graph
    gives -inf.  Without autograd (grad disabled, or x does not require it) no winners are kept and nothing but the result is
    allocated."""
    _require_cuda(x, batch)
    if x.shape[1] > 256:       # (the row shapes instantiated stop at 256 floats, as for segment_pool: wider rows take the framework's scatter)
        refuse_dynamic_rows("max readout of rows wider than 256", x.shape[0])
        idx = batch.long().view(-1, 1).expand_as(x)
        return x.new_full((num_graphs, x.shape[1]), float("-inf")).scatter_reduce(0, idx, x, reduce="amax")
    ptr = graph_ptr_of(batch, num_graphs)
    if not (torch.is_grad_enabled() and x.requires_grad):
        return _segment_max_launch(x, ptr, num_graphs, False)[0]
    return SegmentMax.apply(x, batch.long() if batch.dtype != torch.int64 else batch, ptr, num_graphs)


# ------------------------------------------------------------------------------------------------ virtual node
def _vn_launch(x, v, ptr, num_graphs, want_pool, out=None):
    """(x + v[g], sum of that per graph + v or None) as one kpgnn_vn_add_pool launch; x [N,D], v [G,D] (row stride 0 allowed);
    into `out` when given (a contiguous [N,D] fp32 tensor)."""
    N, D = x.shape
    x = _rows_view(x, D)
    if v.stride(1) != 1 or 0 < v.stride(0) < D:
        v = v.contiguous()
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (N, D) and out.is_contiguous()
    pooled = torch.empty((num_graphs, D), dtype=torch.float32, device=x.device) if want_pool else None
    d = _lib.VnDesc()
    d.N, d.G, d.D = N, num_graphs, D
    d.n_dyn = dyn_ptr(N)
    d.graph_ptr, d.x, d.x_stride, d.v, d.v_stride = ptr.data_ptr(), x.data_ptr(), x.stride(0), v.data_ptr(), v.stride(0)
    d.out, d.out_stride, d.pooled = out.data_ptr(), D, _ptr(pooled)
    _lib.launch("kpgnn_vn_add_pool", x.device, ctypes.byref(d))
    return out, pooled


class VirtualNodeAdd(torch.autograd.Function):
    """out = x + vn[graph of the row], pooled = per-graph sum of out + vn (kpgnn_vn_add_pool): one launch per direction - the
    backward (gx = gout + gpooled[g], gvn = per-graph sum of gx + gpooled) is the same kernel on the gradients.  Without
    `pooled`, gx is gout itself and gvn one segmented sum."""

    @staticmethod
    def forward(ctx, x, vn, ptr, num_graphs, want_pool):
        out, pooled = _vn_launch(x, vn, ptr, num_graphs, want_pool)
        ctx.save_for_backward(ptr)
        ctx.dims = (num_graphs, want_pool)
        return out, pooled

    @staticmethod
    def backward(ctx, gout, gpooled):
        ptr, = ctx.saved_tensors
        G, want_pool = ctx.dims
        if want_pool:
            gx, gv = _vn_launch(gout, gpooled, ptr, G, True)
            return gx, gv, None, None, None
        gv = _segment_pool_launch(gout, ptr, G) if ctx.needs_input_grad[1] else None
        return gout, gv, None, None, None


def virtual_node_add(x, vn, batch, num_graphs, want_pool):
    """The virtual node's two node-level steps (models/GNNs.py:196-199,227-230) for x [N,D] and the virtual-node rows vn [G,D]
    (an expanded single row is read as such): returns (x + vn[batch], global_add_pool(x + vn[batch]) + vn or None).
    fp32 device tensors up to D = 256 run kpgnn_vn_add_pool, driven by the graph pointer of `batch` (rows beyond its last
    entry are left alone: safe on a dataset.StaticBatch); everything else keeps the framework expression."""
    if not (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and vn.dtype == torch.float32 and x.shape[1] <= 256
            and tuple(vn.shape) == (num_graphs, x.shape[1])):
        if x.is_cuda:
            refuse_dynamic_rows("the virtual node on the framework path", x.shape[0])
        out = x + vn[batch]
        if not want_pool:
            return out, None
        if out.is_cuda and out.dim() == 2 and out.dtype == torch.float32:
            return out, segment_pool(out, batch, num_graphs) + vn
        return out, out.new_zeros((num_graphs,) + tuple(out.shape[1:])).index_add_(0, batch, out) + vn
    _require_cuda(vn, batch)
    ptr = graph_ptr_of(batch, num_graphs)
    if not torch.is_grad_enabled() or not (x.requires_grad or vn.requires_grad):
        return _vn_launch(x, vn, ptr, num_graphs, want_pool)        # no autograd node, nothing saved
    return VirtualNodeAdd.apply(x, vn, ptr, num_graphs, want_pool)


# ------------------------------------------------------------------------------------------------ dropout (+ residual)
# Masks are a function of (seed, call id, row, column, width) alone (kpgnn.h, kpgnn_dropout_desc): Philox4x32-10 keyed by the
# seed, counted by the logical element and the ordinal of the launch since seeding.  Seed and ordinal live in a per-device
# int64[3] tensor {seed, calls, ticket}; the forward kernel advances `calls` itself, so a replayed graph draws fresh masks, and
# the backward recomputes the mask from the int64[1] cell the forward left its call id in - nothing of [N,C] size is saved.
_NATIVE_DROPOUT = False    # opt-in: a captured step is slower with it than with nn.Dropout as measured
_DROP_STATE = {}      # device index -> int64[3] device tensor


def set_native_dropout(on):
    """Route training-mode dropout of fp32 device rows through kpgnn_dropout_* (True) or keep nn.Dropout (False, the default).
    Returns the previous setting."""
    global _NATIVE_DROPOUT
    prev, _NATIVE_DROPOUT = _NATIVE_DROPOUT, bool(on)
    return prev


def native_dropout():
    return _NATIVE_DROPOUT


def _drop_device(device):
    device = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)


def _signed64(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def dropout_seed(seed, device=None):
    """(seed, 0) into the device's dropout state: the next dropout launch has call id 0.  Data-parallel callers seed every
    rank differently: dropout_seed(seed + rank)."""
    device = _drop_device(device)
    host = torch.tensor([_signed64(seed), 0, 0], dtype=torch.int64)
    st = _DROP_STATE.get(device.index)
    if st is None:
        _DROP_STATE[device.index] = host.to(device)
    else:
        st.copy_(host)


def dropout_state(device=None):
    """The device's int64[3] {seed, calls, ticket}; a state never seeded starts from torch.initial_seed() at its first use.
    That first use copies from the host: it cannot happen inside a stream capture (KpgnnError) - call dropout_seed, or run one
    eager step, before capturing."""
    device = _drop_device(device)
    if device.index not in _DROP_STATE:
        if torch.cuda.is_current_stream_capturing():
            # (creating it is a host-to-device copy and an allocation outside the graph's pool)
            raise _lib.KpgnnError("the dropout state of this device does not exist yet and cannot be created inside a stream "
                                  "capture: call ops.dropout_seed(seed) (or run one eager step) before capturing")
        dropout_seed(torch.initial_seed(), device)
    return _DROP_STATE[device.index]


def dropout_params(p):
    """(thr, scale) of the mask definition, formed in double: keep iff word >= thr; kept values are multiplied by scale."""
    p = float(p)
    return min(4294967295, int(p * 4294967296.0)), 1.0 / (1.0 - p)


def dropout_mask(shape, p, seed, call, device):
    """The keep mask (bool [N,C]) of launch `call` under `seed` for rows of width C: kpgnn_dropout_mask, no call id consumed."""
    N, C = (int(s) for s in shape)
    mask = torch.empty((N, C), dtype=torch.uint8, device=device)
    _require_cuda(mask)
    d = _lib.DropoutMaskDesc()
    d.seed, d.call, d.N, d.C, d.thr, d.mask = _signed64(seed), _signed64(call), N, C, dropout_params(p)[0], mask.data_ptr()
    if N:
        _lib.launch("kpgnn_dropout_mask", mask.device, ctypes.byref(d))
    return mask.view(torch.bool)


def _dropout_launch(name, x, residual, cell, p):
    N, C = x.shape
    x = _rows_view(x, C)
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    state = dropout_state(x.device)
    d = _lib.DropoutDesc()
    d.N, d.C = N, C
    d.x, d.x_stride, d.out, d.out_stride = x.data_ptr(), x.stride(0), out.data_ptr(), C
    if residual is not None:
        residual = _rows_view(residual, C)
        d.residual, d.r_stride = residual.data_ptr(), residual.stride(0)
    d.thr, d.scale = dropout_params(p)
    d.state, d.call_io, d.ticket = state.data_ptr(), cell.data_ptr(), state.data_ptr() + 16
    d.n_dyn = dyn_ptr(N)
    _lib.launch(name, x.device, ctypes.byref(d))
    return out


class DropoutAdd(torch.autograd.Function):
    """out = dropout(x, p) (+ residual) as one kpgnn_dropout_fwd launch; the backward is one kpgnn_dropout_bwd launch that
    recomputes the mask from the saved int64[1] call cell, and the residual's gradient is the incoming one itself."""

    @staticmethod
    def forward(ctx, x, residual, p):
        cell = torch.empty(1, dtype=torch.int64, device=x.device)
        out = _dropout_launch("kpgnn_dropout_fwd", x, residual, cell, p)
        ctx.save_for_backward(cell)
        ctx.p = p
        return out

    @staticmethod
    def backward(ctx, gout):
        cell, = ctx.saved_tensors
        gx = _dropout_launch("kpgnn_dropout_bwd", gout, None, cell, ctx.p) if ctx.needs_input_grad[0] else None
        return gx, (gout if ctx.needs_input_grad[1] else None), None


def native_dropout_applies(x, p, training):
    return bool(_NATIVE_DROPOUT and training and 0.0 < p < 1.0 and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32
                and x.numel() > 0)


def dropout_add(x, p, training, residual=None):
    """F.dropout(x, p, training) (+ residual).  fp32 device rows [N,C] in training mode with 0 < p < 1 run kpgnn_dropout_fwd
    (masks: the counter-based generator above, not the framework's; rows beyond the live count of a dynamic_rows block are left
    alone); everything else - evaluation, p == 0, p == 1, other dtypes, CPU tensors, the switch off (set_native_dropout, off by default) - keeps the
    framework expression."""
    if not native_dropout_applies(x, p, training) or (
            residual is not None and not (residual.is_cuda and residual.dtype == torch.float32 and residual.shape == x.shape)):
        out = torch.nn.functional.dropout(x, p, training)
        return out if residual is None else out + residual
    if not torch.is_grad_enabled() or not (x.requires_grad or (residual is not None and residual.requires_grad)):
        cell = torch.empty(1, dtype=torch.int64, device=x.device)
        return _dropout_launch("kpgnn_dropout_fwd", x, residual, cell, p)      # no autograd node, nothing saved
    return DropoutAdd.apply(x, residual, float(p))


# ------------------------------------------------------------------------------------------------ jumping-knowledge reduce
# sum / max / softmax-weighted sum over the S = num_layer + 1 states of a body (kpgnn.h, kpgnn_jk_desc): the states are read in
# place through a pointer table, so nothing of [S,N,H] size is formed in the forward; max saves a uint8 [N,H] winner slot, softmax
# its [N,S] weights (and references to the states, which are alive anyway).
JK_MODES = {"sum": _lib.JK_SUM, "max": _lib.JK_MAX, "softmax": _lib.JK_SOFTMAX}
_NATIVE_JK = {"sum": True, "max": True, "softmax": True}


def set_native_jk(on, mode=None):
    """Route the jumping-knowledge reduce of fp32 device states through kpgnn_jk_reduce_* (True, the default) or keep the
    torch.stack expressions (False); for one mode ("sum", "max", "softmax") or, with mode=None, for all three.  Returns the
    previous setting (native_jk(mode))."""
    prev = native_jk(mode)
    for m in (JK_MODES if mode is None else (mode,)):
        if m not in JK_MODES:
            raise ValueError(f"jumping-knowledge mode must be one of {sorted(JK_MODES)}, got {m!r}")
        _NATIVE_JK[m] = bool(on)
    return prev


def native_jk(mode=None):
    return all(_NATIVE_JK.values()) if mode is None else _NATIVE_JK[mode]


def jk_native_applies(states, mode=None):
    """Every state a CUDA fp32 2-D tensor of one (non-empty) shape [N,H], 1 <= S <= 32, and the native route switched on."""
    S = len(states)
    if not (native_jk(mode) and 1 <= S <= _lib.JK_MAX_STATES):
        return False
    shape = states[0].shape
    return bool(all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == shape for t in states)
                and states[0].numel() > 0)


def _jk_desc(states, mode):
    N, H = states[0].shape
    d = _lib.JkDesc()
    d.N, d.H, d.S, d.mode = N, H, len(states), JK_MODES[mode]
    for l, t in enumerate(states):
        d.x[l] = t.data_ptr()
    d.x_stride = H
    d.n_dyn = dyn_ptr(N)
    return d


def _jk_fwd_launch(states, mode, score, save):
    """(out, arg or w or None): one kpgnn_jk_reduce_fwd launch over contiguous states; arg / w only with `save`."""
    N, H = states[0].shape
    dev = states[0].device
    out = torch.empty((N, H), dtype=torch.float32, device=dev)
    d = _jk_desc(states, mode)
    d.out, d.out_stride = out.data_ptr(), H
    kept = None
    if mode == "softmax":
        d.score = score.data_ptr()
        if save:
            kept = torch.empty((N, len(states)), dtype=torch.float32, device=dev)
            d.w = kept.data_ptr()
    elif mode == "max" and save:
        kept = torch.empty((N, H), dtype=torch.uint8, device=dev)
        d.arg = kept.data_ptr()
    _lib.launch("kpgnn_jk_reduce_fwd", dev, ctypes.byref(d))
    return out, kept


def _jk_bwd_launch(states, S, mode, kept, gout):
    """(gx [S,N,H], gscore [N,S] or None): one kpgnn_jk_reduce_bwd launch (max: `states` is only asked for its shape)."""
    N, H = gout.shape
    dev = gout.device
    gout = _rows_view(gout, H)
    gx = torch.empty((S, N, H), dtype=torch.float32, device=dev)
    if mode == "softmax":
        d = _jk_desc(states, mode)
        gscore = torch.empty((N, S), dtype=torch.float32, device=dev)
        d.w, d.gscore = kept.data_ptr(), gscore.data_ptr()
    else:
        d = _lib.JkDesc()
        d.N, d.H, d.S, d.mode, d.n_dyn = N, H, S, JK_MODES[mode], dyn_ptr(N)
        gscore = None
        d.arg = kept.data_ptr()
    d.gout, d.gout_stride, d.gx = gout.data_ptr(), gout.stride(0), gx.data_ptr()
    _lib.launch("kpgnn_jk_reduce_bwd", dev, ctypes.byref(d))
    return gx, gscore


class JKSum(torch.autograd.Function):
    """out = sum of the states in slot order (kpgnn_jk_reduce_fwd); every state's gradient is the incoming one itself."""

    @staticmethod
    def forward(ctx, *states):
        return _jk_fwd_launch(states, "sum", None, False)[0]

    @staticmethod
    def backward(ctx, gout):
        return tuple(gout if need else None for need in ctx.needs_input_grad)


class JKMax(torch.autograd.Function):
    """out = elementwise max over the states, the lowest slot winning a tie; saves the uint8 [N,H] winner slot, and the
    backward (one kpgnn_jk_reduce_bwd launch) routes gout to that slot's block of one [S,N,H] buffer, returned as views."""

    @staticmethod
    def forward(ctx, *states):
        out, arg = _jk_fwd_launch(states, "max", None, True)
        ctx.save_for_backward(arg)
        ctx.S = len(states)
        return out

    @staticmethod
    def backward(ctx, gout):
        arg, = ctx.saved_tensors
        gx, _ = _jk_bwd_launch(None, ctx.S, "max", arg, gout)
        return tuple(gx[l] if need else None for l, need in enumerate(ctx.needs_input_grad))


class JKSoftmax(torch.autograd.Function):
    """out = sum_l softmax(score)[n,l] * states[l][n,:]; saves the [N,S] weights and references to the states; the backward is
    one kpgnn_jk_reduce_bwd launch for every state's gradient (views of one [S,N,H] buffer) and the score's."""

    @staticmethod
    def forward(ctx, score, *states):
        out, w = _jk_fwd_launch(states, "softmax", score, True)
        ctx.save_for_backward(w, *states)
        return out

    @staticmethod
    def backward(ctx, gout):
        w, *states = ctx.saved_tensors
        gx, gscore = _jk_bwd_launch(states, len(states), "softmax", w, gout)
        return (gscore if ctx.needs_input_grad[0] else None,) + tuple(
            gx[l] if need else None for l, need in enumerate(ctx.needs_input_grad[1:]))


def jk_reduce(states, mode, score=None):
    """The jumping-knowledge reduce of models/GNNs.py over the list of states [N,H]: mode "sum", "max", or "softmax" with
    score [N,S] (the weighted sum of JK attention: sum_l softmax(score)[:,l,None] * states[l]).  Where jk_native_applies, one
    kpgnn_jk_reduce_fwd launch (rows beyond the live count of a dynamic_rows block are left alone) and, for max and softmax,
    one kpgnn_jk_reduce_bwd launch; everything else - CPU tensors, other dtypes, S > 32, the switch off (set_native_jk) - keeps
    the torch.stack expressions."""
    if mode not in JK_MODES:
        raise ValueError(f"jumping-knowledge mode must be one of {sorted(JK_MODES)}, got {mode!r}")
    if (mode == "softmax") != (score is not None):
        raise ValueError("jk_reduce: a score goes with mode 'softmax' and with no other")
    states = list(states)
    native = jk_native_applies(states, mode)
    if native and score is not None:
        native = score.is_cuda and score.dtype == torch.float32 and tuple(score.shape) == (states[0].shape[0], len(states))
    if not native:
        if mode == "max":
            return torch.stack(states, dim=-1).max(dim=-1).values
        if mode == "sum":
            return torch.stack(states, dim=0).sum(dim=0)
        return (torch.stack(states, dim=1) * torch.softmax(score, dim=1).unsqueeze(-1)).sum(1)
    states = [t if t.is_contiguous() else t.contiguous() for t in states]
    if score is not None:
        score = score.contiguous()
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in states + ([] if score is None else [score])):
        return _jk_fwd_launch([t.detach() for t in states], mode, score, False)[0]     # no autograd node, nothing saved
    if mode == "sum":
        return JKSum.apply(*states)
    if mode == "max":
        return JKMax.apply(*states)
    return JKSoftmax.apply(score, *states)


# ------------------------------------------------------------------------------------------------ the JK scoring LSTM
# score [N,S] of the attention readout: nn.LSTM(H, P, bidirectional) over the S states, summed over its 2P outputs (kpgnn.h,
# kpgnn_jk_lstm_desc).  The states are read in place - no torch.stack, no [N,S,H] gradient of a stack - and what the backward
# needs is one `saved` buffer in the kernels' own layout.
_NATIVE_JK_LSTM = True
_LSTM_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
                "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def set_native_jk_lstm(on):
    """Route the scoring LSTM of JK attention through kpgnn_jk_lstm_* (True, the default) or keep nn.LSTM on the stacked
    states (False).  Returns the previous setting."""
    global _NATIVE_JK_LSTM
    prev, _NATIVE_JK_LSTM = _NATIVE_JK_LSTM, bool(on)
    return prev


def native_jk_lstm():
    return _NATIVE_JK_LSTM


def jk_lstm_applies(states, lstm):
    """The states as jk_native_applies wants them (CUDA fp32 [N,H], one non-empty shape, 1 <= S <= 32) with H <= 256, and a
    one-layer, bidirectional, bias-carrying fp32 nn.LSTM(H, P <= 16) without projection on the same device; the switch on."""
    states = list(states)
    S = len(states)
    if not (_NATIVE_JK_LSTM and 1 <= S <= _lib.JK_MAX_STATES and isinstance(lstm, torch.nn.LSTM)):
        return False
    shape = states[0].shape
    if not (all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == shape for t in states)
            and states[0].numel() > 0 and shape[1] <= _lib.JK_LSTM_MAX_H):
        return False
    return _jk_lstm_module_ok(lstm, shape[1], states[0].device)


def _jk_lstm_module_ok(lstm, H, device):
    """The module half of jk_lstm_applies: one layer, bidirectional, biases, no projection, input_size H, hidden size
    1 .. 16, fp32 parameters on `device`."""
    if not (lstm.num_layers == 1 and lstm.bidirectional and lstm.bias and getattr(lstm, "proj_size", 0) == 0
            and lstm.input_size == H and 1 <= lstm.hidden_size <= _lib.JK_LSTM_MAX_P):
        return False
    return all(q.dtype == torch.float32 and q.device == device for q in (getattr(lstm, k) for k in _LSTM_PARAMS))


def _jk_lstm_desc(states, params):
    N, H = states[0].shape
    d = _lib.JkLstmDesc()
    d.N, d.H, d.P, d.S = N, H, params[1].shape[1], len(states)
    for l, t in enumerate(states):
        d.x[l] = t.data_ptr()
    d.x_stride = H
    for k in range(2):
        d.w_ih[k], d.w_hh[k] = params[4 * k].data_ptr(), params[4 * k + 1].data_ptr()
        d.b_ih[k], d.b_hh[k] = params[4 * k + 2].data_ptr(), params[4 * k + 3].data_ptr()
    d.n_dyn = dyn_ptr(N)
    return d


def _jk_lstm_workspace(d, dev):
    nbytes = _lib.load().kpgnn_jk_lstm_workspace_bytes(d.N, d.H, d.P, d.S)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    return ws


def _jk_lstm_fwd_launch(states, params, save):
    """(score [N,S], saved or None): one kpgnn_jk_lstm_fwd call over contiguous states; `saved` only with `save`."""
    dev = states[0].device
    d = _jk_lstm_desc(states, params)
    score = torch.empty((d.N, d.S), dtype=torch.float32, device=dev)
    d.score = score.data_ptr()
    saved = None
    if save:
        saved = torch.empty(_lib.load().kpgnn_jk_lstm_saved_bytes(d.N, d.H, d.P, d.S), dtype=torch.uint8, device=dev)
        d.saved = saved.data_ptr()
    ws = _jk_lstm_workspace(d, dev)
    _lib.launch("kpgnn_jk_lstm_fwd", dev, ctypes.byref(d))
    del ws
    return score, saved


class JKLstmScore(torch.autograd.Function):
    """score = nn.LSTM(states).sum(-1) (kpgnn_jk_lstm_fwd); saves `saved` and references to the states and parameters; the
    backward is one kpgnn_jk_lstm_bwd call for every state's gradient (views of one [S,N,H] buffer) and the eight parameter
    gradients (the two biases of a direction share one)."""

    @staticmethod
    def forward(ctx, *args):
        params, states = args[:8], args[8:]
        score, saved = _jk_lstm_fwd_launch(states, params, True)
        ctx.save_for_backward(saved, *args)
        return score

    @staticmethod
    def backward(ctx, gscore):
        saved, *args = ctx.saved_tensors
        params, states = args[:8], args[8:]
        dev = gscore.device
        d = _jk_lstm_desc(states, params)
        gscore = gscore.contiguous()
        d.saved, d.gscore = saved.data_ptr(), gscore.data_ptr()
        gx = None
        if any(ctx.needs_input_grad[8:]):
            gx = torch.empty((d.S, d.N, d.H), dtype=torch.float32, device=dev)
            d.gx = gx.data_ptr()
        grads = [torch.empty_like(params[4 * k + j]) for k in range(2) for j in range(3)]     # dw_ih, dw_hh, db per direction
        for k in range(2):
            d.dw_ih[k], d.dw_hh[k], d.db[k] = (g.data_ptr() for g in grads[3 * k:3 * k + 3])
        ws = _jk_lstm_workspace(d, dev)
        _lib.launch("kpgnn_jk_lstm_bwd", dev, ctypes.byref(d))
        del ws
        out = []
        for k in range(2):
            dw_ih, dw_hh, db = grads[3 * k:3 * k + 3]
            out += [dw_ih, dw_hh, db, db.clone()]         # (two leaves must not end up sharing one .grad)
        out = [g if need else None for g, need in zip(out, ctx.needs_input_grad[:8])]
        return tuple(out) + tuple(gx[l] if need else None for l, need in enumerate(ctx.needs_input_grad[8:]))


def jk_lstm_score(states, lstm):
    """score [N,S] = lstm(torch.stack(states, 1))[0].sum(-1) for the scoring LSTM of JK attention, the states read in place.
    Call it where jk_lstm_applies(states, lstm); under no_grad, or when nothing requires a gradient, the entry is launched
    directly with saved = NULL and no autograd node is made."""
    if not jk_lstm_applies(states, lstm):
        raise _lib.KpgnnError("jk_lstm_score: the native route does not apply (jk_lstm_applies); keep nn.LSTM on the stack")
    states = [t if t.is_contiguous() else t.contiguous() for t in states]
    params = [getattr(lstm, k) for k in _LSTM_PARAMS]
    params = [q if q.is_contiguous() else q.contiguous() for q in params]
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in states + params):
        return _jk_lstm_fwd_launch([t.detach() for t in states], [q.detach() for q in params], False)[0]
    return JKLstmScore.apply(*params, *states)


# ------------------------------------------------------------------------------------------------ the bodies' other norms
# norm_type "Layer", "Instance", "GraphSize", "Pair" (models/GNNs.py:103-112; kpgnn.h, kpgnn_norm_desc): PyG's modules called
# without a batch vector, so the whole batch is one graph.  None has running statistics (training and evaluation compute the
# same), and what the backward keeps besides x is a float [2C + 4] of coefficients.  A caller that does pass a batch vector
# (body_norm(..., batch=, num_graphs=); the bodies under norm_scope="graph") gets every graph normalised over its own rows:
# kpgnn_graph_norm_desc, csrc/body_norm_graph.hip.
NORM_KINDS = {"Layer": _lib.NORM_LAYER, "Instance": _lib.NORM_INSTANCE, "GraphSize": _lib.NORM_GRAPHSIZE, "Pair": _lib.NORM_PAIR}
_NATIVE_NORMS = True
# per kind, on EXACT-SHAPE batches: GraphSize is one framework launch per direction to begin with, and an eager step measured
# 0.08 - 0.12 ms slower with the native one (a captured step the same to 0.04 ms faster) - opt-in, as dropout is.  Inside a dynamic_rows
# block every kind is native whatever this says: it is the only route there.
_NATIVE_NORM_EXACT = {"Layer": True, "Instance": True, "GraphSize": False, "Pair": True}


def set_native_norms(on):
    """Route the Layer / Instance / GraphSize / Pair norms of fp32 device rows through kpgnn_body_norm_* (True, the default) or
    keep the framework expressions for all of them (False).  Returns the previous setting."""
    global _NATIVE_NORMS
    prev, _NATIVE_NORMS = _NATIVE_NORMS, bool(on)
    return prev


def native_norms():
    return _NATIVE_NORMS


def set_native_norm_exact(kind, on):
    """Whether `kind` takes the native route on EXACT-SHAPE batches too, given that the switch (set_native_norms) is on; default:
    every kind but "GraphSize".  Inside a dynamic_rows block every kind is native whatever this says.  Returns the previous
    setting of that kind."""
    if kind not in NORM_KINDS:
        raise ValueError(f"norm kind must be one of {sorted(NORM_KINDS)}, got {kind!r}")
    prev, _NATIVE_NORM_EXACT[kind] = _NATIVE_NORM_EXACT[kind], bool(on)
    return prev


def native_norm_exact(kind):
    """Whether `kind` is native on an exact-shape batch as things are set (the switch and the kind's own setting)."""
    return bool(_NATIVE_NORMS and _NATIVE_NORM_EXACT[kind])


def body_norm_applies(x):
    """fp32 device rows [N,C] with N >= 1 and 1 <= C <= 256 (what csrc/body_norm.hip covers)."""
    return bool(x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and 1 <= x.shape[1] <= _lib.NORM_MAX_C)


def _graph_norm_reference(x, kind, weight, bias, eps, batch, num_graphs):
    """The four norms per graph of `batch` (int64 [N], graph ids in [0, num_graphs)) as index_add_ sums: no loop over graphs."""
    C = x.shape[1]
    cnt = torch.zeros(num_graphs, dtype=x.dtype, device=x.device).index_add_(0, batch, torch.ones_like(x[:, 0])).clamp(min=1)

    def rows_sum(t):        # [N,C] -> [G,C]
        return torch.zeros((num_graphs, C), dtype=x.dtype, device=x.device).index_add_(0, batch, t)

    if kind == "GraphSize":
        return x / cnt.sqrt()[batch].unsqueeze(1)
    if kind == "Layer":
        nc = (cnt * C).unsqueeze(1)
        xc = x - (rows_sum(x).sum(1, keepdim=True) / nc)[batch]
        var = rows_sum(xc * xc).sum(1, keepdim=True) / nc
        pos = var > 0           # (a constant block: sd = 0 with a zero gradient, as torch.std has it, not sqrt's 0 * inf)
        sd = torch.where(pos, var, torch.ones_like(var)).sqrt() * pos
        return xc / (sd + eps)[batch] * weight + bias
    xc = x - (rows_sum(x) / cnt.unsqueeze(1))[batch]
    if kind == "Instance":
        return xc / (rows_sum(xc * xc) / cnt.unsqueeze(1) + eps).sqrt()[batch]
    return xc / (eps + rows_sum(xc * xc).sum(1, keepdim=True) / cnt.unsqueeze(1)).sqrt()[batch]      # Pair


def body_norm_reference(x, kind, weight=None, bias=None, residual=None, eps=1e-5, *, batch=None, num_graphs=None):
    """The framework expression of the four norms (any device, any floating dtype): what PyG's LayerNorm (mode "graph"),
    InstanceNorm (no affine, no running statistics), GraphSizeNorm and PairNorm (scale 1) compute without a batch vector - or,
    with `batch` (sorted graph ids [N]) and `num_graphs`, per graph."""
    if kind not in NORM_KINDS:
        raise ValueError(f"norm kind must be one of {sorted(NORM_KINDS)}, got {kind!r}")
    if batch is not None:
        if num_graphs is None:
            raise ValueError("body_norm: a batch vector needs num_graphs")
        y = _graph_norm_reference(x, kind, weight, bias, eps, batch, int(num_graphs))
        return y if residual is None else y + residual
    if kind == "Layer":
        xc = x - x.mean()
        y = xc / (xc.std(unbiased=False) + eps) * weight + bias
    elif kind == "Instance":
        y = (x - x.mean(0, keepdim=True)) / (x.var(0, unbiased=False, keepdim=True) + eps).sqrt()
    elif kind == "GraphSize":
        y = x / x.shape[0] ** 0.5
    elif kind == "Pair":
        xc = x - x.mean(0, keepdim=True)
        y = xc / (eps + xc.pow(2).sum(-1).mean()).sqrt()
    else:
        raise ValueError(f"norm kind must be one of {sorted(NORM_KINDS)}, got {kind!r}")
    return y if residual is None else y + residual


def _norm_desc(x, kind, eps, saved):
    """(descriptor, workspace): x rows the kernels can walk, the coefficient buffer and a workspace of the entry's size."""
    N, C = x.shape
    d = _lib.NormDesc()
    d.N, d.C, d.kind, d.eps = N, C, NORM_KINDS[kind], eps
    d.x, d.x_stride, d.saved = x.data_ptr(), x.stride(0), saved.data_ptr()
    nbytes = _lib.load().kpgnn_body_norm_workspace_bytes(N, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
    d.n_dyn = dyn_ptr(N)
    return d, ws


def _norm_fwd_launch(x, kind, weight, bias, residual, eps):
    """(out, saved, x as the kernels read it): one kpgnn_body_norm_fwd call."""
    N, C = x.shape
    x = _rows_view(x, C)
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    saved = torch.empty(2 * C + 4, dtype=torch.float32, device=x.device)
    d, ws = _norm_desc(x, kind, eps, saved)
    d.out, d.out_stride = out.data_ptr(), C
    if kind == "Layer":
        weight, bias = weight.contiguous(), bias.contiguous()
        d.weight, d.bias = weight.data_ptr(), bias.data_ptr()
    if residual is not None:
        residual = _rows_view(residual, C)
        d.residual, d.res_stride = residual.data_ptr(), residual.stride(0)
    _lib.launch("kpgnn_body_norm_fwd", x.device, ctypes.byref(d))
    del ws
    return out, saved, x


class BodyNorm(torch.autograd.Function):
    """out = norm(x) (+ residual): one kpgnn_body_norm_fwd call forward, one kpgnn_body_norm_bwd call backward.  Saves x (which
    autograd holds anyway; not for GraphSize), Layer's weight and the float [2C + 4] coefficients; the residual's gradient is
    the incoming one."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, kind, eps):
        out, saved, x = _norm_fwd_launch(x, kind, weight, bias, residual, eps)
        # (GraphSize's backward is gout / sqrt(n): it does not read x, so x is not kept alive for it)
        ctx.save_for_backward(*(() if kind == "GraphSize" else (x,)), saved, *(() if weight is None else (weight,)))
        ctx.kind, ctx.eps = kind, eps
        return out

    @staticmethod
    def backward(ctx, gout):
        N, C = gout.shape
        gout_rows = _rows_view(gout, C)
        if ctx.kind == "GraphSize":
            (saved,), x, w = ctx.saved_tensors, gout_rows, []       # (the descriptor wants some x; this kind never reads it)
        else:
            x, saved, *w = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        gx = gw = gb = None
        if need_x or need_w or need_b:
            d, ws = _norm_desc(x, ctx.kind, ctx.eps, saved)
            gx = torch.empty((N, C), dtype=torch.float32, device=x.device)
            d.gout, d.gout_stride, d.gx, d.gx_stride = gout_rows.data_ptr(), gout_rows.stride(0), gx.data_ptr(), C
            if w:
                weight = w[0].contiguous()
                gw, gb = torch.empty_like(weight), torch.empty_like(weight)
                d.weight, d.gweight, d.gbias = weight.data_ptr(), gw.data_ptr(), gb.data_ptr()
            _lib.launch("kpgnn_body_norm_bwd", x.device, ctypes.byref(d))
            del ws
        return (gx if need_x else None, gw if need_w else None, gb if need_b else None, gout if need_r else None, None, None)


def _graph_norm_desc(x, kind, eps, ptr, num_graphs):
    N, C = x.shape
    d = _lib.GraphNormDesc()
    d.N, d.C, d.kind, d.eps = N, C, NORM_KINDS[kind], eps
    d.x, d.x_stride = x.data_ptr(), x.stride(0)
    d.graph_ptr, d.G = ptr.data_ptr(), num_graphs
    d.n_dyn = dyn_ptr(N)
    return d


def _graph_norm_fwd_launch(x, kind, weight, bias, residual, eps, ptr, num_graphs):
    """(out, x as the kernel reads it): one kpgnn_graph_norm_fwd call."""
    N, C = x.shape
    x = _rows_view(x, C)
    out = torch.empty((N, C), dtype=torch.float32, device=x.device)
    d = _graph_norm_desc(x, kind, eps, ptr, num_graphs)
    d.out, d.out_stride = out.data_ptr(), C
    if kind == "Layer":
        weight, bias = weight.contiguous(), bias.contiguous()
        d.weight, d.bias = weight.data_ptr(), bias.data_ptr()
    if residual is not None:
        residual = _rows_view(residual, C)
        d.residual, d.res_stride = residual.data_ptr(), residual.stride(0)
    _lib.launch("kpgnn_graph_norm_fwd", x.device, ctypes.byref(d))
    return out, x


class GraphBodyNorm(torch.autograd.Function):
    """out = norm per graph (x) (+ residual): one kpgnn_graph_norm_fwd call forward, one kpgnn_graph_norm_bwd call backward.
    Saves x (not for GraphSize), the graph pointer and Layer's weight - the backward recomputes the statistics (kpgnn.h says
    why); the residual's gradient is the incoming one."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, kind, eps, ptr, num_graphs):
        out, x = _graph_norm_fwd_launch(x, kind, weight, bias, residual, eps, ptr, num_graphs)
        ctx.save_for_backward(ptr, *(() if kind == "GraphSize" else (x,)), *(() if weight is None else (weight,)))
        ctx.kind, ctx.eps, ctx.num_graphs = kind, eps, num_graphs
        return out

    @staticmethod
    def backward(ctx, gout):
        N, C = gout.shape
        gout_rows = _rows_view(gout, C)
        if ctx.kind == "GraphSize":
            (ptr,), x, w = ctx.saved_tensors, gout_rows, []     # (the descriptor wants some x; this kind never reads it)
        else:
            ptr, x, *w = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        gx = gw = gb = None
        if need_x or need_w or need_b:
            d = _graph_norm_desc(x, ctx.kind, ctx.eps, ptr, ctx.num_graphs)
            # (rows beyond the live count of a dynamic_rows block are never written: whoever reads gx there skips them too)
            gx = torch.empty((N, C), dtype=torch.float32, device=x.device)
            d.gout, d.gout_stride, d.gx, d.gx_stride = gout_rows.data_ptr(), gout_rows.stride(0), gx.data_ptr(), C
            ws = None
            if w:
                weight = w[0].contiguous()
                d.weight = weight.data_ptr()
                if need_w or need_b:
                    gw, gb = torch.empty_like(weight), torch.empty_like(weight)
                    nbytes = _lib.load().kpgnn_graph_norm_workspace_bytes(N, ctx.num_graphs, C, d.kind)
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
                    d.gweight, d.gbias, d.workspace, d.workspace_bytes = gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), nbytes
            _lib.launch("kpgnn_graph_norm_bwd", x.device, ctypes.byref(d))
            del ws
        return (gx if need_x else None, gw if need_w else None, gb if need_b else None, gout if need_r else None,
                None, None, None, None)


def body_norm(x, kind, weight=None, bias=None, residual=None, eps=1e-5, *, batch=None, num_graphs=None):
    """The Layer / Instance / GraphSize / Pair norm of the bodies over the rows x [N,C] (+ residual); weight / bias [C] go with
    "Layer" and with no other kind.

    With `batch` (the sorted graph ids [N] of a collated batch) and `num_graphs` every graph is normalised on its own rows
    (kpgnn.h, kpgnn_graph_norm_desc): a graph's result does not depend on what else is in the batch.  Where body_norm_applies and
    set_native_norms is on - every kind, exact-shape batches included - that is one kpgnn_graph_norm_fwd call and one
    kpgnn_graph_norm_bwd call; graph_ptr_of(batch, num_graphs) supplies the pointer, so the batch vector needs one eager use
    before a capture.  Everything else keeps the framework expression (body_norm_reference), which has no dynamic row count.

    Without `batch` the whole batch is one graph, as the reference's bodies have it.  Where body_norm_applies and the switch is on
    (set_native_norms; "GraphSize" on exact-shape batches only after set_native_norm_exact("GraphSize", True), inside a dynamic_rows
    block always), one kpgnn_body_norm_fwd call and one kpgnn_body_norm_bwd call - the statistics are over the LIVE rows of
    a dynamic_rows block, and rows beyond them are left alone; under no_grad, or when nothing requires a gradient, no autograd
    node is made.  Everything else - CPU tensors, other dtypes, C > 256, the switch off - keeps the framework expression
    (body_norm_reference), which has no dynamic row count."""
    if kind not in NORM_KINDS:
        raise ValueError(f"norm kind must be one of {sorted(NORM_KINDS)}, got {kind!r}")
    if (kind == "Layer") != (weight is not None and bias is not None) or (kind != "Layer" and (weight is not None or bias is not None)):
        raise ValueError("body_norm: weight and bias go with kind 'Layer' and with no other")
    per_graph = batch is not None
    if per_graph and num_graphs is None:
        raise ValueError("body_norm: a batch vector needs num_graphs")
    native = _NATIVE_NORMS and body_norm_applies(x) and (per_graph or _NATIVE_NORM_EXACT[kind] or dyn_ptr(x.shape[0]) is not None)
    for t in (weight, bias):
        native = native and (t is None or (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (x.shape[1],)))
    native = native and (residual is None or (residual.is_cuda and residual.dtype == torch.float32 and residual.shape == x.shape))
    if not native:
        if x.dim() == 2:
            refuse_dynamic_rows(f"the framework expression of the {kind} norm", x.shape[0])
        return body_norm_reference(x, kind, weight, bias, residual, eps, batch=batch, num_graphs=num_graphs)
    eps = float(eps)
    if per_graph:
        num_graphs = int(num_graphs)
        if batch.shape[0] != x.shape[0]:
            raise ValueError(f"body_norm: batch names {batch.shape[0]} rows, x has {x.shape[0]}")
        ptr = graph_ptr_of(batch, num_graphs)
        if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (x, weight, bias, residual)):
            return _graph_norm_fwd_launch(x.detach(), kind, weight, bias, residual, eps, ptr, num_graphs)[0]
        return GraphBodyNorm.apply(x, weight, bias, residual, kind, eps, ptr, num_graphs)
    if not torch.is_grad_enabled() or not any(t is not None and t.requires_grad for t in (x, weight, bias, residual)):
        return _norm_fwd_launch(x.detach(), kind, weight, bias, residual, eps)[0]      # no autograd node, nothing saved
    return BodyNorm.apply(x, weight, bias, residual, kind, eps)


# ------------------------------------------------------------------------------------------------ the rd projection
# x + rd_projection(rd) of the bodies (models/GNNs.py; kpgnn.h, kpgnn_rd_proj_desc): one launch forward; backward dx is the
# incoming gradient and dw / db are two launches of double partial sums over the LIVE rows - the framework's Linear(1, H)
# sums its weight and bias gradients over every row of a capacity-shaped batch, uninitialised dead ones included.
_NATIVE_RD_PROJ = True


def set_native_rd_proj(on):
    """Route the bodies' rd projection of fp32 device rows through kpgnn_rd_proj_* (True) or keep the framework expression
    x + Linear(rd) on exact-shape batches (False).  Inside a dynamic_rows block it is native whatever this says: it is the
    only route there.  Returns the previous setting."""
    global _NATIVE_RD_PROJ
    prev, _NATIVE_RD_PROJ = _NATIVE_RD_PROJ, bool(on)
    return prev


def native_rd_proj():
    return _NATIVE_RD_PROJ


def _rd_proj_covers(x, rd, w, b):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and 1 <= x.shape[1] <= _lib.RD_PROJ_MAX_H):
        return False
    N, H = x.shape
    ok = rd.is_cuda and rd.dtype == torch.float32 and rd.dim() in (1, 2) and rd.numel() == N and not rd.requires_grad
    ok = ok and w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == (H, 1)
    return bool(ok and b is not None and b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == (H,))


def rd_project_applies(x, rd, w, b):
    """Whether rd_project takes the native route: fp32 device rows x [N,H] with N >= 1 and H <= 256, rd [N,1] or [N] without
    a gradient of its own, w [H,1], b [H] - and the switch is on or a dynamic_rows block over N rows is active."""
    return _rd_proj_covers(x, rd, w, b) and (_NATIVE_RD_PROJ or dyn_ptr(x.shape[0]) is not None)


def rd_project_reference(x, rd, w, b):
    """The framework expression x + Linear(rd) evaluated in float64 (any device): what the tests hold the kernels to."""
    return x.double() + torch.nn.functional.linear(rd.double().reshape(-1, 1), w.double(), b.double())


def _rd_proj_fwd_launch(x, rd, w, b):
    N, H = x.shape
    x = _rows_view(x, H)
    out = torch.empty((N, H), dtype=torch.float32, device=x.device)
    w, b = w.reshape(-1).contiguous(), b.contiguous()
    d = _lib.RdProjDesc()
    d.N, d.H, d.n_dyn = N, H, dyn_ptr(N)
    d.x, d.x_stride, d.rd, d.w, d.b, d.out, d.out_stride = x.data_ptr(), x.stride(0), rd.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), H
    _lib.launch("kpgnn_rd_proj_fwd", x.device, ctypes.byref(d))
    return out


class RdProject(torch.autograd.Function):
    """out = x + rd w^T + b (kpgnn_rd_proj_fwd); backward: x gets the incoming gradient itself, w and b theirs from one
    kpgnn_rd_proj_bwd call (live rows only, no atomics).  Only rd is kept."""

    @staticmethod
    def forward(ctx, x, rd, w, b):
        rd = rd.reshape(-1).contiguous()
        ctx.save_for_backward(rd)
        return _rd_proj_fwd_launch(x, rd, w, b)

    @staticmethod
    def backward(ctx, gout):
        (rd,) = ctx.saved_tensors
        N, H = gout.shape
        need_x, _, need_w, need_b = ctx.needs_input_grad
        dw = db = None
        if need_w or need_b:
            dy = _rows_view(gout, H)
            dw = torch.empty((H, 1), dtype=torch.float32, device=gout.device)
            db = torch.empty(H, dtype=torch.float32, device=gout.device)
            nbytes = _lib.load().kpgnn_rd_proj_workspace_bytes(N, H)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=gout.device)
            d = _lib.RdProjDesc()
            d.N, d.H, d.n_dyn = N, H, dyn_ptr(N)
            d.rd, d.dy, d.dy_stride, d.dw, d.db = rd.data_ptr(), dy.data_ptr(), dy.stride(0), dw.data_ptr(), db.data_ptr()
            d.workspace, d.workspace_bytes = ws.data_ptr(), nbytes
            _lib.launch("kpgnn_rd_proj_bwd", gout.device, ctypes.byref(d))
            del ws
        return gout if need_x else None, None, dw if need_w else None, db if need_b else None


def rd_project(x, rd, w, b):
    """x + rd_projection(rd) for the Linear(1, H) parameters w [H,1], b [H].  Where rd_project_applies: one kpgnn_rd_proj_fwd
    launch, live rows only inside a dynamic_rows block (rows beyond them are left alone).  Everything else - CPU tensors,
    other dtypes, H > 256, the switch off - keeps the framework expression, which has no dynamic row count and refuses one."""
    if not rd_project_applies(x, rd, w, b):
        if x.is_cuda and x.dim() == 2:
            refuse_dynamic_rows("the framework expression of the rd projection", x.shape[0])
        return x + torch.nn.functional.linear(rd, w, b).squeeze()
    if not torch.is_grad_enabled() or not any(t.requires_grad for t in (x, w, b)):
        return _rd_proj_fwd_launch(x.detach(), rd.reshape(-1).contiguous(), w, b)
    return RdProject.apply(x, rd, w, b)


class AttentionPool(torch.autograd.Function):
    """PyG's AttentionalAggregation(gate_nn=nn.Linear(D, 1)) over the node ranges of a collated batch (kpgnn_attn_pool_*):
    one launch forward, one plus a fixed-order reduce backward, no atomics."""

    @staticmethod
    def forward(ctx, x, weight, bias, ptr, num_graphs):
        x = _last_contig(x)
        N, D = x.shape
        w = weight.reshape(-1).contiguous()
        if w.numel() != D:           # the kernel reads D gate weights
            raise _lib.KpgnnError(f"attention_pool: x has {D} columns, the gate weight {w.numel()}")
        out = torch.empty((num_graphs, D), dtype=torch.float32, device=x.device)
        alpha = torch.empty((N,), dtype=torch.float32, device=x.device)
        d = _lib.AttnPoolDesc()
        d.N, d.G, d.D = N, num_graphs, D
        d.n_dyn = dyn_ptr(N)
        d.graph_ptr, d.x, d.x_stride, d.w, d.bias = ptr.data_ptr(), x.data_ptr(), x.stride(0), w.data_ptr(), _ptr(bias)
        d.alpha, d.out = alpha.data_ptr(), out.data_ptr()
        _lib.launch("kpgnn_attn_pool_fwd", x.device, ctypes.byref(d))
        ctx.save_for_backward(x, w, ptr, alpha, out)
        ctx.has_bias = bias is not None
        ctx.wshape = weight.shape
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, gout, _galpha):
        x, w, ptr, alpha, out = ctx.saved_tensors
        N, D = x.shape
        G = out.shape[0]
        dev = x.device
        gout = gout.contiguous()
        gx = torch.empty((N, D), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty((D,), dtype=torch.float32, device=dev)
        db = torch.empty((1,), dtype=torch.float32, device=dev) if ctx.has_bias else None
        nb = int(_lib.load().kpgnn_attn_pool_workspace_bytes(G, D))
        ws = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev)
        d = _lib.AttnPoolDesc()
        d.N, d.G, d.D = N, G, D
        d.n_dyn = dyn_ptr(N)
        d.graph_ptr, d.x, d.x_stride, d.w = ptr.data_ptr(), x.data_ptr(), x.stride(0), w.data_ptr()
        d.alpha, d.out, d.gout = alpha.data_ptr(), out.data_ptr(), gout.data_ptr()
        d.gx, d.gx_stride, d.dw, d.db = _ptr(gx), D, dw.data_ptr(), _ptr(db)
        d.workspace, d.workspace_bytes = ws.data_ptr(), nb
        _lib.launch("kpgnn_attn_pool_bwd", dev, ctypes.byref(d))
        return gx, dw.view(ctx.wshape), db, None, None


def attention_pool_reference(x, batch, num_graphs, gate_lin):
    """The framework formulation (any device / dtype): softmax of gate_lin(x) within each graph, then the weighted sum."""
    gate = gate_lin(x).reshape(-1)
    idx = batch.long()
    mx = gate.new_full((num_graphs,), float("-inf")).scatter_reduce(0, idx, gate.detach(), reduce="amax")
    e = (gate - mx[idx]).exp()
    alpha = e / (gate.new_zeros(num_graphs).index_add_(0, idx, e)[idx] + 1e-16)
    return x.new_zeros((num_graphs, x.shape[1])).index_add_(0, idx, alpha.unsqueeze(-1) * x)


def attention_pool(x, batch, num_graphs, gate_lin, return_alpha=False):
    """AttentionalAggregation(gate_nn=gate_lin)(x, batch): out[g] = sum_n softmax_g(gate_lin(x))[n] x[n].  fp32 device rows up to
    256 floats wide take the HIP kernels; anything else the framework formulation."""
    if (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.shape[1] <= 256 and gate_lin.out_features == 1
            and gate_lin.in_features == x.shape[1] and gate_lin.weight.dtype == torch.float32):
        # (a width mismatch goes to the framework formulation below, whose gate_lin(x) raises the framework's shape error)
        b = batch.long() if batch.dtype != torch.int64 else batch
        out, alpha = AttentionPool.apply(x, gate_lin.weight, gate_lin.bias, graph_ptr_of(b, num_graphs), num_graphs)
        return (out, alpha) if return_alpha else out
    assert not return_alpha
    refuse_dynamic_rows("attention readout on the framework path", x.shape[0])
    return attention_pool_reference(x, batch, num_graphs, gate_lin)


# ------------------------------------------------------------------------------------------------ projected tables
class EncTables(torch.autograd.Function):
    """(table [R,H], bias [H]) of the projected peripheral-feature tables (kpgnn_enc_tables_*): for encoder e with
    components c:  table[rows of c] = squash(gate_e) * Emb_c.weight @ W_e[:, cH:(c+1)H]^T,  bias = sum_e squash(gate_e) *
    mult_e * b_e.  One launch per direction.  Arguments: squash kind (0 sigmoid / 1 tanh), the encoders' multiplicities and
    component counts, then per encoder (proj.weight, proj.bias, gate) and the embedding weights encoder by encoder."""

    @staticmethod
    def forward(ctx, squash, mults, ncomps, *tensors):
        ne = len(ncomps)
        enc_t, embs = tensors[:3 * ne], tensors[3 * ne:]
        _require_cuda(*tensors)
        H = embs[0].shape[1]
        dev = embs[0].device
        embs = [e.contiguous() for e in embs]
        enc_t = [t.contiguous() for t in enc_t]
        R = sum(e.shape[0] for e in embs)
        out = torch.empty((2, R, H), dtype=torch.float32, device=dev)       # table, pre
        bias = torch.empty((H,), dtype=torch.float32, device=dev)
        d = EncTables._desc(squash, mults, ncomps, enc_t, embs, H)
        d.table, d.pre, d.bias = out[0].data_ptr(), out[1].data_ptr(), bias.data_ptr()
        _lib.launch("kpgnn_enc_tables_fwd", dev, ctypes.byref(d))
        ctx.save_for_backward(out, *enc_t, *embs)
        ctx.meta = (squash, tuple(mults), tuple(ncomps), H)
        return out[0], bias

    @staticmethod
    def _desc(squash, mults, ncomps, enc_t, embs, H):
        d = _lib.EncTablesDesc()
        d.H, d.num_components, d.num_encoders = H, len(embs), len(ncomps)
        c = 0
        for e, n in enumerate(ncomps):
            w, b, gate = enc_t[3 * e:3 * e + 3]
            assert tuple(w.shape) == (H, n * H) and b.numel() == H and gate.numel() == 1
            d.enc_w[e], d.enc_b[e], d.enc_gate[e] = w.data_ptr(), b.data_ptr(), gate.data_ptr()
            d.enc_mult[e], d.enc_squash[e] = float(mults[e]), int(squash)
            for _ in range(n):
                assert embs[c].shape[1] == H
                d.comp_emb[c], d.comp_rows[c], d.comp_encoder[c] = embs[c].data_ptr(), embs[c].shape[0], e
                c += 1
        assert c == len(embs)
        return d

    @staticmethod
    def backward(ctx, gtable, gbias):
        out, *rest = ctx.saved_tensors
        squash, mults, ncomps, H = ctx.meta
        ne = len(ncomps)
        enc_t, embs = rest[:3 * ne], rest[3 * ne:]
        dev = out.device
        gtable = gtable.contiguous() if gtable is not None else torch.zeros_like(out[0])
        gbias = gbias.contiguous() if gbias is not None else torch.zeros(H, dtype=torch.float32, device=dev)
        d = EncTables._desc(squash, mults, ncomps, enc_t, embs, H)
        d.pre, d.gtable, d.gbias = out[1].data_ptr(), gtable.data_ptr(), gbias.data_ptr()
        g_enc = []
        for e in range(ne):
            gw, gb, gg = torch.empty_like(enc_t[3 * e]), torch.empty_like(enc_t[3 * e + 1]), torch.empty_like(enc_t[3 * e + 2])
            d.enc_gw[e], d.enc_gb[e], d.enc_ggate[e] = gw.data_ptr(), gb.data_ptr(), gg.data_ptr()
            g_enc += [gw, gb, gg]
        g_emb = [torch.empty_like(e) for e in embs]
        for c, g in enumerate(g_emb):
            d.comp_gemb[c] = g.data_ptr()
        _lib.launch("kpgnn_enc_tables_bwd", dev, ctypes.byref(d))
        return (None, None, None, *g_enc, *g_emb)


def enc_tables(squash, encoders):
    """encoders: list of (proj_weight [H, C*H], proj_bias [H], gate_raw [1], multiplicity, [Emb_c.weight ...]).
    Returns (table [R,H], bias [H])."""
    mults = [m for (_, _, _, m, _) in encoders]
    ncomps = [len(embs) for (_, _, _, _, embs) in encoders]
    enc_t = [t for (w, b, g, _, _) in encoders for t in (w, b, g)]
    embs = [e for (_, _, _, _, es) in encoders for e in es]
    return EncTables.apply(squash, mults, ncomps, *enc_t, *embs)


# ------------------------------------------------------------------------------------------------ embedding collisions
# The result of the regular-graph simulation (run_simulation.py:165-178): how many pairs of rows of an [N,D] matrix lie within
# sqrt(eps) of each other.  Device fp32 rows of up to 256 columns take kpgnn_collision_count (two launches, 64-bit counts, the
# pair matrix never exists); everything else takes the same count as a blocked framework expression.
_NATIVE_COLLISIONS = True
_COLLISION_BLOCK = 2048        # rows of a block of the framework expression: one [2048, 2048] fp32 block of pairs at a time


def set_native_collisions(on):
    """Route collision_count of fp32 device rows with D <= 256 through kpgnn_collision_count (True) or keep the blocked framework
    expression (False).  Returns the previous setting."""
    global _NATIVE_COLLISIONS
    prev, _NATIVE_COLLISIONS = _NATIVE_COLLISIONS, bool(on)
    return prev


def native_collisions():
    return _NATIVE_COLLISIONS


def collision_count_applies(outputs):
    """Whether collision_count takes the native route: the switch is on and `outputs` is a device fp32 [N,D] tensor, D <= 256."""
    return bool(_NATIVE_COLLISIONS and outputs.is_cuda and outputs.dtype == torch.float32 and outputs.dim() == 2
                and 1 <= outputs.shape[1] <= _lib.COLLISION_MAX_D)


def collision_count_reference(outputs, epsilon=1e-10, block=None):
    """(upper, diag) as 0-dim int64 tensors on the device of `outputs`, by the framework expression on blocks of `block` rows:
    d2 accumulates (a[:, d, None] - b[None, :, d])^2 over d in fp32 for one block of pairs at a time (the reference's
    [N, D, N] tensor never exists), d2 < epsilon is counted above the diagonal and on it.  Subtract, square and add are rounded
    separately, 3u per term and (D - 1)u for the sum with u = 2^-24: inside the same band as the kernel (csrc/collisions.hip)."""
    block = int(block or _COLLISION_BLOCK)
    o = outputs.detach().to(torch.float32)
    N, D = o.shape
    upper = torch.zeros((), dtype=torch.int64, device=o.device)
    diag = torch.zeros((), dtype=torch.int64, device=o.device)
    for i0 in range(0, N, block):
        a = o[i0:i0 + block]
        for j0 in range(i0, N, block):
            b = o[j0:j0 + block]
            d2 = torch.zeros((a.shape[0], b.shape[0]), dtype=torch.float32, device=o.device)
            for d in range(D):
                diff = a[:, d, None] - b[None, :, d]
                d2 += diff * diff
            hit = d2 < epsilon
            if i0 == j0:
                upper += torch.triu(hit, diagonal=1).sum()
                diag += hit.diagonal().sum()
            else:
                upper += hit.sum()
    return upper, diag


def _collision_count_launch(o, epsilon):
    """int64[2] device tensor (upper, diag) of fp32 device rows o [N,D], N >= 1: one kpgnn_collision_count call (two launches).
    A strided o with unit column stride is read in place."""
    N, D = o.shape
    o = _rows_view(o, D)
    out = torch.empty(2, dtype=torch.int64, device=o.device)
    nbytes = _lib.load().kpgnn_collision_workspace_bytes(N)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=o.device)
    d = _lib.CollisionDesc()
    d.N, d.D, d.eps = N, D, float(epsilon)
    d.x, d.x_stride, d.out, d.workspace, d.workspace_bytes = o.data_ptr(), o.stride(0), out.data_ptr(), ws.data_ptr(), nbytes
    _lib.launch("kpgnn_collision_count", o.device, ctypes.byref(d))
    return out


def collision_count(outputs, epsilon=1e-10):
    """(upper, diag) as Python ints for the rows of `outputs` [N,D]: upper = #{i < j : d2(i,j) < epsilon}, diag = #{i : d2(i,i) <
    epsilon} with d2 the squared distance in fp32 and epsilon compared as fp32 (run_simulation.py:166-173, whose count
    (diff < epsilon).sum() is 2 * upper + diag).  One read-back.  Where collision_count_applies: kpgnn_collision_count.
    Everything else - CPU tensors, other dtypes (cast to fp32), D > 256, the switch off - takes collision_count_reference."""
    if outputs.dim() != 2:
        raise ValueError(f"collision_count needs an [N,D] matrix, got {tuple(outputs.shape)}")
    N = outputs.shape[0]
    if N == 0:
        return 0, 0
    if N >= 2 and collision_count_applies(outputs):
        both = _collision_count_launch(outputs.detach(), epsilon)
    else:                                       # (a single row has only its diagonal: no launch of ours for it)
        both = torch.stack(collision_count_reference(outputs, epsilon))
    upper, diag = both.tolist()
    return int(upper), int(diag)
