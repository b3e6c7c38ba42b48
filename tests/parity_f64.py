"""Helpers of the float64 parity tests (tests/test_oracle_golden.py, tests/test_gpu_parity.py, tests/golden/make_golden.py):
the seeded body the large-batch tests share, the oracle evaluated in a given dtype, the fp32 yardstick runs at fixed thread
counts, and the one comparison every large-batch check goes through (close_to_f64).  No GPU is touched here."""
import hashlib

import torch

RTOL = 1e-4    # the golden tests' tolerances (tests/test_gpu_parity.py)
ATOL = 1e-5
THREADS = (4, 8, 16)      # thread counts of the fp32 yardstick runs; a one-thread run is up to 50 times looser and is NOT among them

BODY_KIND = {"KPGINPlus": ("GNNPlus", "KPGINPlus"), "KPGIN": ("GNN", "KPGIN")}


def small_body(model_name, combine, K, L, H):
    """The seeded (torch.manual_seed(3)) body + regression head the hipGraph and large-batch tests build, on the CPU."""
    import argparse
    from kp_gnn_amd import body as B
    from kp_gnn_amd.layers import make_gnn_layer
    ns = argparse.Namespace(model_name=model_name, hidden_size=H, K=K, num_layer=L, num_hop1_edge=3, max_pe_num=50,
                            combine=combine, eps=0., train_eps=False, aggr="add")
    torch.manual_seed(3)
    gnn = B.make_GNN(ns)(num_layer=L, gnn_layer=make_gnn_layer(ns), JK="concat", norm_type="Batch",
                         init_emb=B.EmbeddingEncoder(21, H), residual=True, virtual_node=False, use_rd=False,
                         num_hop1_edge=3, max_edge_count=50, max_hop_num=6, max_distance_count=50, drop_prob=0.0)
    return B.GraphRegression(gnn, "sum")


def tensors_sha256(*dicts):
    """sha256 over the tensors of the given dicts (key, dtype, shape, bytes; keys in sorted order): tells 'the inputs drifted'
    from 'the results differ'."""
    h = hashlib.sha256()
    for d in dicts:
        for k in sorted(d):
            t = d[k].detach().cpu().contiguous()
            h.update(f"{k}|{t.dtype}|{tuple(t.shape)}|".encode())
            h.update(t.numpy().tobytes())
    return h.hexdigest()


def to_dtype(d, dtype):
    """Floating tensors of a dict (or one tensor) cast to dtype; integer ones untouched."""
    if torch.is_tensor(d):
        return d.to(dtype) if d.is_floating_point() else d
    return {k: to_dtype(v, dtype) for k, v in d.items()}


def trainable(k, v):
    return v.is_floating_point() and "running" not in k and not k.endswith(".eps")


def oracle_body(sd, data, y, dtype, *, model_name, combine, K, L, threads=None):
    """The CPU oracle of one body (forward, L1 loss, backward) with every floating tensor in `dtype`, at `threads` torch
    threads (restored afterwards).  Returns (score, loss, {parameter name: gradient}), detached, in `dtype`; a trainable
    parameter the loss does not reach gets a zero gradient."""
    from oracle import kp_model_oracle as MO
    kind, layer_kind = BODY_KIND[model_name]
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        p = {k: (v.detach().to(dtype).clone().requires_grad_(True) if trainable(k, v) else to_dtype(v.detach(), dtype).clone())
             for k, v in sd.items()}
        score = MO.graph_regression_forward(p, data, kind=kind, layer_kind=layer_kind, K=K, num_layer=L, combine_kind=combine,
                                            JK="concat", residual=True, training=True)
        loss = (score.squeeze() - y.to(dtype).squeeze()).abs().mean()
        loss.backward()
    finally:
        torch.set_num_threads(before)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in p.items() if v.requires_grad}
    assert score.dtype == dtype and loss.dtype == dtype and all(g.dtype == dtype for g in grads.values())
    return score.detach(), loss.detach(), grads


def oracle_f64_and_f32(sd, data, y, **kw):
    """(float64 oracle result, [fp32 oracle result at 4, 8 and 16 threads])."""
    ref64 = oracle_body(sd, data, y, torch.float64, **kw)
    ref32 = [oracle_body(sd, data, y, torch.float32, threads=t, **kw) for t in THREADS]
    return ref64, ref32


def _maxabs(t):
    return float(t.abs().max()) if t.numel() else 0.0


def close_to_f64(got, ref64, ref32, name, M, cap=None):
    """`got` against the float64 reference `ref64`, with the fp32 CPU oracle's own distance from it as the yardstick.
    got / ref64: a dict of tensors (parameter gradients) or one tensor (score, loss); ref32: a list of the same, one per fp32
    run (THREADS).  Per tensor k, errors max-abs against ref64:

        e32_k   = max over the fp32 runs of |ref32_k - ref64_k|
        E32     = max_k e32_k
        yard_k  = M * max(e32_k, 0.1 * E32)
        floor_k = ATOL * max(|ref64_k|_max, 0.1 * gscale) + RTOL * |ref64_k|        (gscale = max_k |ref64_k|_max)
        assert |got_k - ref64_k| <= max(yard_k, floor_k)                             (elementwise for the RTOL term)

    No tensor is exempt: an analytically-zero gradient has ref64_k ~ 1e-16 and is bounded by yard_k like any other.
    cap(k, ref64_k, gscale) may return an elementwise bound that applies where it is smaller (printed when it binds).
    Returns {k: |got_k - ref64_k|_max / max(e32_k, 0.1 * E32)} with "E32/gscale" added under the key "".  The code under test
    never enters the yardstick."""
    single = torch.is_tensor(ref64)
    if single:
        got, ref64, ref32 = {name: got}, {name: ref64}, [{name: r} for r in ref32]
    assert sorted(got) == sorted(ref64), (name, sorted(set(got) ^ set(ref64)))
    assert len(ref32) >= 1 and all(sorted(r) == sorted(ref64) for r in ref32), name
    ref64 = {k: v.detach().cpu().double() for k, v in ref64.items()}
    e32 = {k: max(_maxabs(r[k].detach().cpu().double().reshape(v.shape) - v) for r in ref32) for k, v in ref64.items()}
    E32 = max(e32.values())
    gscale = max(_maxabs(v) for v in ref64.values())
    ratios, bad = {}, []
    for k, ref in ref64.items():
        g = got[k].detach().cpu().double()
        assert g.numel() == ref.numel(), (name, k, tuple(g.shape), tuple(ref.shape))
        err = (g.reshape(ref.shape) - ref).abs()
        unit = max(e32[k], 0.1 * E32)
        ratios[k] = _maxabs(err) / unit if unit > 0 else (0.0 if _maxabs(err) == 0 else float("inf"))
        bound = torch.clamp(ATOL * max(_maxabs(ref), 0.1 * gscale) + RTOL * ref.abs(), min=M * unit)
        if cap is not None:
            c = cap(k, ref, gscale)
            if c is not None:
                if bool((c < bound).any()):
                    print(f"[close_to_f64] {name}: {k}: the cap binds ({float(c.min()):.3e} < {float(bound.max()):.3e})")
                bound = torch.minimum(bound, c)
        if err.numel() and bool((err > bound).any()):
            bad.append((name, k, f"err {_maxabs(err):.3e}", f"e32_k {e32[k]:.3e}", f"E32 {E32:.3e}", f"gscale {gscale:.3e}",
                        f"ratio {ratios[k]:.2f}", f"M {M}"))
    assert not bad, bad
    ratios[""] = E32 / gscale if gscale > 0 else 0.0
    return ratios


def print_ratios(name, ratios, top=4):
    """One line per case for the record: E32 / gscale and the largest |got - ref64| / max(e32_k, 0.1 E32)."""
    body = {k: v for k, v in ratios.items() if k != ""}
    worst = sorted(body.items(), key=lambda kv: -kv[1])[:top]
    print(f"[f64-parity] {name}: E32/gscale {ratios['']:.3e}  max ratio {max(body.values()):.3f}  "
          + "  ".join(f"{k}={v:.3f}" for k, v in worst))
