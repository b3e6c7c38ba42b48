"""CPU: the oracle restatements (oracle/) against the golden vectors produced by the reference's own
files (tests/golden/make_golden.py).  Integer pre-transform: bit-exact.  Layers: fp32, rtol 1e-5."""
import os

import numpy as np
import pytest
import torch

from oracle import khop_oracle, kp_layers_oracle as LO

RTOL, ATOL = 1e-5, 2e-6


def _close(a, b, name, rtol=RTOL, atol=ATOL):
    assert a.shape == b.shape, (name, a.shape, b.shape)
    b = b.to(a.dtype)              # (the float64 runs: the reference's stored fp32 result, widened)
    scale = max(1.0, float(b.abs().max()))
    assert torch.allclose(a, b, rtol=rtol, atol=atol * scale), (name, float((a - b).abs().max()), scale)


# ----------------------------------------------------------------------------- pre-transform (integer, bit-exact)
def _khop_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "khop_preprocess.npz"))
    return z, sorted({k.split("/in/")[0] for k in z.files if "/in/" in k})


def test_khop_oracle_bit_exact(golden_dir):
    z, cases = _khop_cases(golden_dir)
    assert len(cases) >= 30
    for c in cases:
        a = z["args/" + c.split("/")[0]]
        args = [int(v) for v in a[:6]] + [str(a[6])]
        ea = z[c + "/in/edge_attr"] if c + "/in/edge_attr" in z.files else None
        out = khop_oracle.extract_multi_hop_neighbors(int(z[c + "/in/num_nodes"]), z[c + "/in/edge_index"], ea, *args)
        want = sorted(k.split("/out/")[1] for k in z.files if k.startswith(c + "/out/"))
        assert want == sorted(out.keys()), c
        for k in want:
            g = z[c + "/out/" + k]
            assert g.shape == out[k].shape and np.array_equal(g, out[k]), (c, k)


def test_khop_quirks(golden_dir):
    """Q1 (pe_attr == 0), Q3 (spd: one active hop per edge; code ranges), Q8 (no-edge graph)."""
    z, cases = _khop_cases(golden_dir)
    for c in cases:
        if c + "/out/pe_attr" in z.files:
            assert not z[c + "/out/pe_attr"].any()
        if c.split("/")[0].endswith("spd") and c + "/out/edge_attr" in z.files:
            ea = z[c + "/out/edge_attr"]
            assert ((ea != 0).sum(1) == 1).all()
    assert "zinc_k8_spd/no_edges/out/peripheral_configuration" in z.files
    assert z["zinc_k8_spd/no_edges/out/peripheral_configuration"].shape == (4, 8, 6)


# ----------------------------------------------------------------------------- layers (fp32)
def _cast(v, dtype):
    """A floating tensor in `dtype` (float64: the oracle as the large-batch GPU tests use it); integer tensors as they are."""
    return v.to(dtype) if v.is_floating_point() else v


def _leafify(sd, trainable, dtype=torch.float32):
    """state_dict -> dict of leaves; only real parameters (keys of param_grads) require grad."""
    return {k: (_cast(v, dtype).clone().requires_grad_(True) if k in trainable else _cast(v, dtype).clone()) for k, v in sd.items()}


def _is(dtype, *tensors):
    return all(t.dtype == dtype for t in tensors)


def _run_layer(case, dtype=torch.float32):
    kind, ctor = case["kind"], case["ctor"]
    p = _leafify(case["state_dict"], case["param_grads"], dtype)
    x = case["x"].to(dtype).clone().requires_grad_(True)
    periph = case.get("peripheral_attr")
    if periph is not None:
        periph = periph.to(dtype).clone().requires_grad_(True)
    pe = case.get("pe_attr")
    K = ctor.get("K", 1)
    if kind == "KPGIN":
        out = LO.kpgin_forward(p, x, case["edge_index"], case["edge_attr"], pe, periph, K=K,
                               combine_kind=ctor.get("combine", "geometric"))
    elif kind == "KPGINPlus":
        out = LO.kpginplus_forward(p, x, case["edge_index"], case["edge_attr"], pe, periph, K=K,
                                   combine_kind=ctor.get("combine"), training=True)
    elif kind == "KPGCN":
        out = LO.kpgcn_forward(p, x, case["edge_index"], case["edge_attr"], pe, periph, K=K,
                               combine_kind=ctor.get("combine", "geometric"))
    elif kind == "KPGraphSAGE":
        out = LO.kpgraphsage_forward(p, x, case["edge_index"], case["edge_attr"], pe, periph, K=K,
                                     combine_kind=ctor.get("combine", "geometric"))
    elif kind == "GINE":
        out = LO.gine_forward(p, x, case["edge_index"], case["edge_attr"], training=True)
    (out * case["out_weight"].to(dtype)).sum().backward()
    return p, x, periph, out


def _check_layer_oracle(golden_cases, dtype):
    """fp32: the restatement against the reference.  float64: the same oracle with float64 parameters and inputs has float64
    outputs and gradients throughout (nothing inside falls back to the default dtype) and agrees with the reference's stored
    fp32 results within the same tolerances."""
    cases = golden_cases("layers")
    assert len(cases) >= 22
    for name, case in cases.items():
        p, x, periph, out = _run_layer(case, dtype)
        assert _is(dtype, out, x.grad, *[p[k].grad for k in case["param_grads"] if p[k].grad is not None]), name
        assert periph is None or periph.grad.dtype == dtype, name
        _close(out.detach(), case["out"], name + ":out")
        _close(x.grad, case["grad_x"], name + ":grad_x", rtol=1e-4)
        if periph is not None:
            _close(periph.grad, case["grad_peripheral_attr"], name + ":grad_periph", rtol=1e-4)
        # parameter grads: absolute tolerance relative to the largest grad of the case (a Linear bias in
        # front of BatchNorm has an analytically-zero grad that is pure rounding noise in both runs)
        gscale = max(float(g.abs().max()) for g in case["param_grads"].values())
        for k, g in case["param_grads"].items():
            got = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
            assert torch.allclose(got, g.to(dtype), rtol=1e-4, atol=1e-5 * max(1.0, gscale)), \
                (name, k, float((got - g).abs().max()), gscale)
        for k, v in case["state_dict_after"].items():
            if "running" in k:
                _close(p[k], v, f"{name}:{k}")


def _check_combine_oracle(golden_cases, dtype):
    cases = golden_cases("combine")
    assert len(cases) >= 7
    for name, case in cases.items():
        p = _leafify(case["state_dict"], case["param_grads"], dtype)
        x = case["x"].to(dtype).clone().requires_grad_(True)
        out = LO.attention_combine(p, x) if name.startswith("att") else LO.geometric_combine(p, x)
        (out * case["out_weight"].to(dtype)).sum().backward()
        assert _is(dtype, out, x.grad, *[p[k].grad for k in case["param_grads"]]), name
        _close(out.detach(), case["out"], name + ":out")
        _close(x.grad, case["grad_x"], name + ":grad_x", rtol=1e-4)
        for k, g in case["param_grads"].items():
            _close(p[k].grad, g, f"{name}:grad[{k}]", rtol=1e-4, atol=1e-5)


def test_path_encoding_table_never_trains(golden_cases):
    """Q1: pe_attr is all-zero, row 0 is the padding row -> hopk_node_path_emb gets exactly zero grad."""
    cases = golden_cases("layers")
    for name, case in cases.items():
        g = case["param_grads"].get("hopk_node_path_emb.weight")
        if g is not None:
            assert not g.any(), name


# ----------------------------------------------------------------------------- whole bodies (fp32)
BODY_KIND = {"KPGINPlus": ("GNNPlus", "KPGINPlus"), "KPGIN": ("GNN", "KPGIN"), "KPGCN": ("GNN", "KPGCN"),
             "KPGINPrime": ("GNNPrime", "KPGIN")}


def _check_body_oracle(golden_cases, dtype):
    from oracle import kp_model_oracle as MO
    cases = golden_cases("bodies")
    assert len(cases) >= 6
    for name, case in cases.items():
        kind, layer_kind = BODY_KIND[case["model_name"]]
        p = _leafify(case["state_dict"], case["param_grads"], dtype)
        score = MO.graph_regression_forward(p, case["inputs"], kind=kind, layer_kind=layer_kind, K=case["K"],
                                            num_layer=case["L"], combine_kind=case["combine"], JK=case["JK"],
                                            residual=bool(case["residual"]), virtual_node=bool(case["virtual_node"]),
                                            training=True)
        loss = (score.squeeze() - case["y"].to(dtype).squeeze()).abs().mean()
        loss.backward()
        assert _is(dtype, score, loss, *[p[k].grad for k in case["param_grads"] if p[k].grad is not None]), name
        _close(score.detach(), case["score"], name + ":score", rtol=1e-4, atol=1e-5)
        _close(loss.detach(), case["loss"], name + ":loss", rtol=1e-4, atol=1e-5)
        gscale = max(float(g.abs().max()) for g in case["param_grads"].values())
        for k, g in case["param_grads"].items():
            got = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
            assert torch.allclose(got, g.to(dtype), rtol=1e-3, atol=2e-5 * max(1.0, gscale)), \
                (name, k, float((got - g).abs().max()), gscale)


def _check_kgin_oracle(golden_cases, dtype):
    """oracle.kgin_forward (run_simulation.py's mask-only KGINConv) against vectors produced by the reference's own class
    (cut out of run_simulation.py with ast and executed alone, tests/golden/make_golden.py): output and every gradient."""
    cases = golden_cases("kgin")
    assert len(cases) >= 3
    for name, c in cases.items():
        p = {k: _cast(v, dtype).clone().requires_grad_(v.is_floating_point() and k != "eps") for k, v in c["state_dict"].items()}
        x = c["x"].to(dtype).clone().requires_grad_(True)
        out = LO.kgin_forward(p, x, c["edge_index"], c["edge_attr"], K=c["K"], batch=c["batch"] if c["pool"] else None)
        (out * c["out_weight"].to(dtype)).sum().backward()
        assert _is(dtype, out, x.grad, *[p[k].grad for k in c["param_grads"]]), name
        _close(out, c["out"], name + ":out")
        _close(x.grad, c["grad_x"], name + ":grad_x")
        for k, g in c["param_grads"].items():
            _close(p[k].grad, g, f"{name}:grad[{k}]")


# ----------------------------------------------------------------------------- the four checks above, in fp32 and in float64
def test_layer_oracle_matches_reference(golden_cases):
    _check_layer_oracle(golden_cases, torch.float32)


def test_combine_oracle_matches_reference(golden_cases):
    _check_combine_oracle(golden_cases, torch.float32)


def test_body_oracle_matches_reference(golden_cases):
    _check_body_oracle(golden_cases, torch.float32)


def test_kgin_oracle_matches_reference_goldens(golden_cases):
    _check_kgin_oracle(golden_cases, torch.float32)


@pytest.mark.parametrize("what", ["layer", "combine", "body", "kgin"])
def test_float64_oracle_matches_reference(golden_cases, what):
    """The oracle with float64 parameters and inputs, on every golden case: float64 outputs and gradients throughout (nothing
    inside falls back to the default dtype), in agreement with the reference's stored fp32 results within the tolerances of
    the fp32 checks.  This is the oracle the large-batch GPU tests compare against."""
    {"layer": _check_layer_oracle, "combine": _check_combine_oracle, "body": _check_body_oracle,
     "kgin": _check_kgin_oracle}[what](golden_cases, torch.float64)


# ----------------------------------------------------------------------------- one body at bench size (float64)
N5K_REL = 5e-13      # of gscale (score, loss: of their own largest entry); ten times the measured agreement, see the docstring


def test_float64_oracle_matches_reference_at_bench_size(golden_cases):
    """The oracle where the large-batch GPU tests use it: KP-GIN+ K = 8, L = 8, h = 104 on 220 synthetic molecules (N = 5148),
    float64 on both sides (the golden is the reference's own GNNPlus + GraphRegression under a float64 default dtype,
    tests/golden/make_golden.py: bodies_n5k).  Inputs and weights are rebuilt from their seeds; the stored sha256 tells
    'the inputs drifted' from 'the results differ'.
    Measured agreement: bit-identical at the thread count the golden was made with (8); with 1 / 4 / 16 / 32 threads the
    worst gradient tensor is 8.0e-15 / 2.4e-15 / 8.4e-16 / 1.4e-15 of gscale, the score 3.4e-14 / 8.4e-15 / 2.3e-15 / 3.3e-15
    and the loss at most 1.5e-15 of their magnitude - the same torch ops, float64 sums in another order.  Asserted at ten times
    the worst of those (3.4e-14), rounded up to 5e-13; a value past 1e-9 would mean the oracle is not the reference's
    function."""
    import parity_f64 as PF
    from kp_gnn_amd.batch import synthetic_zinc_batch
    assert N5K_REL <= 1e-9
    c = golden_cases("bodies_n5k")["gnnplus_k8_l8_h104_geo_n5k"]
    K, L, h = c["K"], c["L"], c["h"]
    sd = {k: v.detach().clone() for k, v in PF.small_body(c["model_name"], c["combine"], K, L, h).state_dict().items()}
    host = synthetic_zinc_batch(c["graphs"], seed0=c["seed0"], K=K)
    assert host.num_nodes == c["num_nodes"] >= 4096
    assert PF.tensors_sha256(host.as_dict(), sd) == c["sha256"], "the seeded inputs or weights are not the golden's"
    score, loss, grads = PF.oracle_body(sd, host.as_dict(), host.y, torch.float64, model_name=c["model_name"],
                                        combine=c["combine"], K=K, L=L)
    ref = c["param_grads"]
    assert c["score"].dtype == torch.float64 and all(g.dtype == torch.float64 for g in ref.values())
    assert sorted(grads) == sorted(ref)
    gscale = max(float(g.abs().max()) for g in ref.values())
    worst = max((float((grads[k] - g).abs().max()) / gscale, k) for k, g in ref.items())
    e_score = float((score - c["score"]).abs().max()) / float(c["score"].abs().max())
    e_loss = abs(float(loss) - float(c["loss"])) / abs(float(c["loss"]))
    print(f"[n5k] worst gradient {worst[1]}: {worst[0]:.3e} of gscale; score {e_score:.3e}; loss {e_loss:.3e}")
    assert e_score <= N5K_REL and e_loss <= N5K_REL, (e_score, e_loss)
    for k, g in ref.items():
        err = float((grads[k] - g).abs().max())
        assert err <= N5K_REL * gscale, (k, err, gscale)
