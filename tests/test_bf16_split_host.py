"""No GPU: the harness of tests/test_bf16_split_products.py discriminates.  With the torch emulation of the bf16-split product
(tests/bf3_cases.py) on the CPU, for every family and shape the GPU tests hold to the bound

    rho <= M * max(rho32, 1) + D_SPLIT

  * the documented SIX piece products are inside it with M = 2 (the starting value of M), and
  * any FIVE of them (al bh, ah bl or am bm dropped) are at least 4 times outside it, at the M the GPU tests use
    (bf3_cases.M): a kernel that loses one product fails them.

A family / shape pair that fails either condition may not be used on the GPU (bf3_cases.product_cases is the one list both
tests read).  Also here: the 7.83 figure D_SPLIT comes from, the exactness of the split, and the `exact` family."""
import pytest
import torch

import bf3_cases as C

M_SIX = 2           # the emulated six products sit inside the bound at the starting value of M
OUTSIDE = 4.0       # five products: at least this many times the bound the GPU tests assert


def test_single_product_figure():
    """a = b = 0x3F80FFFF: the dropped terms are 7.83 u |a b|, not below u as the kernels' comments used to say."""
    f = C.single_product_figure()
    print(f"dropped / (u |a b|) = {f:.4f}")
    assert 7.82 < f < 7.84
    assert f <= C.D_SPLIT


@pytest.mark.parametrize("family", C.FAMILIES + ("ones2", "randn_low16", "exact"))
def test_split_is_exact_and_pieces_are_bf16(family):
    a, _, _ = C.operands(family, 257, 8, 104, seed=1, bias=False)
    p = C.split3(a)
    assert torch.equal(p["h"].double() + p["m"].double() + p["l"].double(), a.double())
    for k, v in p.items():
        assert bool(((v.view(torch.int32) & 0xFFFF) == 0).all()), (family, k, "a piece has more than 8 significant bits")


def test_ones_family_bits():
    a, b, bias = C.operands("signed_ones", 64, 32, 104, seed=2)
    for t in (a, b, bias):
        bits = t.view(torch.int32)
        assert bool(((bits & 0xFFFF) == 0xFFFF).all())
        e = (bits >> 23) & 0xFF
        assert 120 <= int(e.min()) and int(e.max()) <= 133 and int(e.max()) - int(e.min()) == 13
    assert bool((a < 0).any()) and bool((a > 0).any())
    assert bool((C.operands("ones", 64, 32, 104, seed=2)[0] > 0).all())


@pytest.mark.parametrize("case", C.product_cases(), ids=lambda c: c[0].replace(" ", "-"))
def test_bound_tells_six_products_from_five(case):
    name, family, R, Cc, K, bias, sequential, masked = case
    a, mask, b, bv, y64, den, r32 = C.reference(family, R, Cc, K, 0, bias, sequential, masked)
    a = a * (mask > 0)
    six = C.rho(C.emulated(a, b, bv), y64, den)
    print(f"[bf3-host] {name}: rho32 {r32:.2f}  six {six:.2f}  bound(M=2) {C.bound(r32, M_SIX, C.D_SPLIT):.2f}", end="")
    assert six <= C.bound(r32, M_SIX, C.D_SPLIT), (name, six, r32)
    worst = float("inf")
    for drop in C.THIRD_ORDER:
        five = C.rho(C.emulated(a, b, bv, C.five_of_six(drop)), y64, den)
        worst = min(worst, five / C.bound(r32, C.M, C.D_SPLIT))
    print(f"  five / bound(M) >= {worst:.2f}")
    assert worst >= OUTSIDE, (name, worst)


@pytest.mark.parametrize("wide", ["a", "b"])
@pytest.mark.parametrize("R,Cc,K", [(257, 104, 104), (64, 96, 2081)])
def test_exact_family_is_exact_on_every_route(R, Cc, K, wide):
    """Every fp32 sample, the six-product emulation and float64 agree bit for bit on the `exact` family."""
    a, b, bv = C.exact(R, Cc, K, seed=3, bias=wide == "a", wide=wide)
    y64 = C.ref64(a, b, bv)
    p = C.split3(a if wide == "a" else b)
    assert all(bool((v != 0).any()) for v in p.values()), "the wide side must exercise all three planes"
    for y in C.fp32_samples(a, b, bv, sequential=True) + [C.emulated(a, b, bv)]:
        assert torch.equal(y.double(), y64)


def test_subnormal_piece_case_would_see_a_flush():
    """The GPU edge at (2^-110 x, 2^110 W): with the subnormal pieces of x (nearly every l, the smallest m) flushed to zero the
    emulated product is outside the bound at any M the rule allows (cap 4) - it loses about as much as a lost al bh product;
    with them kept it is where the unscaled product is.  The case tells the two apart."""
    a, b, bias = C.edge_operands(257, 104, 104, seed=9)
    y64, den = C.ref64(a, b, bias), C.denominator(a, b, bias)
    r32 = max(C.rho(y, y64, den) for y in C.fp32_samples(a, b, bias))
    sa, sb = C.scaled(a, -110), C.scaled(b, 110)
    kept = C.rho(C.emulated(sa, sb, bias), y64, den)
    flushed = C.rho(C.emulated(sa, sb, bias, flush=True), y64, den)
    print(f"kept {kept:.2f}  flushed {flushed:.1f}  bound {C.bound(r32, C.M, C.D_SPLIT):.2f}")
    assert kept == C.rho(C.emulated(a, b, bias), y64, den)
    assert kept <= C.bound(r32, M_SIX, C.D_SPLIT)
    assert flushed > 2 * C.bound(r32, 4, C.D_SPLIT)
