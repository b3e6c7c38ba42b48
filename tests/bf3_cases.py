"""Inputs, measure and yardstick of the bf16-split product tests (tests/test_bf16_split_host.py, tests/test_bf16_split_products.py).
No GPU is touched here.

A product is y = a b^T + bias with a [R, K], b [C, K], bias [C] (a Linear: a = x, b = W; a weight gradient: a = dy^T, b = x^T,
K = the row count).  With y64 the same in float64 and u = 2^-24,

    rho(y) = max_ij |y_ij - y64_ij| / (u * (sum_k |a_ik| |b_jk| + |bias_j|))

is the error relative to each element's OWN operands.  The yardstick rho32 is the largest rho of fp32 CPU implementations on the
same inputs: torch matmul at parity_f64.THREADS and, for the forward products (every width I <= 128; the group forward chains S
of them, SEQUENTIAL_UP_TO = 312 terms at the most here), a plain sequential accumulation over k.  The weight gradient's
reduction over 2081 rows gets no sequential sample (rho ~ 100: it would hide a lost product).  A kernel passes
when

    rho(kernel) <= M * max(rho32, 1) + D

with D = D_SPLIT = 8 for the bf16-split route and 0 for the fp32 one.  D is derived: the split keeps six of the nine piece
products, and the three dropped ones sum to at most 7.83 * 2^-24 |a b| (a = b = 0x3F80FFFF, single_product_figure below).
M: below, with the ratios measured on the MI355X.  The code under test never enters the yardstick.

emulated(a, b, bias, products) is the split product in torch on the CPU: h = v & 0xffff0000, m = (v - h) & 0xffff0000,
l = v - h - m, a chosen subset of the nine piece products, accumulated in fp32.  tests/test_bf16_split_host.py proves with it
that the bound tells the documented six products from any five of them at every family and shape the GPU tests use."""
import functools

import torch

from parity_f64 import THREADS

U = 2.0 ** -24
D_SPLIT = 8       # ceil(7.83): the worst sum of the dropped terms in units of u |a b|
# M, by the rule beside M_F64 in tests/test_gpu_parity.py: start at 2; for a largest (rho - D) / max(rho32, 1) between 1 and 2, twice
# it rounded up to one digit; cap 4; a ratio above 2 is a finding, not a reason for a larger M.  Measured on the MI355X, largest
# ratio per kernel (DESIGN.md 5.27 has the table):
#   bf16-split route   linear_bn 0.56, blocked output 0.76, group forward 0.42 (64 terms) and 1.04 (312 terms, `ones2`),
#                      weight gradients 0 (rho 7.7 < D), edge inputs 0
#   fp32 route         linear_bn, blocked output, group forward 1.000 (59 of 72 cases have the sequential sample's rho to the
#                      last digit: these kernels ARE sequential sums), edge inputs 1.11, weight gradients 0.62
#   db, both routes    1.34 (`ones`, [2081, 32]: rho 2.61 against 1.95)            -> M = 2 * 1.34 = 2.7 -> 3
# With the yardstick WITHOUT a sequential sample above 128 terms the fp32 group forward over 3 * 104 terms stood at 1.49 to 2.16
# (`ones`: rho 33.69 against torch's 15.57) and the split one at 6.07 on `ones2` (20.80 against 2.11) on the MI355X host, and
# both at 1.0 on a host whose matmul adds in sequence: fp32_samples says why the sequential sample is there.
M = 3
SEQUENTIAL_UP_TO = 312     # 3 * 104: the longest forward reduction of the cases below

# the six products of bf3_mma6, in its order (smallest terms first): (piece of a, piece of b)
SIX = (("l", "h"), ("h", "l"), ("m", "m"), ("m", "h"), ("h", "m"), ("h", "h"))
THIRD_ORDER = (("l", "h"), ("h", "l"), ("m", "m"))     # dropping any ONE of these must be seen
DROPPED = (("m", "l"), ("l", "m"), ("l", "l"))

FAMILIES = ("randn", "ones", "signed_ones", "wide")


# ------------------------------------------------------------------------------------------------------------ families
def _ones(shape, g, signed, binades=14):
    """Low 16 mantissa bits all set, 7 random top bits, exponents in a window of 14 binades: the worst case of truncation."""
    e = torch.randint(127 - binades // 2, 127 - binades // 2 + binades, shape, generator=g, dtype=torch.int32)
    top = torch.randint(0, 128, shape, generator=g, dtype=torch.int32)
    bits = (e << 23) | (top << 16) | 0xFFFF
    if signed:
        bits = bits | (torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 31)
    return bits.view(torch.float32)


def _draw(family, shape, g):
    if family == "randn":
        return torch.randn(shape, generator=g)
    if family == "ones":
        return _ones(shape, g, False)
    if family == "signed_ones":
        return _ones(shape, g, True)
    if family == "ones2":            # `ones` in a window of 2 binades: more terms of one size per element, a smaller rho32
        return _ones(shape, g, False, binades=2)
    if family == "randn_low16":      # randn with the low 16 mantissa bits set: mixed sign, Gaussian magnitudes, worst truncation
        return (torch.randn(shape, generator=g).view(torch.int32) | 0xFFFF).view(torch.float32)
    if family == "wide":       # randn times 2^e, e uniform in [-20, 20] per element: cancellation across magnitudes
        return torch.ldexp(torch.randn(shape, generator=g), torch.randint(-20, 21, shape, generator=g))
    raise KeyError(family)


def operands(family, R, C, K, seed, bias=True):
    """(a [R, K], b [C, K], bias [C] or None) of one family, seeded."""
    if family == "exact":
        return exact(R, C, K, seed, bias=bias)
    g = torch.Generator().manual_seed(1000 * seed + len(family))
    a, b = _draw(family, (R, K), g), _draw(family, (C, K), g)
    return a, b, (_draw(family, (C,), g) if bias else None)


def exact(R, C, K, seed, bias=True, wide="a", nonzero=8):
    """Small integers times powers of two, for which EVERY route must return y64 exactly.  The wide side holds odd 20-bit
    integers (all three pieces h, m, l are non-zero), the other side `nonzero` entries of +-1 per row of the product's k range,
    times 2^s per row; bias = a 20-bit integer on the same scale.  Every partial sum is an integer below 2^24 on that scale
    (8 * 2^20 + 2^20), so any summation order is exact in fp32, and the dropped piece products (m l, l m, l l) are zero because
    the narrow side has only an h piece."""
    g = torch.Generator().manual_seed(7000 + seed)

    def wide_side(n):
        v = torch.randint(1 << 19, 1 << 20, (n, K), generator=g) | 1
        return (v * (2 * torch.randint(0, 2, (n, K), generator=g) - 1)).float() * 2.0 ** -5

    def narrow_side(n):
        v = torch.zeros(n, K)
        for r in range(n):      # (rows are short: at most a few thousand assignments of 8 entries)
            idx = torch.randperm(K, generator=g)[:nonzero]
            v[r, idx] = (2 * torch.randint(0, 2, (min(nonzero, K),), generator=g) - 1).float()
        return torch.ldexp(v, torch.randint(-3, 4, (n, 1), generator=g))

    a, b = (wide_side(R), narrow_side(C)) if wide == "a" else (narrow_side(R), wide_side(C))
    bv = None
    if bias:
        assert wide == "a", "the bias shares the scale of b's rows"
        scale = b.abs().max(dim=1).values            # 2^s of every row of b
        bv = torch.randint(-(1 << 20), 1 << 20, (C,), generator=g).float() * 2.0 ** -5 * scale
    return a, b, bv


# ------------------------------------------------------------------------------------------------------- measure, yardstick
def ref64(a, b, bias=None):
    y = a.double() @ b.double().t()
    return y if bias is None else y + bias.double()


def denominator(a, b, bias=None):
    """sum_k |a_ik| |b_jk| + |bias_j| in float64."""
    d = a.double().abs() @ b.double().abs().t()
    return d if bias is None else d + bias.double().abs()


def rho(y, y64, den):
    """max_ij |y - y64| / (u den); an element whose operands are all zero must be exactly right; a non-finite y is inf."""
    y = y.detach().cpu().double().reshape(y64.shape)
    if not bool(torch.isfinite(y).all()):
        return float("inf")
    err = (y - y64).abs()
    unit = U * den
    r = torch.where(unit > 0, err / unit.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


def _sequential(a, b, bias):
    acc = torch.zeros(a.shape[0], b.shape[0])
    for k in range(a.shape[1]):
        acc = acc + a[:, k:k + 1] * b[:, k].unsqueeze(0)
    return acc if bias is None else acc + bias


def fp32_samples(a, b, bias=None, sequential=None):
    """The fp32 CPU results the yardstick is taken over: torch matmul at THREADS, and for K <= SEQUENTIAL_UP_TO (sequential=None)
    the plain sequential accumulation over k.  sequential=False leaves it out (the weight gradient: over K = 2081 it sits at
    rho ~ 100 and would hide a lost product).
    Why the sequential sample is there at all lengths the forward kernels reduce over: what torch's matmul does is the host's
    business.  On `ones2` over 312 terms it measured rho32 = 2.1 on the MI355X host (blocked partial sums) and 12.3 on a host
    whose matmul adds in sequence, on `ones` 15.6 and 33.7 - the same kernel result passed on one host and failed on the other.
    The sequential sum is the same number everywhere, and a matrix kernel that adds k step after k step into one accumulator
    is a sequential sum; tests/test_bf16_split_host.py shows that with it five products are still 4 times outside the bound."""
    before = torch.get_num_threads()
    out = []
    try:
        for t in THREADS:
            torch.set_num_threads(t)
            y = a @ b.t()
            out.append(y if bias is None else y + bias)
    finally:
        torch.set_num_threads(before)
    if sequential is None:
        sequential = a.shape[1] <= SEQUENTIAL_UP_TO
    if sequential:
        out.append(_sequential(a, b, bias))
    return out


def bound(rho32, M, D):
    return M * max(rho32, 1.0) + D


# --------------------------------------------------------------------------------------------------------- the emulation
def split3(v, flush=False):
    """v = h + m + l exactly, three bf16 pieces by truncation (csrc/bf3.h).  flush: subnormal pieces become zero, as a matrix unit
    that flushes subnormal inputs would see them."""
    mask = -65536       # 0xffff0000 as int32
    h = (v.view(torch.int32) & mask).view(torch.float32)
    r = v - h
    m = (r.view(torch.int32) & mask).view(torch.float32)
    p = {"h": h, "m": m, "l": r - m}
    if flush:
        p = {k: torch.where(t.abs() < 2.0 ** -126, torch.zeros_like(t), t) for k, t in p.items()}
    return p


def emulated(a, b, bias=None, products=SIX, flush=False):
    """The split product with the given piece products, accumulated in fp32 in the given order."""
    pa, pb = split3(a.contiguous(), flush), split3(b.contiguous(), flush)
    acc = torch.zeros(a.shape[0], b.shape[0])
    for p, q in products:
        acc = acc + pa[p] @ pb[q].t()
    return acc if bias is None else acc + bias


def five_of_six(drop):
    assert drop in THIRD_ORDER
    return tuple(pq for pq in SIX if pq != drop)


def single_product_figure():
    """The three dropped terms of a = b = 0x3F80FFFF, in units of u |a b|: 7.83 (exact arithmetic in float64)."""
    a = torch.tensor([0x3F80FFFF], dtype=torch.int32).view(torch.float32)
    p = {k: float(v) for k, v in split3(a).items()}
    assert p["h"] + p["m"] + p["l"] == float(a)
    dropped = sum(p[x] * p[y] for x, y in DROPPED)
    kept = sum(p[x] * p[y] for x, y in SIX)
    assert kept + dropped == float(a) * float(a)          # (48-bit product: exact in float64)
    return dropped / (U * float(a) * float(a))


# ------------------------------------------------------------------------------------------------- the cases both tests use
N_FWD = 4129          # >= 4096 (the bf16-split forward kernels' threshold), and 4129 = 129 * 32 + 1 = 43 * 96 + 1: a ragged last tile
N_WGRAD = 2081        # 65 chunks of 32 rows + 1
LIN_BN_SHAPES = ((104, 104), (32, 64), (96, 32))          # (I, O)
GROUP_SHAPES = ((3, 104, 104), (2, 32, 32))               # (S, H, O)
# kpgnn_linear_fwd takes a blocked output only with more than 128 columns in all (S * H > 128, include/kpgnn.h): (2, 32, 32) is
# refused (asserted in the GPU test), five blocks of 32 are the smallest that reach lin3_kernel<2, 1>
BLOCKED_SHAPES = ((3, 104, 104), (5, 32, 32))
BLOCKED_REFUSED = (2, 32, 32)
WGRAD_SHAPES = ((104, 104), (32, 96))                     # (O, I)
WGRAD_GROUP = 3
FWD_FAMILIES = FAMILIES
# Pairs that tests/test_bf16_split_host.py does not pass, and what takes their place.  Over the group forward's reduction of
# 3 * 104 terms randn leaves five products at 3.9 times the bound (M = 2 already), and `ones` at 3.9 times (M = 3; on a host
# whose fp32 matmul accumulates in sequence rho32 is 33.7 there): below the 4 asked for.
REPLACED = {("group_fwd", "randn", (3, 104, 104)): "randn_low16", ("group_fwd", "ones", (3, 104, 104)): "ones2"}
POSITIVE = ("ones", "ones2")


def group_fwd_family(fam, shape):
    return REPLACED.get(("group_fwd", fam, tuple(shape)), fam)
WGRAD_FAMILIES = ("ones", "signed_ones")     # randn over a reduction of 2081 leaves five products at ~1.2 of the bound: not used


def product_cases():
    """Every (name, family, R, C, K, bias, sequential, masked) the GPU tests hold to the bound: the host test proves the bound
    discriminates at each of them.  masked: a third of a's entries are zeroed by a ReLU mask (third_mask)."""
    out = []
    for fam in FWD_FAMILIES:
        for I, O in LIN_BN_SHAPES:
            out.append((f"linear_bn {fam} I{I} O{O}", fam, N_FWD, O, I, True, None, False))
        for S, H, O in GROUP_SHAPES:
            gf = group_fwd_family(fam, (S, H, O))
            out.append((f"group_fwd {gf} S{S} H{H} O{O}", gf, N_FWD, O, S * H, True, None, False))
        for S, H, O in BLOCKED_SHAPES:
            for masked in (False, True):
                out.append((f"blocked {fam} S{S} H{H} O{O}{' masked' if masked else ''}", fam, N_FWD, S * H, O, False, None, masked))
    for fam in WGRAD_FAMILIES:
        for O, I in WGRAD_SHAPES:
            out.append((f"wgrad {fam} O{O} I{I}", fam, O, I, N_WGRAD, False, False, False))
            for masked in (False, True):
                out.append((f"wgrad_group {fam} O{O} I{I}{' masked' if masked else ''}", fam, O, WGRAD_GROUP * I, N_WGRAD, False, False, masked))
    return out


def third_mask(shape, seed):
    """A ReLU mask as the kernels read it (an entry passes where mask > 0): a third of the entries are 0 or negative."""
    g = torch.Generator().manual_seed(9000 + seed)
    r = torch.rand(shape, generator=g)
    return torch.where(r < 1.0 / 6, torch.zeros(shape), torch.where(r < 1.0 / 3, -torch.ones(shape), 0.5 + r))


@functools.lru_cache(maxsize=4)        # (consecutive cases share a reference; up to 30 MB each)
def reference(family, R, C, K, seed, bias=True, sequential=None, masked=False, wide="a"):
    """(a, mask, b, bias, y64, den, rho32) of one case, computed once; callers must not modify the tensors.  mask: all positive,
    or third_mask; the product is taken with a * [mask > 0].  rho32 of the `exact` family is 0: it is asserted with equality."""
    if family == "exact":
        a, b, bv = exact(R, C, K, seed, bias=bias, wide=wide)
    else:
        a, b, bv = operands(family, R, C, K, seed, bias=bias)
    mask = third_mask(a.shape, seed) if masked else torch.ones_like(a)
    am = a * (mask > 0)
    y64, den = ref64(am, b, bv), denominator(am, b, bv)
    r32 = max(rho(y, y64, den) for y in fp32_samples(am, b, bv, sequential=sequential)) if family != "exact" else 0.0
    return a, mask, b, bv, y64, den, r32


def edge_operands(R, C, K, seed):
    """randn with magnitudes clamped to [2^-4, 4]: scaled by 2^-110 every VALUE stays a normal fp32 number (only its m and l pieces
    go subnormal), scaled by 2^124 none passes 2^126."""
    g = torch.Generator().manual_seed(500 + seed)

    def draw(shape):
        v = torch.randn(shape, generator=g)
        return torch.where(v < 0, -torch.ones(shape), torch.ones(shape)) * v.abs().clamp(2.0 ** -4, 4.0)
    return draw((R, K)), draw((C, K)), draw((C,))


def scaled(t, p):
    """t * 2^p, exact while nothing leaves the normal range."""
    return torch.ldexp(t, torch.tensor(p))
