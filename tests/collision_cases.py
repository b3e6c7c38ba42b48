"""Shared by tests/test_collisions_host.py, tests/test_collisions.py and tests/golden/make_collision_golden.py: the inputs of the
collision-count tests, the float64 yardstick and the band rule.

make(N, D, P, seed): N fp32 rows, each a copy of one of P base rows (standard normal, column 0 redrawn in [0.5, 0.99)) whose
column 0 is left alone (kinds 0, 1: copy), raised by 5e-6 (kind 2: near) or by 2e-5 (kind 3: far).  Rows of one base row then
sit at a squared distance of 0 (same kind), ~2.5e-11 (copy / near: they collide at eps = 1e-10), ~2.25e-10 (near / far) or
~4e-10 (copy / far: they do not); rows of different base rows are O(1) apart.  Column 0 is below 1, so the fp32 sum carries
the offset with an error of at most 2^-25 ~ 3e-8 absolutely, under 1 % of 5e-6: no pair comes near the threshold's band.

Band rule (include/kpgnn.h, csrc/collisions.hip): with delta = (D + 2) 2^-23, a pair whose float64 d2 lies outside
[eps (1 - delta), eps (1 + delta)] must be classified as float64 classifies it; eps is the fp32 value of 1e-10, which is what
both routes compare against.  f64_counts returns the float64 counts and the number of pairs inside the band."""
import numpy as np
import torch

EPS = 1e-10
EPS32 = float(np.float32(EPS))

# (N, D, P): the constructed cases of the golden fixture, seed 1234 + N each
GOLDEN_SHAPES = ((127, 16, 8), (129, 1, 5), (257, 17, 8), (200, 3, 6), (300, 100, 8), (256, 64, 8))


def make(N, D, P, seed):
    rng = np.random.RandomState(seed)
    base = rng.standard_normal((P, D)).astype(np.float32)
    base[:, 0] = rng.uniform(0.5, 0.99, P).astype(np.float32)
    rows = base[rng.randint(0, P, N)].copy()
    kind = rng.randint(0, 4, N)
    rows[:, 0] += np.where(kind == 2, np.float32(5e-6), np.where(kind == 3, np.float32(2e-5), np.float32(0))).astype(np.float32)
    return torch.from_numpy(rows)


def nan_inf_case():
    """40 rows of make(40, 8, 4, ..) with a NaN in row 5 and the same Inf in rows 11 and 23: none of the three collides with
    anything, itself included (x - x is NaN there), so the reference's count subtracts N from a sum that holds only 37 diagonal
    hits."""
    o = make(40, 8, 4, 99)
    o[5, 3] = float("nan")
    o[11] = o[23]
    o[11, 2] = o[23, 2] = float("inf")
    return o


def identical_case(N=300, D=16):
    return torch.full((N, D), 0.375).contiguous()


def golden_inputs():
    """name -> fp32 [N,D] input of every entry of tests/golden/collisions.npz."""
    cases = {"make_%d_%d_%d" % s: make(*s, 1234 + s[0]) for s in GOLDEN_SHAPES}
    cases["nan_inf"] = nan_inf_case()
    cases["identical_300"] = identical_case()
    return cases


def delta(D):
    return (D + 2) * 2.0 ** -23


def f64_counts(o, eps=EPS32):
    """(upper, diag, band_pairs) by brute force in float64 on the host: d2 is accumulated column by column into one [N,N] float64
    matrix; band_pairs counts the pairs i <= j whose d2 lies inside [eps (1 - delta), eps (1 + delta)]."""
    a = o.detach().cpu().double().numpy()
    N, D = a.shape
    d2 = np.zeros((N, N))
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(D):
            diff = a[:, d, None] - a[None, :, d]
            d2 += diff * diff
        hit = d2 < eps
        band = (d2 >= eps * (1 - delta(D))) & (d2 <= eps * (1 + delta(D)))
    iu = np.triu_indices(N, 1)
    return int(hit[iu].sum()), int(np.diagonal(hit).sum()), int(band[iu].sum() + np.diagonal(band).sum())


def n_collision(upper, diag, N):
    """The reference's count from the two integers (run_simulation.py:173)."""
    return int((2 * upper + diag - N) / 2)


def check_against_f64(got, o, eps=EPS32, constructed=True):
    """got = (upper, diag) of the code under test: the band assertion on both integers, after the precondition band_pairs == 0
    for the constructed inputs (asserted, not skipped; embeddings of a model are taken as they come).  Returns the float64 pair."""
    upper, diag, band = f64_counts(o, eps)
    print(f"collisions N={o.shape[0]} D={o.shape[1]}: got {tuple(got)} float64 {(upper, diag)} band_pairs {band}")
    if constructed:
        assert band == 0, band
    assert abs(got[0] - upper) <= band and abs(got[1] - diag) <= band, (got, (upper, diag), band)
    return upper, diag
