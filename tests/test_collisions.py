"""GPU (-m gpu): the collision count of the regular-graph simulation - ops.collision_count / simulation.* on csrc/collisions.hip
(kpgnn_collision_count).

The yardstick is float64 brute force on the host under the band rule (tests/collision_cases.py): a pair whose float64 squared
distance lies outside [eps (1 - delta), eps (1 + delta)], delta = (D + 2) 2^-23, must be classified as float64 classifies it, so
|count - float64 count| <= pairs inside the band - and the constructed inputs have none there, which is asserted.  The recorded
answers of the reference's own function (tests/golden/collisions.npz) are met exactly.  The counts above 2^31 are analytic.
The kernel's tile is 128 x 128 pairs, a 16-column chunk at a time: the row counts straddle 64, 128 and 256 and reach 1000 (36
tiles, the linear tile index decoded on every block), the column counts straddle the chunk (16, 17) and reach the limit 256."""
import os

import numpy as np
import pytest
import torch

import collision_cases as CC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collisions.npz")
NAMES = sorted(CC.golden_inputs())
ROWS = (1, 2, 63, 64, 65, 127, 128, 129, 257, 1000)
COLS = (1, 3, 16, 17, 64, 100, 256)
# every row count at both sides of the column chunk, every column count at 2 tile rows + 1 and at 36 tiles
SHAPES = sorted({(n, d) for n in ROWS for d in (16, 17)} | {(n, d) for n in (129, 1000) for d in COLS})


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


class _Spy:
    """Names of the C-ABI launches made inside the block."""

    def __enter__(self):
        from kp_gnn_amd import _lib
        self.names, self._lib, self._real = [], _lib, _lib.launch

        def spy(name, *a, **k):
            self.names.append(name)
            return self._real(name, *a, **k)

        _lib.launch = spy
        return self

    def __exit__(self, *exc):
        self._lib.launch = self._real
        return False


def _kernel(o):
    """(upper, diag) straight from kpgnn_collision_count, whatever the row count and the switch."""
    from kp_gnn_amd import ops
    return tuple(ops._collision_count_launch(o, CC.EPS).tolist())


@pytest.mark.parametrize("name", NAMES)
def test_golden_entries_through_the_kernel(golden, name):
    from kp_gnn_amd import ops, simulation
    o = torch.from_numpy(golden[name + "/x"]).to(_dev())
    assert ops.collision_count_applies(o)
    with _Spy() as spy:
        assert simulation.compute_simulation_collisions(o, ratio=False) == int(golden[name + "/n_collision"])
        assert simulation.compute_simulation_collisions(o) == float(golden[name + "/ratio"])
    assert spy.names == ["kpgnn_collision_count"] * 2
    CC.check_against_f64(ops.collision_count(o), o)


@pytest.mark.parametrize("N,D", SHAPES)
def test_tile_and_chunk_edges(N, D):
    from kp_gnn_amd import ops
    o = CC.make(N, D, min(8, max(1, N // 2)), 7000 + 31 * N + D)
    dev_o = o.to(_dev())
    got = _kernel(dev_o)
    want = CC.check_against_f64(got, o)
    if N >= 64:
        assert want[0] > 0 and want[0] < N * (N - 1) // 2          # the case has collisions and near misses
    assert ops.collision_count(dev_o) == got


def test_identical_rows_are_counted_once_per_pair():
    o = CC.identical_case().to(_dev())
    assert _kernel(o) == (300 * 299 // 2, 300) == (44850, 300)


def test_strided_rows_are_read_in_place():
    from kp_gnn_amd import ops
    o = CC.make(257, 17, 8, 1234 + 257)
    want = CC.check_against_f64(_kernel(o.to(_dev())), o)
    wide = torch.full((257, 40), 7.0)
    wide[:, 3:20] = o                                    # rows 160 B apart, the first column 12 B into a row
    view = wide.to(_dev())[:, 3:20]
    assert ops._rows_view(view, 17) is view and not view.is_contiguous()
    assert _kernel(view) == want
    assert ops.collision_count(view) == want
    assert ops.collision_count(wide.to(_dev()).t()[3:20].t()) == want      # the same rows again, through two transposes
    cols = o.t().contiguous().to(_dev()).t()              # unit ROW stride: not walkable in place, copied
    assert cols.stride(1) != 1 and ops.collision_count(cols) == want


def test_nan_and_inf_rows_fall_out_as_in_the_framework():
    from kp_gnn_amd import ops
    o = CC.nan_inf_case()
    upper, diag, band = CC.f64_counts(o)
    assert diag == 37 and band == 0
    assert _kernel(o.to(_dev())) == (upper, diag)
    both = torch.tensor([[float("inf"), 1.0], [float("inf"), 1.0], [float("-inf"), 1.0], [float("nan"), 1.0], [0.5, 1.0]])
    assert _kernel(both.to(_dev())) == (0, 1) == ops.collision_count(both)


def test_switch_off_and_wide_rows_take_the_framework_expression():
    from kp_gnn_amd import ops
    o = CC.make(300, 100, 8, 1234 + 300)
    dev_o = o.to(_dev())
    want = CC.check_against_f64(_kernel(dev_o), o)
    prev = ops.set_native_collisions(False)
    try:
        assert not ops.collision_count_applies(dev_o)
        with _Spy() as spy:
            assert ops.collision_count(dev_o) == want
        assert spy.names == []
    finally:
        ops.set_native_collisions(prev)
    ops.set_native_collisions(True)
    try:
        wide = torch.cat([o, torch.zeros(300, 200)], dim=1).to(_dev())          # D = 300: beyond the kernel's 256 columns
        assert not ops.collision_count_applies(wide)
        with _Spy() as spy:
            assert ops.collision_count(wide) == want
            assert ops.collision_count(dev_o.double()) == want                     # another dtype: cast inside the framework expression
        assert spy.names == []
        with _Spy() as spy:
            assert ops.collision_count(dev_o) == want
        assert spy.names == ["kpgnn_collision_count"]
    finally:
        ops.set_native_collisions(prev)


def test_counts_beyond_32_bits():
    """70,000 rows of 16 columns.  Row i is one of three well-separated constants by i % 3: sum_r C(n_r, 2) = 816,631,667 pairs
    (n = 23334, 23333, 23333), below 2^31.  Then every row the same: C(70000, 2) = 2,449,965,000, above 2^31."""
    N = 70000
    i = torch.arange(N, device=_dev())
    o = ((i % 3).float() * 0.25 + 0.125).unsqueeze(1).expand(N, 16).contiguous()
    sizes = [len(range(r, N, 3)) for r in range(3)]
    want = sum(n * (n - 1) // 2 for n in sizes)
    assert sizes == [23334, 23333, 23333] and want == 816631667 < 2 ** 31
    assert _kernel(o) == (want, N)
    o.fill_(0.375)
    assert _kernel(o) == (2449965000, N) and 2449965000 > 2 ** 31


@pytest.mark.parametrize("graph", (False, True))
def test_simulation_on_twenty_node_graphs(graph):
    """simulate([20], R=3, N=4, K=2): with k = 1 every node of a 3-regular graph has the same 1-hop picture, so all 80 node rows
    (and all 4 pooled rows) collide: rate exactly 1.0.  With k = 2 the device count is held to float64 brute force on the returned
    embeddings under the band rule."""
    from kp_gnn_amd import ops, simulation
    rates, outs = simulation.simulate([20], R=3, N=4, K=2, graph=graph, return_outputs=True, device=_dev())
    rows = 4 if graph else 80
    assert sorted(rates) == [(20, 1), (20, 2)] == sorted(outs)
    for k in (1, 2):
        out = outs[(20, k)]
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (rows, 16)
        got = ops.collision_count(out)
        upper, diag = CC.check_against_f64(got, out, constructed=False)
        assert got[1] == rows == diag
        assert rates[(20, k)] == CC.n_collision(got[0], got[1], rows) / (rows * (rows - 1) / 2)
    assert rates[(20, 1)] == 1.0
    again, outs2 = simulation.simulate([20], R=3, N=4, K=2, graph=graph, device=_dev(), chunk_graphs=3, return_outputs=True)
    assert again[(20, 1)] == 1.0                         # two chunks, 3 + 1 graphs: the same rows, concatenated on the device
    assert torch.allclose(outs2[(20, 2)], outs[(20, 2)], rtol=1e-5, atol=1e-6)
