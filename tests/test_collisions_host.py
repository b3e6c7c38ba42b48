"""CPU: the framework route of the collision count (ops.collision_count on host tensors) and simulation.compute_simulation_collisions
against what the reference's function answered for the same inputs (tests/golden/collisions.npz, written by
tests/golden/make_collision_golden.py), and against float64 brute force under the band rule (tests/collision_cases.py)."""
import os

import numpy as np
import pytest
import torch

import collision_cases as CC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collisions.npz")
NAMES = sorted(CC.golden_inputs())


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_inputs_are_the_generated_ones(golden):
    assert sorted({k.split("/")[0] for k in golden}) == NAMES
    for name, o in CC.golden_inputs().items():
        assert np.array_equal(golden[name + "/x"], o.numpy(), equal_nan=True), name
    assert int(golden["identical_300/n_collision"]) == 44850 and float(golden["identical_300/ratio"]) == 1.0


@pytest.mark.parametrize("name", NAMES)
def test_cpu_route_equals_the_reference(golden, name):
    from kp_gnn_amd import ops, simulation
    o = torch.from_numpy(golden[name + "/x"])
    assert not ops.collision_count_applies(o)
    assert simulation.compute_simulation_collisions(o, ratio=False) == int(golden[name + "/n_collision"])
    assert simulation.compute_simulation_collisions(o) == float(golden[name + "/ratio"])
    got = ops.collision_count(o)
    upper, diag = CC.check_against_f64(got, o)
    assert CC.n_collision(upper, diag, o.shape[0]) == int(golden[name + "/n_collision"])


def test_blocks_smaller_than_the_input_and_other_dtypes():
    from kp_gnn_amd import ops
    o = CC.make(257, 17, 8, 1234 + 257)
    want = ops.collision_count(o)
    for block in (1, 64, 100, 256, 257):
        upper, diag = ops.collision_count_reference(o, CC.EPS, block=block)
        assert (int(upper), int(diag)) == want, block
    assert ops.collision_count(o.double()) == want          # cast to fp32, as the reference's float outputs are
    wide = torch.cat([o, o.new_zeros(257, 300 - 17)], dim=1)  # D = 300: zero columns add nothing to any distance
    assert ops.collision_count(wide) == want
    assert ops.collision_count(torch.cat([o, o.new_zeros(257, 3)], dim=1)[:, :17]) == want        # a strided view


def test_small_row_counts():
    from kp_gnn_amd import ops, simulation
    assert ops.collision_count(torch.zeros(0, 16)) == (0, 0)
    assert ops.collision_count(torch.ones(1, 16)) == (0, 1)
    assert ops.collision_count(torch.full((1, 4), float("nan"))) == (0, 0)
    with pytest.raises(ZeroDivisionError):
        simulation.compute_simulation_collisions(torch.ones(1, 16))
    with pytest.raises(ZeroDivisionError):
        simulation.compute_simulation_collisions(torch.zeros(0, 16))
    with pytest.raises(ZeroDivisionError):                  # the reference divides before it looks at `ratio`
        simulation.compute_simulation_collisions(torch.ones(1, 16), ratio=False)
    two = torch.tensor([[0.5, 1.0], [0.5, 1.0]])
    assert ops.collision_count(two) == (1, 2)
    assert simulation.compute_simulation_collisions(two) == 1.0
    assert simulation.compute_simulation_collisions(two, ratio=False) == 1
    two[1, 0] += 2e-5
    assert ops.collision_count(two) == (0, 2)
    assert simulation.compute_simulation_collisions(two) == 0.0
    with pytest.raises(ValueError):
        ops.collision_count(torch.zeros(5))


def test_switch_returns_the_previous_setting():
    from kp_gnn_amd import ops
    prev = ops.set_native_collisions(False)
    try:
        assert ops.native_collisions() is False
        assert ops.set_native_collisions(True) is False and ops.native_collisions() is True
    finally:
        ops.set_native_collisions(prev)


def test_simulation_refuses_the_cpu():
    from kp_gnn_amd import KpgnnError, simulation
    with pytest.raises(KpgnnError):
        simulation.simulate([20], N=2, K=1, device="cpu")
