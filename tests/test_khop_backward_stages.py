"""GPU (-m gpu): the launch sequence of KHopAggregate.backward on every route (tests/khop_backward_cases.py) against the sequence
recorded from the commit before the backward was split into stages (tests/golden/khop_backward_traces.json)."""
import json

import pytest

import khop_backward_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_traces():
    with open(C.FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_every_case(golden_traces):
    assert sorted(golden_traces) == sorted(C.CASES)


@pytest.mark.parametrize("name", list(C.CASES))
def test_backward_launch_trace(name, golden_traces):
    """Entry points and route-telling descriptor fields of every launch the backward call makes, in order."""
    trace, grads = C.CASES[name]()
    assert grads
    assert C.ROUTES[name](trace), (name, "is not on the route it is named after")
    want = golden_traces[name]
    assert len(trace) == len(want), (len(trace), len(want), [n for n, _ in trace], [n for n, _ in want])
    for i, (got, ref) in enumerate(zip(trace, want)):
        assert got == ref, (i, got, ref)
