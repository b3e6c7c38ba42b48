import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            assert k not in dst, k
            dst[k] = v


def load_golden_cases(name):
    """The cases of tests/golden/<name>.pt, or of <name>.part00.pt, .part01.pt, ... merged in order: a fixture whose
    tensors pass 1 MiB is stored in parts (tests/golden/make_golden.py: save_cases)."""
    import torch
    whole = os.path.join(GOLDEN, name + ".pt")
    if os.path.exists(whole):
        return torch.load(whole, weights_only=True)
    parts = sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".part[0-9][0-9].pt")))
    assert parts, f"golden fixture {name} not found under {GOLDEN}"
    cases = {}
    for p in parts:
        _merge(cases, torch.load(p, weights_only=True))
    return cases


@pytest.fixture(scope="session")
def golden_cases():
    return load_golden_cases
