"""kpgnn_random_regular_graphs through ctypes (csrc/regular_graphs.hip): the refusals, which need no device, and on the GPU
(-m gpu) the bits of the host route - edge_index, attempts and status - at the smallest shapes on both sides of every bound the
kernel has (tests/regular_graph_cases.py: each power-of-two padding step of the key count, the wavefront / block bound, every
block size), for one graph and for a count that leaves the last wavefront-class block partly filled."""
import ctypes

import numpy as np
import pytest
import torch

import regular_graph_cases as RC

SENTINEL = -7


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _call(G, n, d, seed=0, first_graph=0, max_attempts=4096):
    """One launch over sentinel-filled outputs: (rc, edge_index, attempts, status) as host arrays."""
    from kp_gnn_amd import _lib
    dev = _dev()
    ei = torch.full((2, G * n * d), SENTINEL, dtype=torch.int64, device=dev)
    attempts = torch.full((G,), SENTINEL, dtype=torch.int32, device=dev)
    status = torch.full((G,), SENTINEL, dtype=torch.int32, device=dev)
    desc = _lib.RrgDesc()
    desc.G, desc.n, desc.d, desc.max_attempts, desc.seed, desc.first_graph = G, n, d, max_attempts, seed, first_graph
    desc.edge_index, desc.attempts, desc.status = ei.data_ptr(), attempts.data_ptr(), status.data_ptr()
    rc = _lib.load().kpgnn_random_regular_graphs(ctypes.byref(desc), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc, ei.cpu().numpy(), attempts.cpu().numpy(), status.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,G", RC.device_cases())
def test_bits_of_the_host_route(n, d, G):
    rc, ei, attempts, status = _call(G, n, d)
    _, _, want_ei, want_attempts, want_status = RC.host(G, n, d)
    assert rc == 0
    assert np.array_equal(status, want_status) and (status == 0).all()
    assert np.array_equal(attempts, want_attempts)
    assert np.array_equal(ei, want_ei)


@pytest.mark.gpu
def test_seed_and_first_graph_reach_the_counter():
    """A 64-bit seed (negative as int64) and a graph id above 2^32: both halves of each enter the generator."""
    for seed, first in ((-3, 1), (2 ** 63 - 1, 0), (7, 2 ** 33 + 5)):
        rc, ei, attempts, status = _call(5, 20, 3, seed=seed, first_graph=first)
        want = RC.host(5, 20, 3, seed, first)
        assert rc == 0 and np.array_equal(ei, want[2]) and np.array_equal(attempts, want[3]) and np.array_equal(status, want[4])


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,G", ((6, 3, 200), (86, 3, 40)))
def test_exhausted_graphs_keep_their_columns(n, d, G):
    """max_attempts = 1, in the wavefront class and in the block class: status 1 and attempts 1 where the first pairing is
    rejected, those graphs' columns still hold the sentinel, the others are the host route's."""
    m = n * d
    rc, ei, attempts, status = _call(G, n, d, max_attempts=1)
    _, _, want_ei, want_attempts, want_status = RC.host(G, n, d, max_attempts=1)
    assert rc == 0 and (attempts == 1).all() and np.array_equal(attempts, want_attempts)
    assert np.array_equal(status, want_status) and set(status.tolist()) == {0, 1}
    out = status != 0
    assert (ei.reshape(2, G, m)[:, out] == SENTINEL).all()
    assert np.array_equal(ei.reshape(2, G, m)[:, ~out], want_ei.reshape(2, G, m)[:, ~out])


def test_refusals_come_before_any_device_call():
    """Odd n * d, d >= n, counts that make no sense and a NULL output are KPGNN_EINVAL; d = 5, n = 2049 and n * d > 8192 are
    KPGNN_ELIMIT; G = 0 is KPGNN_OK with nothing behind the pointers.  No stream, no device memory: nothing may be launched."""
    from kp_gnn_amd import _lib
    lib = _lib.load()
    a = 0x10000                                       # dummy, non-NULL: never dereferenced

    def rc(G=2, n=6, d=3, max_attempts=4096, first_graph=0, ei=a, attempts=a, status=a):
        desc = _lib.RrgDesc()
        desc.G, desc.n, desc.d, desc.max_attempts, desc.seed, desc.first_graph = G, n, d, max_attempts, 0, first_graph
        desc.edge_index, desc.attempts, desc.status = ei, attempts, status
        return lib.kpgnn_random_regular_graphs(ctypes.byref(desc), None)

    assert lib.kpgnn_random_regular_graphs(None, None) == -1
    assert rc(n=5, d=3) == -1 and b"odd" in lib.kpgnn_last_error()
    assert rc(n=4, d=4) == -1 and b"d >= n" in lib.kpgnn_last_error()
    assert rc(n=3, d=5) == -1                         # (d >= n before the degree limit)
    assert rc(G=-1) == -1 and rc(n=0, d=0) == -1 and rc(d=0) == -1 and rc(max_attempts=0) == -1 and rc(first_graph=-1) == -1
    assert rc(ei=None) == -1 and rc(attempts=None) == -1 and rc(status=None) == -1
    assert b"NULL" in lib.kpgnn_last_error()
    assert rc(n=12, d=5) == -3 and b"degree limit" in lib.kpgnn_last_error()
    assert rc(n=2049, d=2) == -3 and rc(n=2050, d=4) == -3 and rc(n=4096, d=3) == -3
    assert rc(G=0, ei=None, attempts=None, status=None) == 0
