"""Uniform random simple d-regular graphs by the pairing model with rejection, on the host: the definition of
include/kpgnn.h (kpgnn_random_regular_graphs) written out in numpy - Philox4x32-10 on uint64 arrays, np.sort of the keys, the
two checks - and therefore the specification the kernel of csrc/regular_graphs.hip is tested against, bit for bit.  Graph g of a
call is a function of (seed, first_graph + g, n, d) alone.  Host only: numpy, never the HIP library (of _lib, its constants)."""
import numpy as np

from ._lib import RRG_EXHAUSTED, RRG_MAX_DEGREE, RRG_MAX_NODES, RRG_MAX_STUBS, RRG_OK

_U32 = np.uint64(0xFFFFFFFF)
_INDEX = np.uint64(RRG_MAX_STUBS - 1)                   # the 13 index bits of a key
_CHUNK = 1 << 21                                        # keys sorted at once


def check_arguments(G, n, d, max_attempts=1, first_graph=0):
    """ValueError for what no route serves: no simple d-regular graph on n nodes exists (n * d odd, d >= n), or a count that
    makes no sense."""
    if G < 0 or n < 1 or d < 1 or max_attempts < 1 or first_graph < 0:
        raise ValueError(f"bad G={G} n={n} d={d} max_attempts={max_attempts} first_graph={first_graph}")
    if d >= n:
        raise ValueError(f"no simple {d}-regular graph on n={n} nodes (d >= n)")
    if (n * d) % 2:
        raise ValueError(f"n * d = {n} * {d} is odd")


def within_limits(n, d):
    """Whether the pairing routes (device and host) serve (n, d): 13 index bits per key, and an acceptance rate worth a sort."""
    return d <= RRG_MAX_DEGREE and n <= RRG_MAX_NODES and n * d <= RRG_MAX_STUBS


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit values: the four output words."""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # 32 x 32 bits: no overflow
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + w0) & _U32, (k1 + w1) & _U32
    return c0, c1, c2, c3


def pairing_keys(n, d, seed, graph_ids, attempt):
    """The sort keys [len(graph_ids), n * d] uint64 of pairing number `attempt` of the graphs `graph_ids` (ids of the stream:
    first_graph + g)."""
    m = n * d
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids = np.asarray(graph_ids, dtype=np.uint64).reshape(-1, 1)
    shape = (ids.shape[0], m // 2)
    q = np.broadcast_to(np.arange(m // 2, dtype=np.uint64), shape)
    a = np.full(shape, attempt, dtype=np.uint64)
    w = philox4x32_10(q, a, np.broadcast_to(ids & _U32, shape), np.broadcast_to(ids >> np.uint64(32), shape),
                      seed & 0xFFFFFFFF, seed >> 32)
    r = np.empty((shape[0], m), dtype=np.uint64)
    r[:, 0::2] = w[0] | (w[1] << np.uint64(32))
    r[:, 1::2] = w[2] | (w[3] << np.uint64(32))
    return (r & ~_INDEX) | np.arange(m, dtype=np.uint64)


def partners(keys):
    """[p, m] int64: the partner of every stub under the keys - the stubs at the sorted positions 2 i and 2 i + 1 pair up."""
    order = (np.sort(keys, axis=1) & _INDEX).astype(np.int64)
    part = np.empty_like(order)
    np.put_along_axis(part, order[:, 0::2], order[:, 1::2], axis=1)
    np.put_along_axis(part, order[:, 1::2], order[:, 0::2], axis=1)
    return part


def neighbours(part, n, d):
    """[p, n, d] int64: the node at the other end of every stub, each node's d of them ascending."""
    return np.sort((part // d).reshape(-1, n, d), axis=2)


def accepted(nbr):
    """[p] bool: no stub's partner in its own node, no node with two partners in one node."""
    n = nbr.shape[1]
    loop = (nbr == np.arange(n).reshape(1, n, 1)).any(axis=(1, 2))
    double = (np.diff(nbr, axis=2) == 0).any(axis=(1, 2))
    return ~(loop | double)


def random_regular_graphs_host(G, n, d, seed, first_graph=0, max_attempts=4096):
    """G graphs of the stream (seed, n, d) from graph `first_graph` on: (node_ptr [G+1], edge_ptr [G+1], edge_index [2, G n d]
    int64 with LOCAL ids, (src, dst)-sorted per graph; attempts [G] int32: pairings drawn; status [G] int32: RRG_OK, or
    RRG_EXHAUSTED after max_attempts rejected pairings - the columns of such a graph stay 0).  Serves 1 <= d <= 4, n <= 2048,
    n * d <= 8192 (ValueError beyond: the keys have 13 index bits)."""
    G, n, d, max_attempts, first_graph = int(G), int(n), int(d), int(max_attempts), int(first_graph)
    check_arguments(G, n, d, max_attempts, first_graph)
    if not within_limits(n, d):
        raise ValueError(f"n={n} d={d} is beyond the pairing model's limits: d <= {RRG_MAX_DEGREE}, n <= {RRG_MAX_NODES}, "
                         f"n * d <= {RRG_MAX_STUBS}")
    m = n * d
    ei = np.zeros((2, G * m), dtype=np.int64)
    src, dst = ei[0].reshape(G, m), ei[1].reshape(G, m)
    attempts = np.full(G, max_attempts, dtype=np.int32)
    status = np.full(G, RRG_EXHAUSTED, dtype=np.int32)
    rows = np.repeat(np.arange(n, dtype=np.int64), d)
    step = max(1, _CHUNK // m)
    for g0 in range(0, G, step):
        pending = np.arange(g0, min(G, g0 + step))
        for a in range(max_attempts):
            if not pending.size:
                break
            nbr = neighbours(partners(pairing_keys(n, d, seed, first_graph + pending, a)), n, d)
            ok = accepted(nbr)
            done = pending[ok]
            src[done], dst[done] = rows, nbr[ok].reshape(-1, m)
            attempts[done], status[done] = a + 1, RRG_OK
            pending = pending[~ok]
    ptr = np.arange(G + 1, dtype=np.int64)
    return ptr * n, ptr * m, ei, attempts, status
