"""The random graphs of the graph- and node-property dataset on the host: the definition of include/kpgnn.h
(kpgnn_property_graphs_generate) written out in numpy - Philox4x32-10 on uint64 arrays, integer comparisons only - and
therefore the specification the kernel of csrc/property_graphs.hip is tested against, bit for bit.  The laws are those of the
reference's datasets/graph_generation.py generate_graph (ten graph types, a uniform relabelling, `randomize`, a retry while a
node has no neighbour); the stream is Philox, so the graphs are another draw.  Graph g of a call is a function of (seed,
first_graph + g, n_g, graph_type, flags) alone.  Graphs of one size and type go through every stage together; the two
sequential walks (Barabasi-Albert's attachment, the tree's degree swaps) are Python loops over words drawn in chunks.
Host only: numpy, never the HIP library (of _lib, its constants)."""
import numpy as np

from ._lib import PG_EXHAUSTED, PG_MAX_NODES, PG_MIN_NODES, PG_OK, PG_STREAMS, PG_TREE_SWAPS, PG_TYPES
from .regular_graphs import philox4x32_10

TYPE_NAMES = {v: k for k, v in PG_TYPES.items()}
# the reference's MIXTURE as cumulative twentieths: x = below(TYPE word, 20) picks the first type with x < bound
MIXTURE = (("ERDOS_RENYI", 4), ("BARABASI_ALBERT", 8), ("GRID", 9), ("CAVEMAN", 10), ("TREE", 13), ("LADDER", 14), ("LINE", 15),
           ("STAR", 16), ("CATERPILLAR", 18), ("LOBSTER", 20))
_U32 = np.uint64(0xFFFFFFFF)
_CHUNK = 512                                            # words a sequential walk draws at once


def type_id(graph_type):
    """The id of a type given by name, id or an Enum member with such a value."""
    t = PG_TYPES.get(graph_type) if isinstance(graph_type, str) else int(getattr(graph_type, "value", graph_type))
    if t not in TYPE_NAMES:
        raise ValueError(f"unknown graph type {graph_type!r}")
    return t


def check_nodes(nodes):
    """The node counts as an int64 array; ValueError for a size outside [2, 128]."""
    nodes = np.atleast_1d(np.asarray(nodes, dtype=np.int64))
    if nodes.ndim != 1:
        raise ValueError("nodes is an int or a sequence of node counts")
    bad = np.flatnonzero((nodes < PG_MIN_NODES) | (nodes > PG_MAX_NODES))
    if bad.size:
        raise ValueError(f"graph {int(bad[0])} has {int(nodes[bad[0]])} nodes, outside [{PG_MIN_NODES}, {PG_MAX_NODES}]")
    return nodes


def words(stream, seed, ids, attempt, index):
    """(w0, w1, w2, w3), uint64 arrays [len(ids), len(index)]: W(stream, attempt, index) of the graphs `ids`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1, 1)
    index = np.asarray(index, dtype=np.uint64).reshape(1, -1)
    shape = (ids.shape[0], index.shape[1])
    c1 = np.full(shape, (int(attempt) << 4) | PG_STREAMS[stream], dtype=np.uint64)
    return philox4x32_10(np.broadcast_to(index, shape), c1, np.broadcast_to(ids & _U32, shape),
                         np.broadcast_to(ids >> np.uint64(32), shape), seed & 0xFFFFFFFF, seed >> 32)


def below(w, L):
    """((uint64) w * L) >> 32: uniform in [0, L), bias below L / 2^32."""
    return ((w * np.asarray(L, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def degrees(v, n):
    """round(paretovariate(2)) of 32-bit words, at most n: the smallest k >= 1 with v (2k+1)^2 < 2^32 ((2k+1)^2 - 4)."""
    v = np.asarray(v, dtype=np.uint64)
    k = np.full(v.shape, n, dtype=np.int64)
    todo = np.ones(v.shape, dtype=bool)
    for c in range(1, n):
        q = np.uint64((2 * c + 1) ** 2)
        hit = todo & (v * q < (q - np.uint64(4)) << np.uint64(32))
        k[hit] = c
        todo &= ~hit
        if not todo.any():
            break
    return k


def graph_type_of(seed, ids):
    """[len(ids)] int32: the type a RANDOM graph of each id takes (kept over its attempts)."""
    x = below(words("TYPE", seed, ids, 0, [0])[0][:, 0], 20)
    bounds = np.array([b for _, b in MIXTURE])
    return np.array([PG_TYPES[t] for t, _ in MIXTURE], dtype=np.int32)[np.searchsorted(bounds, x, side="right")]


def grid_rows(n):
    """The largest divisor of n not above sqrt(n)."""
    return max(i for i in range(1, n + 1) if i * i <= n and n % i == 0)


class _Walk:
    """Word t = 0, 1, .. of one graph's stream for a sequential walk, drawn _CHUNK at a time."""

    def __init__(self, stream, seed, gid, attempt):
        self.args, self.buf, self.base = (stream, seed, [gid], attempt), [], 0

    def __call__(self, t):
        while t >= self.base + len(self.buf):
            self.base += len(self.buf)
            self.buf = words(*self.args, np.arange(self.base, self.base + _CHUNK))[0][0].tolist()
        return self.buf[t - self.base]


def _from_parents(par):
    """[p, n, n] bool from the parent of every node but 0 (par[:, 0] is ignored)."""
    p, n = par.shape
    C = np.zeros((p, n, n), dtype=bool)
    g, i = np.meshgrid(np.arange(p), np.arange(1, n), indexing="ij")
    C[g, i, par[:, 1:]] = True
    return C | C.transpose(0, 2, 1)


def _fixed(n, t):
    """The canonical adjacency of the five types that draw nothing."""
    C = np.zeros((n, n), dtype=bool)
    i = np.arange(n)
    if t == "GRID":
        c = n // grid_rows(n)
        C[i[i % c != 0], i[i % c != 0] - 1] = True
        C[i[i >= c], i[i >= c] - c] = True
    elif t == "CAVEMAN":
        k = n // grid_rows(n)
        C = (i[:, None] // k == i[None, :] // k) & (i[:, None] > i[None, :])
    elif t == "LADDER":
        h = n // 2
        on = (i != 0) & (i != h) & (i < 2 * h)
        C[i[on], i[on] - 1] = True
        C[i[(i >= h) & (i < 2 * h)], i[(i >= h) & (i < 2 * h)] - h] = True
        if n % 2:
            C[n - 1, 0] = True
    elif t == "LINE":
        C[i[1:], i[1:] - 1] = True
    elif t == "STAR":
        C[i[1:], 0] = True
    return C | C.T


def _barabasi_albert(n, m, draw):
    """The lower neighbours of every node as bit masks: networkx 3.x's procedure on the words draw(t)."""
    low = [0] + [1] * m + [0] * (n - m - 1)
    rep = [0] * m + list(range(1, m + 1))
    t = 0
    for s in range(m + 1, n):
        mask = cnt = 0
        while cnt < m:
            x = rep[(draw(t) * len(rep)) >> 32]
            t += 1
            if not (mask >> x) & 1:
                mask, cnt = mask | (1 << x), cnt + 1
        low[s] = mask
        rep += [j for j in range(n) if (mask >> j) & 1] + [s] * m
    return low


def tree_sequence(n, seed, gid, attempt):
    """The degree sequence of the TREE of this attempt (a list summing to 2n - 2), or None when PG_TREE_SWAPS swaps did not
    reach one; and the swaps made."""
    deg = degrees(words("TREE", seed, [gid], attempt, np.arange(n))[0][0], n).tolist()
    total, draw, s = sum(deg), _Walk("TREE", seed, gid, attempt), 0
    while total != 2 * n - 2:
        if s == PG_TREE_SWAPS:
            return None, s
        pos, v, new = (draw(n + 2 * s) * n) >> 32, draw(n + 2 * s + 1), 1
        while new < n and not v * (2 * new + 1) ** 2 < ((2 * new + 1) ** 2 - 4) << 32:
            new += 1
        total, deg[pos], s = total + new - deg[pos], new, s + 1
    return deg, s


def tree_parents(deg):
    """nx.degree_sequence_tree(deg) as the parent of every node: a path 0 .. I+1 whose inner nodes take the degrees above 1
    ascending, the leaves numbered after it."""
    inner = sorted(d for d in deg if d > 1)
    nb = len(inner) + 2
    par = list(range(-1, nb - 1))
    for b, d in enumerate(inner, start=1):
        par += [b] * (d - 2)
    return par


def structure(n, graph_type, seed, gid, attempt, param=None):
    """The canonical adjacency [n, n] bool of attempt `attempt` of graph `gid` (None for a rejected TREE).  param forces p of
    ERDOS_RENYI (a fraction in [0, 1]), m of BARABASI_ALBERT, or B of CATERPILLAR and LOBSTER."""
    C, ok = structures(n, type_id(graph_type), seed, [gid], attempt, param)
    return C[0] if ok[0] else None


def structures(n, t, seed, ids, attempt, param=None):
    """([p, n, n] bool, [p] bool): the canonical adjacencies of one attempt of the graphs `ids`, and which of them exist."""
    ids = np.asarray(ids, dtype=np.int64)
    p, name = ids.shape[0], TYPE_NAMES[t]
    ok = np.ones(p, dtype=bool)
    if name in ("GRID", "CAVEMAN", "LADDER", "LINE", "STAR"):
        return np.broadcast_to(_fixed(n, name), (p, n, n)), ok
    if name == "ERDOS_RENYI":
        prob = words("PARAM", seed, ids, attempt, [0])[0] if param is None else np.full((p, 1), int(param * 2 ** 32), dtype=np.uint64)
        iu, ju = np.tril_indices(n, -1)                 # pair q = i (i - 1) / 2 + j in this order
        C = np.zeros((p, n, n), dtype=bool)
        C[:, iu, ju] = words("PAIR", seed, ids, attempt, np.arange(iu.size))[2] < prob
        return C | C.transpose(0, 2, 1), ok
    if name == "BARABASI_ALBERT":
        m = 1 + below(words("PARAM", seed, ids, attempt, [0])[0][:, 0], n - 1) if param is None else np.full(p, int(param))
        C = np.zeros((p, n, n), dtype=bool)
        for g in range(p):
            low = _barabasi_albert(n, int(m[g]), _Walk("BA", seed, int(ids[g]), attempt))
            C[g] = [[(low[i] >> j) & 1 for j in range(n)] for i in range(n)]
        return C | C.transpose(0, 2, 1), ok
    par = np.zeros((p, n), dtype=np.int64)
    if name == "TREE":
        for g in range(p):
            deg, _ = tree_sequence(n, seed, int(ids[g]), attempt)
            ok[g] = deg is not None
            if ok[g]:
                par[g] = tree_parents(deg)
        return _from_parents(par), ok
    w = words("PARAM", seed, ids, attempt, [0, 1])[0]
    B = (1 + below(w[:, 0], n - 1) if param is None else np.full(p, int(param)))[:, None]
    F = B + 1 + below(w[:, 1:2], n - B) if name == "LOBSTER" else np.full((p, 1), n)
    i = np.arange(n)[None, :]
    att = words("ATTACH", seed, ids, attempt, np.arange(n))[0]
    par = np.where(i < B, i - 1, np.where(i < F, below(att, np.broadcast_to(B, att.shape)),
                                          B + below(att, np.broadcast_to(np.maximum(F - B, 1), att.shape))))
    return _from_parents(par), ok


def relabelling(n, seed, ids, a):
    """[p, n] int64: inv[g, rank] = the canonical node of graph ids[g] that attempt `a` gives the label `rank` - the order of
    the nodes' SHUFFLE keys."""
    w = words("SHUFFLE", seed, ids, a, np.arange(n))
    keys = ((w[0] | (w[1] << np.uint64(32))) & ~np.uint64(127)) | np.arange(n, dtype=np.uint64)
    return np.argsort(keys, axis=1)


def attempts(n, t, seed, ids, a, randomize=True, shuffle=True, param=None):
    """([p, n, n] bool, [p] bool): the adjacencies attempt `a` of the graphs `ids` ends with - accepted or not - and which of
    them exist (a TREE whose swaps ran out does not)."""
    ids = np.asarray(ids, dtype=np.int64)
    C, ok = structures(n, t, seed, ids, a, param)
    p = ids.shape[0]
    if shuffle:
        inv = relabelling(n, seed, ids, a)
        A = C[np.arange(p)[:, None, None], inv[:, :, None], inv[:, None, :]]
    else:
        A = np.array(C)
    if randomize:
        iu, ju = np.tril_indices(n, -1)
        w = words("PAIR", seed, ids, a, np.arange(iu.size))
        t2 = (w[0] + w[1]).astype(np.int64)             # 33 bits
        has = A[:, iu, ju]
        e = has.sum(axis=1, dtype=np.int64)[:, None]
        r = iu.size - e
        few = e <= r
        stays = np.where(few, 10 * t2 < (9 << 33), 10 * t2 * e < ((10 * e - r) << 33))
        appears = np.where(few, 10 * t2 * r < (e << 33), 10 * t2 < (1 << 33))
        A = np.zeros((p, n, n), dtype=bool)
        A[:, iu, ju] = np.where(has, stays, appears)
        A |= A.transpose(0, 2, 1)
    return A, ok


def attempt(n, graph_type, seed, gid, a, randomize=True, shuffle=True, param=None):
    """The adjacency [n, n] bool attempt `a` of graph `gid` ends with, accepted or not (None for a rejected TREE)."""
    A, ok = attempts(n, type_id(graph_type), seed, [gid], a, randomize, shuffle, param)
    return A[0] if ok[0] else None


def property_graphs_host(nodes, seed, graph_type, first_graph=0, max_attempts=4096, randomize=True, shuffle=True):
    """The graphs first_graph .. of the stream `seed` with the node counts `nodes` (an int or a sequence): (node_ptr [G+1],
    edge_ptr [G+1], edge_index [2, E] int64 with LOCAL ids, (src, dst)-sorted per graph, features [N] float32, source [G],
    types [G], attempts [G], status [G], the last four int32).  A graph still without an accepted attempt after max_attempts
    is PG_EXHAUSTED: no edges, features 0, source 0.  ValueError for a size outside [2, 128]."""
    nodes = check_nodes(nodes)
    t0, first_graph, max_attempts = type_id(graph_type), int(first_graph), int(max_attempts)
    if max_attempts < 1 or max_attempts > 1 << 27 or first_graph < 0:
        raise ValueError(f"bad max_attempts={max_attempts} first_graph={first_graph}")
    G = nodes.shape[0]
    ids = first_graph + np.arange(G, dtype=np.int64)
    types = graph_type_of(seed, ids) if t0 == PG_TYPES["RANDOM"] else np.full(G, t0, dtype=np.int32)
    node_ptr = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
    features = np.zeros(int(node_ptr[-1]), dtype=np.float32)
    source, tried = np.zeros(G, dtype=np.int32), np.full(G, max_attempts, dtype=np.int32)
    status = np.full(G, PG_EXHAUSTED, dtype=np.int32)
    edges = [np.zeros((2, 0), dtype=np.int64)] * G
    for n, t in sorted(set(zip(nodes.tolist(), types.tolist()))):
        pending = np.flatnonzero((nodes == n) & (types == t))
        for a in range(max_attempts):
            if not pending.size:
                break
            A, ok = attempts(n, t, seed, ids[pending], a, randomize, shuffle)
            ok &= A.any(axis=2).all(axis=1)
            done = pending[ok]
            if done.size:
                feat = (words("FEATURE", seed, ids[done], a, np.arange(n))[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
                src = below(words("SOURCE", seed, ids[done], a, [0])[0][:, 0], n)
                for k, g in enumerate(done):
                    features[node_ptr[g]:node_ptr[g + 1]] = feat[k]
                    edges[g] = np.stack(np.nonzero(A[ok][k])).astype(np.int64)
                source[done], tried[done], status[done] = src, a + 1, PG_OK
            pending = pending[~ok]
    edge_ptr = np.concatenate([[0], np.cumsum([e.shape[1] for e in edges])]).astype(np.int64)
    edge_index = np.concatenate(edges, axis=1) if G else np.zeros((2, 0), dtype=np.int64)
    return node_ptr, edge_ptr, edge_index, features, source, types, tried, status
