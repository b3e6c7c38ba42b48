#!/usr/bin/env python3
"""Generate tests/golden/resistance_distance.pt by running the REFERENCE's own data_utils.resistance_distance.

Run in the build container only (needs the reference checkout, read-only, and scipy):

    python tests/golden/make_rd_golden.py

As make_golden.py does, the reference file is imported unmodified and tests/pyg_standin/ supplies the one PyG symbol it
touches here (to_scipy_sparse_matrix, which fills float32 ones as PyG's does).  Only data is written.  Per case:
    n          node count
    edge_index int16 [2,E] (local ids)
    ref32      float32 [n]: the reference's output (scipy float32 pinv)
    ref64      float64 [n]: the same formula on a float64 pinv of the same scipy Laplacian, computed here
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("KPGNN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(HERE, "..", "pyg_standin"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse as ssp  # noqa: E402
import scipy.sparse.csgraph  # noqa: E402, F401
import torch  # noqa: E402
from torch_geometric.data import Data  # noqa: E402  (stand-in)

import data_utils as ref_data_utils  # noqa: E402  (reference)

torch.set_num_threads(1)


def sym(pairs):
    e = [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]
    return torch.tensor(e, dtype=torch.long).t().reshape(2, -1)


def path(n):
    return sym([(i, i + 1) for i in range(n - 1)])


def ref64_of(n, ei):
    adj = ssp.coo_matrix((np.ones(ei.shape[1], dtype=np.float64), (ei[0].numpy(), ei[1].numpy())), (n, n)).tocsr()
    Lp = np.linalg.pinv(ssp.csgraph.laplacian(adj).toarray())
    d = np.diagonal(Lp)
    return torch.from_numpy(np.ascontiguousarray(Lp[0, 0] + d - Lp[0, :] - Lp[:, 0]))


def case(n, ei):
    ei = ei.reshape(2, -1).long()
    ref32 = ref_data_utils.resistance_distance(Data(edge_index=ei, num_nodes=n)).rd
    assert ref32.dtype == torch.float32 and tuple(ref32.shape) == (n, 1)
    return {"n": torch.tensor(n), "edge_index": ei.to(torch.int16), "ref32": ref32.reshape(-1).clone(), "ref64": ref64_of(n, ei)}


def main():
    empty = torch.zeros((2, 0), dtype=torch.long)
    cases = {
        "single": case(1, empty),
        "isolated3": case(3, empty),
        "path5": case(5, path(5)),
        "two_components_plus_isolated": case(8, sym([(0, 1), (1, 2), (2, 0), (2, 3), (4, 5), (5, 6)])),
        "node0_isolated": case(5, sym([(1, 2), (2, 3), (3, 4), (4, 1)])),
        "duplicated_edge": case(4, torch.cat([path(4), sym([(1, 2)])], dim=1)),
        "self_loop": case(4, torch.cat([path(4), torch.tensor([[2], [2]])], dim=1)),
        "complete20": case(20, sym([(i, j) for i in range(20) for j in range(i + 1, 20)])),
        "cycle37": case(37, sym([(i, (i + 1) % 37) for i in range(37)])),
        "directed_cycle3": case(3, torch.tensor([[0, 1, 2], [1, 2, 0]])),
    }
    for n in (32, 33, 64, 65, 128, 129):
        cases["path%d" % n] = case(n, path(n))
    from kp_gnn_amd import khop_transform as KT
    node_ptr, edge_ptr, ei, ea, _ = KT.synth_molecules(64, 11)
    out = KT.khop_batch(node_ptr, edge_ptr, ei, ea, 4, 50, 6, 3, 50, 50, "spd")
    kp, kei = out["edge_ptr"].numpy(), out["edge_index"]
    for g in range(64):
        n0, n1 = int(node_ptr[g]), int(node_ptr[g + 1])
        cases["mol%02d" % g] = case(n1 - n0, kei[:, kp[g]:kp[g + 1]] - n0)
    dst = os.path.join(HERE, "resistance_distance.pt")
    torch.save(cases, dst)
    worst = max(float((c["ref32"].double() - c["ref64"]).abs().max()) for c in cases.values())
    print("wrote %s: %d cases, %d bytes, largest |ref32 - ref64| = %.3g" % (dst, len(cases), os.path.getsize(dst), worst))


if __name__ == "__main__":
    main()
