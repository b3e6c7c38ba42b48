#!/usr/bin/env python3
"""Generate tests/golden/resistance_distance_large.pt by running the REFERENCE's own data_utils.resistance_distance on graphs
of 129 to 300 nodes, the sizes csrc/resistance_large.hip serves first.

Run in the build container only (needs the reference checkout, read-only, scipy and networkx):

    python tests/golden/make_rd_large_golden.py

As make_rd_golden.py does, the reference file is imported unmodified and tests/pyg_standin/ supplies the one PyG symbol it
touches here.  Only data is written, the same four fields per case:
    n          node count
    edge_index int16 [2,E] (local ids)
    ref32      float32 [n]: the reference's output (scipy float32 pinv)
    ref64      float64 [n]: the same formula on a float64 pinv of the same scipy Laplacian, computed here
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import networkx as nx  # noqa: E402
import torch  # noqa: E402

from make_rd_golden import case, path, sym  # noqa: E402  (sets up the reference and the stand-in on import)


def main():
    gnm = sorted(nx.gnm_random_graph(191, 382, seed=5).edges())
    assert len(gnm) == 382
    cases = {
        "path130": case(130, path(130)),
        "cycle160": case(160, sym([(i, (i + 1) % 160) for i in range(160)])),
        "star161": case(161, sym([(0, i) for i in range(1, 161)])),
        "complete150": case(150, sym([(i, j) for i in range(150) for j in range(i + 1, 150)])),
        # one edge twice (both directions) and one self-loop, which scipy's laplacian ignores
        "gnm191_dup_loop": case(191, torch.cat([sym(gnm), sym([gnm[7]]), torch.tensor([[90], [90]])], dim=1)),
        # nodes 0 .. 127 a path (node 0 in it), 128 .. 255 a second path, 256 isolated
        "two_paths_plus_isolated257": case(257, sym([(i, i + 1) for i in range(127)] + [(i, i + 1) for i in range(128, 255)])),
        "node0_isolated140": case(140, sym([(i, i + 1) for i in range(1, 139)] + [(139, 1)])),
        "directed_cycle200": case(200, torch.tensor([[i for i in range(200)], [(i + 1) % 200 for i in range(200)]])),
    }
    dst = os.path.join(HERE, "resistance_distance_large.pt")
    torch.save(cases, dst)
    worst = max(float((c["ref32"].double() - c["ref64"]).abs().max()) for c in cases.values())
    print("wrote %s: %d cases, %d bytes, largest |ref32 - ref64| = %.3g" % (dst, len(cases), os.path.getsize(dst), worst))


if __name__ == "__main__":
    main()
