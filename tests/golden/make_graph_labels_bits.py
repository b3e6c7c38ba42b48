"""Writes tests/golden/graph_labels_bits.npz: the int32 bit patterns of node_out and graph_out and the status that each
instantiation of the graph-property label kernel writes for the cases of tests/graph_labels_classes.py - the wavefront and the
block class of kpgnn_graph_labels on the 53 served fixture graphs and the edge-size cases, kpgnn_graph_labels_large on the 17
graphs of graph_property_large.npz and the boundary cases - with a zlib.crc32 of each case's inputs.  Needs a GPU.

    python tests/golden/make_graph_labels_bits.py --package /path/to/a/built/checkout

Recorded ONCE, from a build of the commit before the three kernels became one template, so that the template is held to the bits
of the kernels it replaced: `--package` names the checkout whose kp_gnn_amd is imported (default: this one).  The bits are a
function of IEEE double add, multiply, divide and square root in a fixed order with contraction off, not of a compiler version.
The fixture holds names, checksums and recorded numbers only."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import graph_labels_classes as GB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.dirname(os.path.dirname(HERE)), help="the built checkout whose kp_gnn_amd records")
    ap.add_argument("--out", default=GB.GOLDEN)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import kp_gnn_amd
    from kp_gnn_amd import ops
    print("recording from", os.path.dirname(kp_gnn_amd.__file__), flush=True)
    arrays = {}
    for cls in GB.CLASSES:
        cases, got = GB.cases_of(cls), GB.run_class(ops, cls)
        status = np.asarray([got[k][2] for k in cases], dtype=np.int32)
        assert not status.any(), (cls, status.tolist())
        arrays[f"{cls}/names"] = np.asarray(list(cases))
        arrays[f"{cls}/crc"] = np.asarray([GB.checksum(v) for v in cases.values()], dtype=np.uint32)
        arrays[f"{cls}/status"] = status
        arrays[f"{cls}/graph"] = np.stack([got[k][1] for k in cases]).astype(np.int32)
        arrays[f"{cls}/node"] = np.concatenate([got[k][0] for k in cases]).astype(np.int32)       # rows in the order of names
        print(f"{cls}: {len(cases)} graphs, {arrays[f'{cls}/node'].shape[0]} nodes", flush=True)
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
