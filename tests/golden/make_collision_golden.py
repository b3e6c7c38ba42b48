"""Writes tests/golden/collisions.npz: the inputs of tests/collision_cases.golden_inputs() and, for each, what the reference's
compute_simulation_collisions (run_simulation.py:165-178) answers on the CPU - the count (ratio=False) and the rate (ratio=True).

    python tests/golden/make_collision_golden.py --reference /path/to/reference/checkout

The reference's module cannot be imported (it parses the command line and starts the simulation on import), so its file is
parsed and that ONE function definition is compiled and executed in memory, with torch as its only global.  Nothing of the
reference's text is written anywhere: the fixture holds inputs and recorded numbers."""
import argparse
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import collision_cases as CC  # noqa: E402


def reference_function(path, name="compute_simulation_collisions"):
    tree = ast.parse(open(path).read(), filename=path)
    defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(defs) == 1, f"{name} not found once in {path}"
    ns = {"torch": torch}
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory that holds the reference's run_simulation.py")
    ap.add_argument("--out", default=os.path.join(HERE, "collisions.npz"))
    args = ap.parse_args()
    fn = reference_function(os.path.join(args.reference, "run_simulation.py"))
    arrays = {}
    for name, o in CC.golden_inputs().items():
        arrays[name + "/x"] = o.numpy()
        arrays[name + "/n_collision"] = np.int64(fn(o, ratio=False))
        arrays[name + "/ratio"] = np.float64(fn(o, ratio=True))
        upper, diag, band = CC.f64_counts(o)
        print(f"{name}: reference n_collision {int(arrays[name + '/n_collision'])} ratio {float(arrays[name + '/ratio']):.6f}; "
              f"float64 upper {upper} diag {diag} -> {CC.n_collision(upper, diag, o.shape[0])}, band_pairs {band}")
    np.savez_compressed(args.out, **arrays)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
