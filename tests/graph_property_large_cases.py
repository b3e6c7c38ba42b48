"""Graphs of the tests of the graph-property labels' third size class, 65 to 128 nodes (test_graph_property_large*.py,
golden/make_graph_property_large_golden.py): the 17 sparse fixture graphs, the 145 graphs of the overflow argument and the
boundary sizes.  The builders and helpers are graph_property_cases's."""
import os

import numpy as np

import graph_property_cases as GC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_property_large.npz")
BOUNDARY_SIZES = (1, 2, 63, 64, 65, 66, 127, 128)
ARGUMENT_SIZES = (65, 80, 100, 127, 128)


def star(n):
    return [(0, i) for i in range(1, n)]


def ladder(rungs):
    return GC.path(rungs) + GC.path(rungs, rungs) + [(i, i + rungs) for i in range(rungs)]


def grid(r, c):
    return [(a * c + b, a * c + b + 1) for a in range(r) for b in range(c - 1)] + [(a * c + b, a * c + b + c) for a in range(r - 1) for b in range(c)]


def caterpillar(spine, legs):
    """A path of `spine` nodes, each with `legs` leaves: spine * (1 + legs) nodes."""
    return GC.path(spine) + [(i, spine + i * legs + q) for i in range(spine) for q in range(legs)]


def lollipop(clique, n):
    """K_clique and a path of the other n - clique nodes hanging off its last node."""
    return GC.complete(clique) + GC.path(n - clique + 1, clique - 1)


def fixture_cases():
    """name -> (n, edge_index): 17 graphs of 65 to 128 nodes, none dense - the reference's own triple loop labels them."""
    c = {}
    c["path65"], c["path128"] = GC.sym(65, GC.path(65)), GC.sym(128, GC.path(128))
    c["cycle127"], c["cycle66"] = GC.sym(127, GC.cycle(127)), GC.sym(66, GC.cycle(66))
    c["star100"] = GC.sym(100, star(100))
    c["ladder128"] = GC.sym(128, ladder(64))
    c["grid10x10"] = GC.sym(100, grid(10, 10))
    c["caterpillar96"] = GC.sym(96, caterpillar(32, 2))
    c["lollipop100"] = GC.sym(100, lollipop(10, 100))
    c["iso_last65"] = GC.sym(65, GC.cycle(64))                               # node 64, the second word's only bit, is isolated
    c["c63_c65"] = GC.sym(128, GC.cycle(63) + GC.cycle(65, 63))              # two components, the second across the word edge
    rng = np.random.default_rng(20250128)
    for n, p in ((65, 0.1), (66, 0.1), (96, 0.06), (100, 0.05), (127, 0.08), (128, 0.1)):
        c[f"gnp{n}_{p}"] = GC.sym(n, GC.gnp(n, p, rng))
    assert len(c) == 17 and all(64 < n <= 128 for n, _ in c.values())
    return c


def argument_cases():
    """name -> (n, edge_index): 29 graphs at each of 65, 80, 100, 127 and 128 nodes - G(n, p) from 0.02 to 0.95, both cycle
    parities, a path, a star, the complete graph, lollipops, and a clique next to a disjoint path."""
    rng = np.random.default_rng(128)
    c = {}
    for n in ARGUMENT_SIZES:
        for p in (0.02, 0.03, 0.05, 0.08, 0.12, 0.2, 0.35, 0.6, 0.9, 0.95):
            for draw in range(2):
                c[f"gnp{n}_{p}_{draw}"] = GC.sym(n, GC.gnp(n, p, rng))
        c[f"cycle{n}"], c[f"cycle{n - 1}_iso"] = GC.sym(n, GC.cycle(n)), GC.sym(n, GC.cycle(n - 1))
        c[f"path{n}"], c[f"star{n}"], c[f"complete{n}"] = GC.sym(n, GC.path(n)), GC.sym(n, star(n)), GC.sym(n, GC.complete(n))
        c[f"lollipop{n}_half"], c[f"lollipop{n}_10"] = GC.sym(n, lollipop(n // 2, n)), GC.sym(n, lollipop(10, n))
        c[f"k{n - 5}_p5"] = GC.sym(n, GC.complete(n - 5) + GC.path(5, n - 5))
        c[f"k{n // 2}_p{n - n // 2}"] = GC.sym(n, GC.complete(n // 2) + GC.path(n - n // 2, n // 2))
    assert len(c) == 29 * len(ARGUMENT_SIZES) == 145
    return c


def boundary_cases():
    """Each boundary size as a path, a complete graph, a cycle, an edgeless graph and a graph whose last node is isolated (a
    cycle on the others), then G(128, 0.95); complete128 is the dense K128."""
    c = {}
    for n in BOUNDARY_SIZES:
        c[f"path{n}"], c[f"complete{n}"], c[f"cycle{n}"] = GC.sym(n, GC.path(n)), GC.sym(n, GC.complete(n)), GC.sym(n, GC.cycle(n))
        c[f"edgeless{n}"], c[f"isolated{n}"] = GC.sym(n, []), GC.sym(n, GC.cycle(n - 1))
    c["gnp128_0.95"] = GC.sym(128, GC.gnp(128, 0.95, np.random.default_rng(95)))
    return c
