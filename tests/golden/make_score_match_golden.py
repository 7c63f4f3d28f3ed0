#!/usr/bin/env python3
"""Golden fixtures for the particle-level matching of score_detections, produced by the REAL
reference in THIS container (CPU only).

Test infrastructure only (the reference never travels to the GPU box).  Imports
/root/reference/repic/commands/get_cliques.py and calls its
``get_jaccard(set_a, set_b, box_size, threshold)`` (get_cliques.py:59-69) on the ground truth
and the picks of every case: equal squares at integer coordinates, the domain where the
reference defines the edges.  Records

* ``score_match/cases.npz``: boxes (x, y, w, h, conf) of every case;
* ``score_match/meta.json``: box size, the thresholds (float.hex) and per threshold the
  reference's edge list as (ground-truth index, pick index) and the size of a maximum matching
  of that list (scipy.sparse.csgraph.maximum_bipartite_matching).

  python tests/golden/make_score_match_golden.py
"""
from __future__ import annotations

import json
import math
import os
import shutil
import sys

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "score_match")
sys.path.insert(0, "/root/reference")

import repic.commands.get_cliques as ref  # noqa: E402  (reference module)


def _xy(rng, n, field, B):
    return rng.integers(0, field - B + 1, (n, 2))


def cases():
    """-> (name, box size, gt (n, 2) int, picks (n, 2) int, thresholds)"""
    rng = np.random.default_rng(41)
    z = np.zeros((0, 2), np.int64)
    out = []
    # a chain: pick i joins boxes i and i + 1, the last pick only box 0.  Lowest-index greedy
    # leaves it out; the one augmenting path runs through the whole chain.
    g = np.stack([100 * np.arange(300), np.zeros(300, np.int64)], axis=1)
    p = np.stack([np.concatenate([100 * np.arange(299) + 50, [-50]]), np.zeros(300, np.int64)],
                 axis=1)
    out.append(("chain300", 100, g, p, [0.3]))
    g = _xy(rng, 300, 4096, 180)
    p = np.concatenate([g, g[rng.choice(300, 30, replace=False)]]) + rng.integers(-40, 41, (330, 2))
    out.append(("jitter", 180, g, p[rng.permutation(330)], [0.3]))
    out.append(("dense_t0", 64, _xy(rng, 200, 1024, 64), _xy(rng, 260, 1024, 64), [0.0]))
    g = _xy(rng, 150, 1200, 60)
    out.append(("strict", 60, g, (g + rng.integers(-12, 13, (150, 2)))[rng.permutation(150)],
                [0.6]))
    # B = 10: a shift of 5 px is I / U = 50 / 150, of 6 px 40 / 160
    g = np.array([[0, 0], [100, 0], [200, 0], [300, 0], [400, 0]])
    p = np.array([[5, 0], [100, 5], [206, 0], [300, -6], [400, 0]])
    third = 1.0 / 3.0
    out.append(("ties", 10, g, p, [third, math.nextafter(third, 0.0), 0.25,
                                   math.nextafter(0.25, 0.0)]))
    out.append(("empty_picks", 50, _xy(rng, 12, 400, 50), z, [0.3]))
    out.append(("empty_gt", 50, z, _xy(rng, 12, 400, 50), [0.3]))
    out.append(("both_empty", 50, z, z, [0.3]))
    return out


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    meta, arrays = {"cases": []}, {}
    for name, B, g, p, ts in cases():
        set_a = [(int(x), int(y), 1.0, i) for i, (x, y) in enumerate(g.tolist())]
        set_b = [(int(x), int(y), 1.0, i) for i, (x, y) in enumerate(p.tolist())]
        edges, sizes = [], []
        for t in ts:
            vals = ref.get_jaccard(set_a, set_b, B, t)
            e = sorted((int(v[3]), int(v[7])) for v in vals)
            m = 0
            if e:
                gi, pi = zip(*e)
                M = csr_matrix((np.ones(len(e), np.int8), (pi, gi)), shape=(len(p), len(g)))
                m = int((maximum_bipartite_matching(M, perm_type="column") >= 0).sum())
            edges.append(e)
            sizes.append(m)
        for key, a in ((name + "_gt", g), (name + "_pk", p)):
            n = len(a)
            arrays[key] = np.concatenate([a.astype(np.float64).reshape(n, 2),
                                          np.full((n, 2), float(B)), np.ones((n, 1))], axis=1)
        meta["cases"].append({"name": name, "box_size": B,
                              "thresh_hex": [float(t).hex() for t in ts],
                              "edges": edges, "sizes": sizes})
        print(name, [len(e) for e in edges], sizes)
    np.savez_compressed(os.path.join(OUT, "cases.npz"), **arrays)
    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print(f"wrote {len(meta['cases'])} cases to {OUT}")


if __name__ == "__main__":
    main()
