#!/usr/bin/env python3
"""Particle-level matching of score_detections: kernel time of one call over a data set, and
the time of the numpy / scipy restatement of the tests for the same pairs on one core.

The pairs have the C2 geometry of repic_amd/synth.py (4096^2 px, 180 px boxes, 90 % of the true
particles kept with 8 % jitter, 10 % false positives) with 900 true particles: picker 0 of a
synthetic micrograph is the ground truth, picker 1 the picks, about 900 boxes each.  After a
warm-up call, ``--rounds`` calls of ``match_pairs`` with RGC_F_TIMING give the two kernel times
from HIP events and the wall time of the whole call (layout, upload, the two launches, copy
back).  The oracle (tests/score_match_util.py: brute-force int64 / f64 edges, then
scipy.sparse.csgraph.maximum_bipartite_matching) runs once, single threaded; its counts are
compared with the device's before anything is written.

  python tools/score_match_bench.py [--pairs 1000] [--rounds 5] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_pairs(n, n_true=900):
    from repic_amd import synth
    cfg = synth.SynthConfig(**dict(synth.CONFIGS["C2"], k=2, n_true=n_true))
    pairs = []
    for mg in synth.batch(cfg, n):
        g, p = ([np.stack([x, y, np.full(len(x), float(cfg.box)), np.full(len(x), float(cfg.box)),
                           s], axis=1) for (x, y, s) in mg])
        pairs.append((g, p))
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ji", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from repic_amd import score_detections as sd
    from score_match_util import edge_matrix, matching_size, rects
    pairs = make_pairs(a.pairs)
    sd.match_pairs(pairs[:8], a.ji)                                # warm-up
    rounds = []
    for _ in range(a.rounds):
        t0 = time.perf_counter()
        counts, ms = sd.match_pairs(pairs, a.ji, timing=True)
        rounds.append({"wall_ms": (time.perf_counter() - t0) * 1e3, **ms})
    t0 = time.perf_counter()
    edges, t_match, want = 0, 0.0, []
    for g, p in pairs:
        E = edge_matrix(rects(g), rects(p), a.ji)
        t1 = time.perf_counter()
        want.append(matching_size(E))
        t_match += time.perf_counter() - t1
        edges += int(E.sum())
    t_oracle = time.perf_counter() - t0
    assert counts[:, 2].tolist() == want, "device and oracle disagree"
    res = {"pairs": a.pairs, "ji_thresh": a.ji,
           "n_gt_mean": float(counts[:, 0].mean()), "n_picked_mean": float(counts[:, 1].mean()),
           "edges": edges, "tp": int(counts[:, 2].sum()),
           "rounds": rounds,
           "k_score_match_ms_median": float(np.median([r["k_score_match"] for r in rounds])),
           "k_score_match_count_ms_median":
               float(np.median([r["k_score_match_count"] for r in rounds])),
           "call_wall_ms_median": float(np.median([r["wall_ms"] for r in rounds])),
           "oracle_one_core_s": t_oracle, "oracle_scipy_matching_only_s": t_match}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
