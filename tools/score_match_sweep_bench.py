#!/usr/bin/env python3
"""Particle-level precision / recall curve: one ``match_sweep`` call over T confidence
thresholds against T ``match_pairs`` calls at the same thresholds (the only way to the curve
before the sweep), in one process.

The pairs are those of tools/score_match_bench.py (C2 geometry of repic_amd/synth.py, 900 true
particles: about 900 ground-truth boxes and 900 picks per pair); the thresholds are the
j / T quantiles (j = 0..T-1) of all the picks' confidences, so every step of the sweep adds
about 1 / T of the picks and the loop's calls keep from all of them down to 1 / T.  After a
warm-up of both paths and the comparison of their counts (equal, or nothing is written), the
two alternate for ``--rounds`` rounds.  A round's figures are the wall time of the path (host
layout, upload, launches, copy back; every call ends in a stream synchronise) and its kernel
time from HIP events (RGC_F_TIMING), summed over the T calls of the loop.  Medians are reported.

  python tools/score_match_sweep_bench.py [--pairs 1000] [--thr 16] [--rounds 5] [--out FILE.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--thr", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ji", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_match_sweep_C2.json"))
    a = ap.parse_args()
    from repic_amd import score_detections as sd
    from score_match_bench import make_pairs
    pairs = make_pairs(a.pairs)
    conf = np.concatenate([p[:, 4] for _, p in pairs])
    ts = np.quantile(conf, np.arange(a.thr) / a.thr).tolist()

    def sweep():
        t0 = time.perf_counter()
        counts, ms = sd.match_sweep(pairs, a.ji, ts, timing=True)
        return counts, (time.perf_counter() - t0) * 1e3, ms

    def loop():
        t0 = time.perf_counter()
        counts, ms = [], {}
        for t in ts:
            c, m = sd.match_pairs(pairs, a.ji, conf_thresh=t, timing=True)
            counts.append(c)
            for k, v in m.items():
                ms[k] = ms.get(k, 0.0) + v
        return np.stack(counts, axis=1), (time.perf_counter() - t0) * 1e3, ms

    sd.match_pairs(pairs[:8], a.ji)                                 # code objects
    cs, _, _ = sweep()                                              # warm-up of both paths
    cl, _, _ = loop()
    assert np.array_equal(cs, cl), "match_sweep and the loop of match_pairs disagree"
    rounds = []
    for _ in range(a.rounds):
        _, ws, ks = sweep()
        _, wl, kl = loop()
        rounds.append({"sweep_wall_ms": ws, "loop_wall_ms": wl,
                       "sweep_kernel_ms": ks, "loop_kernel_ms": kl})

    def med(f):
        return float(np.median([f(r) for r in rounds]))
    tot = cs.sum(axis=0)
    res = {"pairs": a.pairs, "n_thr": a.thr, "ji_thresh": a.ji, "conf_threshs": ts,
           "n_gt_mean": float(cs[:, 0, 0].mean()),
           "n_picked_mean_per_thr": cs[:, :, 1].mean(axis=0).tolist(),
           "tp_per_thr": tot[:, 2].tolist(),
           "average_precision_pooled": sd.average_precision(tot),
           "rounds": rounds,
           "sweep_wall_ms_median": med(lambda r: r["sweep_wall_ms"]),
           "loop_wall_ms_median": med(lambda r: r["loop_wall_ms"]),
           "k_score_match_sweep_ms_median":
               med(lambda r: r["sweep_kernel_ms"]["k_score_match_sweep"]),
           "sweep_count_ms_median": med(lambda r: r["sweep_kernel_ms"]["k_score_match_count"]),
           "loop_k_score_match_ms_median": med(lambda r: r["loop_kernel_ms"]["k_score_match"]),
           "loop_count_ms_median": med(lambda r: r["loop_kernel_ms"]["k_score_match_count"])}
    res["wall_speedup"] = res["loop_wall_ms_median"] / res["sweep_wall_ms_median"]
    res["kernel_speedup"] = ((res["loop_k_score_match_ms_median"] + res["loop_count_ms_median"]) /
                             (res["k_score_match_sweep_ms_median"] + res["sweep_count_ms_median"]))
    print(json.dumps({k: v for k, v in res.items() if k not in ("rounds", "conf_threshs")}))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
