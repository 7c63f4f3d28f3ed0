#!/usr/bin/env python3
"""score_detections threshold sweep against a loop of single-threshold calls.

64 micrograph pairs like the mg4096 goldens (4096^2 px, 300 ground-truth boxes and 330 picks
of 180 px) are scored at T in {1, 16, 64} thresholds two ways in one process: one
``score_sweep`` call (k_score_sweep), and T ``score_pairs`` calls (k_score_raster, the path
that existed before the sweep).  After a warm-up of both, the two alternate for five rounds; a
round's figure is the kernel time from HIP events (RGC_F_TIMING), summed over the T calls of
the loop.  The results of the two are compared before anything is printed.

Then the command line end to end: ``--sweep`` with 16 thresholds against 16 runs with ``-c``,
each a fresh process on the same BOX files (wall clock).

  python tools/score_sweep_bench.py [--pairs 64] [--rounds 5] [--cli-pairs 16]
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "repic-copy_amd")
sys.path.insert(0, PKG)
sys.path.insert(0, ROOT)

W = H = 4096
BOX = 180


def make_pairs(n, seed=0):
    rng = np.random.default_rng(seed)

    def boxes(m):
        xy = np.rint(rng.uniform(0, [W - BOX, H - BOX], (m, 2)))
        return np.concatenate([xy, np.full((m, 2), float(BOX)), rng.uniform(0, 1, (m, 1))], axis=1)
    return [(boxes(300), boxes(330)) for _ in range(n)]


def kernel_rounds(sd, pairs, T, rounds):
    ts = np.linspace(0.0, 1.0, T).tolist() if T > 1 else [0.3]
    kw = {"mrc_w": W, "mrc_h": H}

    def sweep():
        t0 = time.perf_counter()
        res, kt = sd.score_sweep(pairs, ts, timing=True, **kw)
        return res, kt["k_score_sweep"], (time.perf_counter() - t0) * 1e3

    def loop():
        t0 = time.perf_counter()
        res, ms = [], 0.0
        for t in ts:
            r, kt = sd.score_pairs(pairs, conf_thresh=t, timing=True, **kw)
            res.append(r)
            ms += kt["k_score_raster"]
        return res, ms, (time.perf_counter() - t0) * 1e3
    a, _, _ = sweep()                                  # warm-up of both, and the comparison
    b, _, _ = loop()
    for i in range(len(pairs)):
        for j in range(T):
            assert a[i][j] == b[j][i], (T, i, j, a[i][j], b[j][i])
    out = {"sweep": [], "loop": []}
    for _ in range(rounds):
        out["sweep"].append(sweep()[1:])
        out["loop"].append(loop()[1:])
    return out


def cli_times(pairs, T):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    ts = [repr(float(t)) for t in np.linspace(0.0, 1.0, T)]
    with tempfile.TemporaryDirectory() as d:
        g, p = [], []
        for i, (gt, pk) in enumerate(pairs):
            for lst, a, nm in ((g, gt, f"gt/mg{i:03d}.box"), (p, pk, f"pk/mg{i:03d}_picks.box")):
                path = os.path.join(d, nm)
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "w") as f:
                    for r in a:
                        f.write(f"{int(r[0])}\t{int(r[1])}\t{BOX}\t{BOX}\t{float(r[4])!r}\n")
                lst.append(path)
        base = [sys.executable, "-m", "repic_amd.score_detections", "-g"] + g + ["-p"] + p + [
            "--width", str(W), "--height", str(H)]

        def run(extra, out):
            t0 = time.perf_counter()
            subprocess.run(base + extra + ["--out_dir", os.path.join(d, out)], check=True, env=env)
            return time.perf_counter() - t0
        run(["-c", "0.5"], "warm")                     # page cache, code object
        sweep = run(["--sweep"] + ts, "sweep")
        loop = [run(["-c", t], f"c{j}") for j, t in enumerate(ts)]
    return sweep, loop


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli-pairs", type=int, default=16)
    a = ap.parse_args()
    from repic_amd import score_detections as sd
    pairs = make_pairs(a.pairs)
    print(f"# {a.pairs} pairs of {W}x{H} px, 300 ground-truth boxes + 330 picks of {BOX} px; "
          f"kernel ms from HIP events, {a.rounds} alternating rounds after a warm-up")
    print("# T  path   kernel ms per round                      min     max   | call wall ms (median)")
    for T in (1, 16, 64):
        r = kernel_rounds(sd, pairs, T, a.rounds)
        for name in ("sweep", "loop"):
            k = [v[0] for v in r[name]]
            wall = float(np.median([v[1] for v in r[name]]))
            print(f"{T:3d}  {name:5s}  " + " ".join(f"{v:7.3f}" for v in k) +
                  f"   {min(k):7.3f} {max(k):7.3f}  | {wall:9.2f}")
        s, lp = [v[0] for v in r["sweep"]], [v[0] for v in r["loop"]]
        print(f"{T:3d}  sweep slowest {max(s):.3f} ms vs loop fastest {min(lp):.3f} ms: "
              f"{'sweep faster' if max(s) < min(lp) else 'SWEEP NOT FASTER'} "
              f"(x{min(lp) / max(s):.2f})", flush=True)
    if a.cli_pairs:
        sweep, loop = cli_times(pairs[:a.cli_pairs], 16)
        print(f"# command line, {a.cli_pairs} pairs (BOX files on disk), fresh process per run")
        print(f"cli  --sweep with 16 thresholds: {sweep:.2f} s")
        print(f"cli  16 runs with -c: {sum(loop):.2f} s (per run min {min(loop):.2f} "
              f"max {max(loop):.2f})")


if __name__ == "__main__":
    main()
