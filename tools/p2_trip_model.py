#!/usr/bin/env python3
"""CPU model of the fused kernel's P2 inner-loop trip counts (rgc_fused.hip: pairs_count*).

A thread owns one box per round; its candidates are the 2 (K - 1 - p) stencil ranges of the
higher pickers' grids.  A wave pays, per loop, the longest trip count among its 64 lanes, so
the loop shape decides how many wave iterations the same candidates cost:

  ranges     one inner loop per range:         sum_r max_lanes len_r
  per grid   one loop per target grid:         sum_g max_lanes (len_g0 + len_g1)
  flattened  one loop per box:                 max_lanes sum_r len_r
  perfect    candidates dealt evenly to lanes: ceil(sum_lanes sum_r len_r / 64)

The model restates the grid plan (tools/stencil_check.plan), the (picker, cell, index)
counting sort, the half-column stencil and the boustrophedon thread-to-box order, runs them on
`synth` micrographs (seed 0) and prints wave iterations per micrograph.  Plain numpy, no GPU.

  python tools/p2_trip_model.py [--config C2] [--threads 512] [--micrographs 40] [--frac]

--degrees reports what the list write that follows the count in the same pass works on: the
forward degree (edges to higher pickers, brute force over the micrograph) of the box each lane
holds.  A wave-round is one wave in one round, i.e. one aligned block of 64 sorted positions:
  boxes > 2 edges      boxes whose targets the count cannot keep packed (they walk their mask)
  wave-rounds, slow    wave-rounds that hold a box, and those that hold a box with > 2 edges
  write trips          sum over wave-rounds of the largest forward degree (write-loop trips)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from repic_amd import synth  # noqa: E402
from stencil_check import plan  # noqa: E402

f32 = np.float32
# the workgroup size the host picks for the bench configs (rgc_run.cpp: plan_fused)
DEFAULT_THREADS = {"C2": 512, "C3": 1024, "C4": 768, "C5": 1024}


def box_ranges(mg, B):
    """Stencil range lengths of every box in sorted-position order: (len [n, K-1, 2], p [n],
    order [n]).  Axis 1 of len is the ordinal of the target grid (picker p + 1 + j), as the
    kernel's q loop; order[t] is the index (pickers concatenated) of the box at position t."""
    K = len(mg)
    xs = np.concatenate([t[0] for t in mg]).astype(np.float64)
    ys = np.concatenate([t[1] for t in mg]).astype(np.float64)
    pk = np.concatenate([np.full(len(t[0]), p) for p, t in enumerate(mg)])
    n = len(xs)
    mnx, mny, icl, icly, gx, gy = plan(xs, ys, B, n, K)
    u = (xs - mnx).astype(f32) * f32(icl)
    cx = np.minimum(np.floor(u).astype(int), gx - 1)
    cy = np.minimum(np.floor((ys - mny).astype(f32) * f32(icly)).astype(int), gy - 1)
    nc = gx * gy
    key = pk * nc + cx * gy + cy
    order = np.argsort(key, kind="stable")          # (picker, cell, index)
    key, cx, cy, u, pk = key[order], cx[order], cy[order], u[order], pk[order]
    cstart = np.searchsorted(key, np.arange(K * nc + 1), side="left")
    c0 = cx - ((u - cx.astype(f32)) < f32(0.5)).astype(int)
    y0, y1 = np.maximum(cy - 1, 0), np.minimum(cy + 1, gy - 1)
    ln = np.zeros((n, max(K - 1, 1), 2), np.int64)
    for j in range(K - 1):
        q = pk + 1 + j
        for d in (0, 1):
            col = c0 + d
            ok = (q < K) & (col >= 0) & (col < gx)
            cb = np.where(ok, q * nc + col * gy, 0)
            ln[:, j, d] = np.where(ok, cstart[cb + y1 + 1] - cstart[cb + y0], 0)
    return ln, pk, order


def wave_iterations(ln, threads):
    """(ranges, per grid, flattened, perfect) wave iterations of one micrograph."""
    n = len(ln)
    out = np.zeros(4, np.int64)
    tid = np.arange(threads)
    for rnd, r0 in enumerate(range(0, n, threads)):
        ts = r0 + threads - 1 - tid if rnd & 1 else r0 + tid
        act = ts < n
        lw = np.zeros((threads,) + ln.shape[1:], np.int64)
        lw[act] = ln[ts[act]]
        lw = lw.reshape(threads // 64, 64, *ln.shape[1:])        # [wave, lane, grid, column]
        out[0] += lw.max(axis=1).sum()
        out[1] += lw.sum(axis=3).max(axis=1).sum()
        out[2] += lw.sum(axis=(2, 3)).max(axis=1).sum()
        out[3] += (-(-lw.sum(axis=(1, 2, 3)) // 64)).sum()
    return out


def forward_degrees(mg, B, order):
    """Forward degree (JI > 0.3 partners in higher pickers, reference arithmetic) of the box at
    every sorted position; `order` as returned by box_ranges."""
    xs = np.concatenate([t[0] for t in mg]).astype(np.float64)
    ys = np.concatenate([t[1] for t in mg]).astype(np.float64)
    pk = np.concatenate([np.full(len(t[0]), p) for p, t in enumerate(mg)])
    xo = np.maximum((np.minimum(xs[:, None], xs[None, :]) + B) - np.maximum(xs[:, None], xs[None, :]), 0.0)
    yo = np.maximum((np.minimum(ys[:, None], ys[None, :]) + B) - np.maximum(ys[:, None], ys[None, :]), 0.0)
    inter = xo * yo
    with np.errstate(invalid="ignore"):
        edge = (inter / (2 * B * B - inter) > 0.3) & (pk[:, None] < pk[None, :])
    return edge.sum(axis=1)[order]


def degree_report(deg, threads):
    """One micrograph's {boxes, edges, slow_boxes, wave_rounds, slow_wave_rounds, write_trips}
    from the forward degrees in sorted-position order (see the module docstring)."""
    n = len(deg)
    out = dict(boxes=n, edges=int(deg.sum()), slow_boxes=int((deg > 2).sum()), wave_rounds=0,
               slow_wave_rounds=0, write_trips=0)
    tid = np.arange(threads)
    for rnd, r0 in enumerate(range(0, n, threads)):
        ts = r0 + threads - 1 - tid if rnd & 1 else r0 + tid
        act = (ts < n).reshape(threads // 64, 64)
        dw = np.zeros(threads, np.int64)
        dw[ts < n] = deg[ts[ts < n]]
        dw = dw.reshape(threads // 64, 64)                         # [wave, lane]
        out["wave_rounds"] += int(act.any(axis=1).sum())
        out["slow_wave_rounds"] += int((dw > 2).any(axis=1).sum())
        out["write_trips"] += int(dw.max(axis=1).sum())
    return out


def degree_model(config, threads, n_mg, frac=False):
    """degree_report averaged over n_mg synth micrographs (seed 0)."""
    cfg = synth.SynthConfig(**synth.CONFIGS[config], seed=0, frac=frac)
    tot = {}
    for mg in synth.batch(cfg, n_mg):
        order = box_ranges(mg, float(cfg.box))[2]
        for k, v in degree_report(forward_degrees(mg, float(cfg.box), order), threads).items():
            tot[k] = tot.get(k, 0) + v
    return {k: v / n_mg for k, v in tot.items()}


def model(config, threads, n_mg, frac=False):
    cfg = synth.SynthConfig(**synth.CONFIGS[config], seed=0, frac=frac)
    tot = np.zeros(4, np.int64)
    for mg in synth.batch(cfg, n_mg):
        ln = box_ranges(mg, float(cfg.box))[0]
        tot += wave_iterations(ln, threads)
    return tot / n_mg


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="C2", choices=sorted(synth.CONFIGS))
    ap.add_argument("--threads", type=int, default=0, help="workgroup size (multiple of 64)")
    ap.add_argument("--micrographs", type=int, default=0)
    ap.add_argument("--frac", action="store_true", help="3-decimal coordinates (C2_frac)")
    ap.add_argument("--degrees", action="store_true",
                    help="forward degrees per wave-round (the one-pass list write)")
    a = ap.parse_args()
    threads = a.threads or DEFAULT_THREADS[a.config]
    n_mg = a.micrographs or (40 if a.config == "C2" else 20)
    if a.degrees:
        d = degree_model(a.config, threads, n_mg, a.frac)
        print(f"{a.config}{'_frac' if a.frac else ''}: {n_mg} micrographs, {threads} threads, "
              f"per micrograph")
        print(f"  boxes / forward edges        {d['boxes']:8.1f} / {d['edges']:.1f}")
        print(f"  boxes with > 2 edges         {d['slow_boxes']:8.1f}  "
              f"({100 * d['slow_boxes'] / d['boxes']:.1f} %)")
        print(f"  wave-rounds holding a box    {d['wave_rounds']:8.1f}")
        print(f"  ... one with > 2 edges       {d['slow_wave_rounds']:8.1f}  "
              f"({100 * d['slow_wave_rounds'] / d['wave_rounds']:.0f} %)")
        print(f"  write-loop trips             {d['write_trips']:8.1f}")
        sys.exit(0)
    rg, pg, fl, pf = model(a.config, threads, n_mg, a.frac)
    print(f"{a.config}{'_frac' if a.frac else ''}: {n_mg} micrographs, {threads} threads, "
          f"count-loop wave iterations per micrograph")
    print(f"  one loop per range (before)  {rg:8.1f}")
    print(f"  one loop per target grid     {pg:8.1f}  ({100 * (pg / rg - 1):+.0f} %)")
    print(f"  one loop per box (flattened) {fl:8.1f}  ({100 * (fl / rg - 1):+.0f} %)")
    print(f"  lane-perfect                 {pf:8.1f}")
    print(f"  flattening removes {100 * (rg - fl) / (rg - pf):.0f} % of the removable waste")
