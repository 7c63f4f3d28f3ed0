#!/usr/bin/env python3
"""Golden fixtures for the score_detections threshold sweep, produced by the REAL reference in
THIS container (CPU only).

Test infrastructure only (the reference never travels to the GPU box).  Imports
/root/reference/repic/utils/score_detections.py and calls its ``get_segmentation_scores``
(score_detections.py:16-48) once per threshold of every case, and records

* ``score_sweep/cases.npz``: boxes (x, y, w, h, conf) of every case;
* ``score_sweep/meta.json``: the thresholds (float.hex), the other arguments, and per threshold
  the reference's (prec, rec, f1, pos_frac) as float64 bit patterns and types.

  python tests/golden/make_score_sweep_golden.py
"""
from __future__ import annotations

import json
import os
import shutil
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "score_sweep")
sys.path.insert(0, "/root/reference/repic/utils")

import score_detections as ref  # noqa: E402  (reference module)
from coord_converter import Box  # noqa: E402


def _boxes(rng, n, W, H, size, frac=False, spread=0):
    x = rng.uniform(-spread, W - size + spread, n)
    y = rng.uniform(-spread, H - size + spread, n)
    if frac:
        x = np.round(x * 2) / 2          # exact .5 values: Python round() goes to even
        y = np.round(y * 2) / 2
    else:
        x, y = np.rint(x), np.rint(y)
    w = np.full(n, float(size))
    h = np.full(n, float(size))
    c = rng.uniform(0, 1, n)
    return np.stack([x, y, w, h, c], axis=1)


def cases():
    rng = np.random.default_rng(23)
    inf = float("inf")
    out = []
    out.append(("sweep512", _boxes(rng, 30, 512, 512, 40), _boxes(rng, 40, 512, 512, 40),
                [0.0, 0.25, 0.5, 0.75, 1.0, 2.0], {"mrc_w": 512, "mrc_h": 512}))
    p = _boxes(rng, 60, 512, 512, 40)
    p[:, 4] = np.round(p[:, 4] * 10) / 10      # confidences on the thresholds themselves
    out.append(("tenths", _boxes(rng, 30, 512, 512, 40), p, (np.arange(11) / 10).tolist(),
                {"mrc_w": 512, "mrc_h": 512}))
    out.append(("half_neg_inferred", _boxes(rng, 40, 600, 500, 64, True, 80),
                _boxes(rng, 50, 600, 500, 64, True, 80), [0.9, 0.1, 0.5, 0.5, 0.3], {}))
    p = _boxes(rng, 40, 512, 512, 40)
    p[3, 4] = np.nan                           # kept at every threshold, +inf included
    p[7, 4] = np.nan
    out.append(("nan_conf", _boxes(rng, 30, 512, 512, 40), p,
                [0.5, -inf, 0.5, inf, 0.1, 2.0], {"mrc_w": 512, "mrc_h": 512}))
    out.append(("no_picks", _boxes(rng, 20, 400, 400, 30), np.zeros((0, 5)), [0.0, 0.5, 1.0], {}))
    out.append(("mg4096", _boxes(rng, 300, 4096, 4096, 180), _boxes(rng, 330, 4096, 4096, 180),
                np.linspace(0.0, 1.0, 32).tolist(), {"mrc_w": 4096, "mrc_h": 4096}))
    return out


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    meta, arrays = {"cases": []}, {}
    for name, g, p, ts, kw in cases():
        gb = [Box(*r) for r in g.tolist()]
        pb = [Box(*r) for r in p.tolist()]
        res = []
        for t in ts:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res.append(ref.get_segmentation_scores(gb, pb, conf_thresh=t, **kw))
        arrays[name + "_gt"] = g
        arrays[name + "_pk"] = p
        meta["cases"].append({"name": name, "kwargs": kw,
                              "thresh_hex": [float(t).hex() for t in ts],
                              "result_hex": [[float(v).hex() for v in r] for r in res],
                              "result_type": [[type(v).__name__ for v in r] for r in res]})
    np.savez_compressed(os.path.join(OUT, "cases.npz"), **arrays)
    with open(os.path.join(OUT, "meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print(f"wrote {len(meta['cases'])} cases to {OUT}")


if __name__ == "__main__":
    main()
