"""CPU oracle of the greedy non-maximum suppression contract (include/repic_gc.h, rgc_nms), in
plain Python floats: ``min``, ``max``, ``+``, ``-``, ``*``, ``/`` on Python floats are the f64
operations of the reference's numpy scalars (get_cliques.py:40-46), in the same order.

A segment is a list of boxes in priority order; two boxes conflict iff the quotient exceeds the
threshold, strictly; keep[i] iff no kept j < i conflicts with i.  A box with a non-finite
coordinate conflicts with nothing.
"""
from __future__ import annotations

import bisect
import math

import numpy as np


def jaccard(x1, y1, x2, y2, box):
    """calc_jaccard of the reference on Python floats (box is a float)."""
    xo = max((min(x1, x2) + box) - max(x1, x2), 0.0)
    yo = max((min(y1, y2) + box) - max(y1, y2), 0.0)
    inter = xo * yo
    return inter / ((2.0 * box * box) - inter)


def conflict(x1, y1, x2, y2, box, t):
    if not (math.isfinite(x1) and math.isfinite(y1) and math.isfinite(x2) and math.isfinite(y2)):
        return False
    return jaccard(x1, y1, x2, y2, box) > t


def _windows(x, y, box):
    """Per box the candidates whose x lies within box (and a relative margin far above any
    rounding of the bounds) of its own, from one x-sorted list of the finite boxes."""
    fin = [i for i in range(len(x)) if math.isfinite(x[i]) and math.isfinite(y[i])]
    fin.sort(key=lambda i: x[i])
    xs = [x[i] for i in fin]

    def cand(i):
        if not (math.isfinite(x[i]) and math.isfinite(y[i])):
            return ()
        m = box + (abs(x[i]) + box) * 1e-9
        return fin[bisect.bisect_left(xs, x[i] - m):bisect.bisect_right(xs, x[i] + m)]
    return cand


def nms_oracle(x, y, box_size, t):
    """keep mask (bool array) of one segment in priority order."""
    x = [float(v) for v in x]
    y = [float(v) for v in y]
    box, t = float(box_size), float(t)
    cand = _windows(x, y, box)
    keep = [False] * len(x)
    for i in range(len(x)):
        xi, yi = x[i], y[i]
        ok = True
        for j in cand(i):
            if j < i and keep[j] and jaccard(x[j], y[j], xi, yi, box) > t:
                ok = False
                break
        keep[i] = ok
    return np.array(keep, bool)


def nms_oracle_segments(seg_off, x, y, box_size, t):
    """(keep uint8[n], kept int64[n_seg]) as ``Context.nms`` returns them."""
    keep = np.zeros(len(x), np.uint8)
    kept = np.zeros(len(seg_off) - 1, np.int64)
    for s in range(len(seg_off) - 1):
        a, b = int(seg_off[s]), int(seg_off[s + 1])
        keep[a:b] = nms_oracle(x[a:b], y[a:b], box_size, t)
        kept[s] = int(keep[a:b].sum())
    return keep, kept


def characterised(x, y, keep, box_size, t):
    """The characterisation check: for every i, keep[i] == not any(keep[j] for j < i
    conflicting with i).  -> the first i at which it fails, or None."""
    x = [float(v) for v in x]
    y = [float(v) for v in y]
    box, t = float(box_size), float(t)
    cand = _windows(x, y, box)
    for i in range(len(x)):
        hit = any(j < i and keep[j] and jaccard(x[j], y[j], x[i], y[i], box) > t
                  for j in cand(i))
        if bool(keep[i]) == hit:
            return i
    return None


def oracle_keep_list(segments, box_size, ji_threshold=0.3, ctx=None, device=0):
    """Drop-in for ``repic_amd.nms.nms_keep`` without a device."""
    return [nms_oracle(xs, ys, box_size, ji_threshold) for xs, ys in segments]


def parse_box_lines(raw: bytes):
    """(header or None, data lines with endings) of BOX bytes; the header rule of the parser:
    line 1 is a header iff its first token is not a float."""
    lines = raw.splitlines(keepends=True)
    if not lines:
        return None, []
    tok = lines[0].split()
    try:
        float(tok[0])
    except (ValueError, IndexError):
        return lines[0], lines[1:]
    return None, lines


def box_xys(lines):
    """x, y, score of data lines (5 whitespace-separated columns)."""
    cols = [ln.split() for ln in lines]
    return ([float(c[0]) for c in cols], [float(c[1]) for c in cols],
            [float(c[4]) for c in cols])
