"""Greedy non-maximum suppression of picks on the device (``rgc_nms``).

A *segment* is a list of boxes in priority order (index 0 first), all squares of side
``box_size`` with lower-left corner ``(x, y)``.  Two boxes conflict iff the reference's Jaccard
quotient (get_cliques.py:40-46, f64, one division) exceeds the threshold, strictly.  A box is kept
iff no kept box before it in its segment conflicts with it; a box with a non-finite coordinate
conflicts with nothing.  The kept set is unique, so the mask is a function of the input alone.
"""
from __future__ import annotations

import numpy as np

from . import _lib

# boxes per device call (nms_keep splits a longer list of segments between calls)
CALL_BOXES = 1 << 25


def nms_order(score):
    """The priority permutation of a file's scores: descending, NaN after every number, ties
    (-0.0 == 0.0 included) by original index."""
    return np.argsort(-np.asarray(score, np.float64), kind="stable")


def nms_keep(segments, box_size, ji_threshold=0.3, ctx=None, device=0):
    """``segments``: a list of ``(x, y)`` pairs already in priority order -> a list of bool
    arrays, True where the box is kept.  One device call per at most ``CALL_BOXES`` boxes (a
    larger segment gets a call of its own).  ``ctx``: a :class:`_lib.Context` to run on (else
    one on ``device`` for the duration of the call)."""
    t = _lib.check_ji_threshold(ji_threshold)
    segs = [(np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64))
            for x, y in segments]
    for x, y in segs:
        if x.ndim != 1 or x.shape != y.shape:
            raise ValueError("nms_keep: x and y of a segment must be 1-D arrays of one length")
    own = ctx is None
    if own:
        ctx = _lib.Context(int(device or 0))
    out = []
    try:
        i = 0
        while i < len(segs):
            j, n = i + 1, len(segs[i][0])
            while j < len(segs) and n + len(segs[j][0]) <= CALL_BOXES:
                n += len(segs[j][0])
                j += 1
            off = np.zeros(j - i + 1, np.int64)
            np.cumsum([len(x) for x, _ in segs[i:j]], out=off[1:])
            keep, _ = ctx.nms(off, np.concatenate([x for x, _ in segs[i:j]]),
                              np.concatenate([y for _, y in segs[i:j]]), box_size, t)
            keep = keep.astype(bool)
            out.extend(keep[off[s]:off[s + 1]] for s in range(j - i))
            i = j
    finally:
        if own:
            ctx.close()
    return out


def nms_boxes(x, y, score, box_size, ji_threshold=0.3, ctx=None):
    """The keep mask of one file's boxes, in file order: priority is ``nms_order(score)``."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    order = nms_order(score)
    if not (x.shape == y.shape == order.shape):
        raise ValueError("nms_boxes: x, y and score must be 1-D arrays of one length")
    keep = nms_keep([(x[order], y[order])], box_size, ji_threshold, ctx)[0]
    mask = np.zeros(len(x), bool)
    mask[order] = keep
    return mask
