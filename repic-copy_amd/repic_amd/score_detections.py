"""``score_detections`` — precision / recall / F1 of picked particle sets, MI355X raster.

Same interface as the reference module (repic/utils/score_detections.py):
``get_segmentation_scores(gt_boxes, pckr_boxes, conf_thresh=None, mrc_w=None, mrc_h=None)``
returns ``(prec, rec, f1, pos_frac)`` with the reference's numpy scalar types, and the command
line (``-g``, ``-p``, ``-c``, ``--height``, ``--width``, ``--verbose``, ``--out_dir``) writes the
same ``particle_set_comp.tsv``.  The (H x W) int16 masks the reference paints
(score_detections.py:28-41) are never materialised: ``librepic_gc.so``'s ``rgc_score_pairs``
paints 1-bit tiles in LDS and returns three pixel counts per pair (rgc_score.hip), many
micrograph pairs per launch (``score_pairs``).  No CPU fallback: the library must load.

Beyond the reference: ``score_sweep`` / ``sweep_counts`` give what ``score_pairs`` gives at each
of a list of confidence thresholds from one launch that paints every box once
(``rgc_score_sweep``), and ``--sweep T [T ...]`` writes those curves per file
(``particle_set_sweep.tsv``) and pooled over all files (``particle_set_sweep_pooled.tsv``).
``match_pairs`` / ``match_scores`` give the particle-level metric the picking papers report: the
picks that hit a ground-truth particle one to one at an IoU cutoff, as the size of a
maximum-cardinality matching found on the device for every pair of a data set in one call
(``rgc_score_match``, rgc_match.hip); ``--match_ji T`` writes it per file
(``particle_set_match.tsv``) and pooled (``particle_set_match_pooled.tsv``).
``match_sweep`` / ``match_curve`` give that metric at every confidence threshold of a list, the
precision / recall curve, from one device call that builds the edges once and augments the
matching from threshold to threshold (``rgc_score_match_sweep``); ``average_precision`` is the
area under it, and ``--match_sweep T [T ...]`` writes both (``particle_set_match_sweep.tsv``,
``particle_set_match_sweep_pooled.tsv``).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

from . import _lib

# the reference's coordinate record (coord_converter.py:50-51: conf defaults to 0)
Box = namedtuple("Box", ["x", "y", "w", "h", "conf"])
Box.__new__.__defaults__ = (0,)


class ScoreIn(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("height", C.c_void_p), ("width", C.c_void_p),
                ("gt_off", C.c_void_p), ("pk_off", C.c_void_p), ("boxes", C.c_void_p),
                ("flags", C.c_uint32)]


_lib.lib.rgc_score_pairs.argtypes = [C.c_void_p, C.POINTER(ScoreIn), C.c_void_p]
_lib.lib.rgc_score_pairs.restype = C.c_int


class ScoreSweepIn(C.Structure):
    _fields_ = [("pairs", ScoreIn), ("n_thr", C.c_int32), ("keep", C.c_void_p)]


_lib.lib.rgc_score_sweep.argtypes = [C.c_void_p, C.POINTER(ScoreSweepIn), C.c_void_p]
_lib.lib.rgc_score_sweep.restype = C.c_int


class ScoreMatchIn(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("gt_off", C.c_void_p), ("pk_off", C.c_void_p),
                ("boxes", C.c_void_p), ("ji_threshold", C.c_double), ("flags", C.c_uint32)]


_lib.lib.rgc_score_match.argtypes = [C.c_void_p, C.POINTER(ScoreMatchIn), C.c_void_p, C.c_void_p]
_lib.lib.rgc_score_match.restype = C.c_int


class ScoreMatchSweepIn(C.Structure):
    _fields_ = [("pairs", ScoreMatchIn), ("n_thr", C.c_int32), ("keep", C.c_void_p)]


_lib.lib.rgc_score_match_sweep.argtypes = [C.c_void_p, C.POINTER(ScoreMatchSweepIn), C.c_void_p]
_lib.lib.rgc_score_match_sweep.restype = C.c_int
_lib.lib.rgc_test_iou_edge.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_double]
_lib.lib.rgc_test_iou_edge.restype = C.c_int


def _py_round(v):
    """Python ``round(v)`` of each value (score_detections.py:31,36): half to even -> int."""
    v = np.asarray(v)
    if v.dtype.kind in "iu":
        return v.astype(np.int64)
    v = v.astype(np.float64)
    if not np.isfinite(v).all():
        raise ValueError("cannot convert float NaN or infinity to integer")
    return np.rint(v).astype(np.int64)


def _slice_bounds(a, n):
    """Python slice.indices for step 1: negative values wrap once, then clamp to [0, n]."""
    return np.where(a < 0, np.maximum(a + n, 0), np.minimum(a, n))


def _as_cols(boxes):
    """(x, y, w, h, conf) columns of a box list (namedtuples / tuples) or a (n, >=4) array."""
    if isinstance(boxes, np.ndarray):
        a = boxes
        conf = a[:, 4] if a.shape[1] > 4 else np.zeros(len(a))
        return a[:, 0], a[:, 1], a[:, 2], a[:, 3], conf
    if not len(boxes):
        z = np.zeros(0)
        return z, z, z, z, z
    cols = list(zip(*[tuple(b) for b in boxes]))
    conf = cols[4] if len(cols) > 4 else [0] * len(boxes)
    return tuple(np.asarray(c) for c in cols[:4]) + (np.asarray(conf, dtype=np.float64),)


def _mask_slices(x, y, w, h, H, W, kept=False):
    """Non-empty numpy slices [r0, r1) x [c0, c1) of ``arr[y:y+h, x:x+w] = 1``; with ``kept``
    also the mask of the boxes that have one."""
    xi, yi, wi, hi = (_py_round(v) for v in (x, y, w, h))
    r0, r1 = _slice_bounds(yi, H), _slice_bounds(yi + hi, H)
    c0, c1 = _slice_bounds(xi, W), _slice_bounds(xi + wi, W)
    keep = (r0 < r1) & (c0 < c1)
    s = np.stack([r0[keep], r1[keep], c0[keep], c1[keep]], axis=1).astype(np.int32)
    return (s, keep) if kept else s


def _scores(counts, H, W):
    """score_detections.py:43-48 on the three pixel counts, same numpy scalar arithmetic."""
    gsum, num_pos, tp = (np.int64(v) for v in counts)
    pos_frac = num_pos / (H * W)
    prec = 0.0 if (tp == num_pos == 0.0) else (tp / num_pos)
    rec = tp / gsum
    f1 = 0.0 if (prec == rec == 0.0) else ((2 * prec * rec) / (prec + rec))
    return prec, rec, f1, pos_frac


_CTX = None


def _ctx():
    global _CTX
    if _CTX is None:
        _CTX = _lib.Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _CTX


def score_pairs(pairs, conf_thresh=None, mrc_w=None, mrc_h=None, ctx=None, timing=False):
    """Batched ``get_segmentation_scores`` over (gt_boxes, pckr_boxes) pairs: one device call.
    Returns a list of (prec, rec, f1, pos_frac); with ``timing`` also the kernel ms."""
    ctx = ctx or _ctx()
    Hs, Ws, gts, pks = [], [], [], []
    for gt, pk in pairs:
        g = _as_cols(gt)
        p = _as_cols(pk)
        H, W = _pair_dims(g, p, mrc_w, mrc_h)
        if conf_thresh is not None:
            keep = ~(p[4] < conf_thresh)          # b.conf < conf_thresh -> skipped (:35-36)
            p = tuple(c[keep] for c in p)
        gts.append(_mask_slices(*g[:4], H, W))
        pks.append(_mask_slices(*p[:4], H, W))
        Hs.append(H)
        Ws.append(W)
    npairs = len(Hs)
    si, H, W, hold = _score_in(gts, pks, Hs, Ws, timing)
    counts = np.zeros((npairs, 3), dtype=np.int64)
    ctx._retire()   # a live Result of an earlier run keeps its host buffers
    _lib._check(_lib.lib.rgc_score_pairs(ctx._p, C.byref(si), counts.ctypes.data))
    del hold
    out = [_scores(counts[i], int(H[i]), int(W[i])) for i in range(npairs)]
    if timing:
        return out, dict(ctx.kernel_times())
    return out


def _pair_dims(g, p, mrc_w, mrc_h):
    """(H, W) of a pair's masks from its (x, y, w, h, conf) columns."""
    # mrc_w / mrc_h default: round(max(x + w)) over every box, thresholded or not (:22-26)
    W = mrc_w if mrc_w is not None else int(_py_round(np.max(np.concatenate(
        [g[0] + g[2], p[0] + p[2]]))))
    H = mrc_h if mrc_h is not None else int(_py_round(np.max(np.concatenate(
        [g[1] + g[3], p[1] + p[3]]))))
    if H < 0 or W < 0:
        raise ValueError("negative dimensions are not allowed")
    return H, W


def _score_in(gts, pks, Hs, Ws, timing):
    """rgc_score_in of per-pair slice arrays: every pair's ground-truth boxes, then every
    pair's picks -> (ScoreIn, H, W, the arrays it points into)."""
    z = np.zeros((0, 4), np.int32)
    boxes = np.ascontiguousarray(np.concatenate(gts + pks + [z]), dtype=np.int32)
    ng = np.cumsum([0] + [len(v) for v in gts]).astype(np.int64)
    gt_arr = ng
    pk_arr = (ng[-1] + np.cumsum([0] + [len(v) for v in pks])).astype(np.int64)
    H = np.asarray(Hs, dtype=np.int64)
    W = np.asarray(Ws, dtype=np.int64)
    si = ScoreIn(len(Hs), H.ctypes.data, W.ctypes.data, gt_arr.ctypes.data, pk_arr.ctypes.data,
                 boxes.ctypes.data, _lib.F_TIMING if timing else 0)
    return si, H, W, (boxes, gt_arr, pk_arr)


# ------------------------------------------------------------------------- threshold sweep
def _check_threshs(conf_threshs):
    """The thresholds of a sweep as a float64 array: any non-NaN floats, at least one."""
    ts = np.asarray(list(conf_threshs), dtype=np.float64).reshape(-1)
    if ts.size == 0:
        raise ValueError("conf_threshs is empty: a sweep needs at least one threshold")
    if np.isnan(ts).any():
        raise ValueError("conf_threshs holds NaN: every pick would be kept at it, as at -inf")
    return ts


def _sweep_plan(conf, uniq):
    """Order of a pair's picks for the sweep over the ascending unique thresholds ``uniq``.
    A pick is kept at t iff not (conf < t) (score_detections.py:34-36), so its level, the number
    of thresholds that keep it, is the count of t <= conf (all of them for a NaN confidence)
    and it is kept at ``uniq[j]`` iff level > j.  -> (order, keep): ``order`` sorts the picks by
    level descending (stable), ``keep[j]`` picks of that order are kept at ``uniq[j]``."""
    conf = np.asarray(conf, dtype=np.float64)
    level = np.searchsorted(uniq, conf, side="right")
    level[np.isnan(conf)] = len(uniq)
    order = np.argsort(-level, kind="stable")
    below = np.cumsum(np.bincount(level, minlength=len(uniq) + 1))[:len(uniq)]   # level <= j
    keep = (len(level) - below).astype(np.int64)
    return order, keep


def _sweep(pairs, conf_threshs, mrc_w=None, mrc_h=None, ctx=None, timing=False):
    """-> (counts (n_pairs, T, 3) in the caller's threshold order, H, W, kernel times)."""
    ts = _check_threshs(conf_threshs)
    uniq, inv = np.unique(ts, return_inverse=True)
    ctx = ctx or _ctx()
    Hs, Ws, gts, pks, keeps = [], [], [], [], []
    for gt, pk in pairs:
        g = _as_cols(gt)
        p = _as_cols(pk)
        H, W = _pair_dims(g, p, mrc_w, mrc_h)
        s, has = _mask_slices(*p[:4], H, W, kept=True)
        order, keep = _sweep_plan(np.asarray(p[4], dtype=np.float64)[has], uniq)
        gts.append(_mask_slices(*g[:4], H, W))
        pks.append(s[order])
        keeps.append(keep)
        Hs.append(H)
        Ws.append(W)
    npairs, T = len(Hs), len(uniq)
    si, H, W, hold = _score_in(gts, pks, Hs, Ws, timing)
    keep = np.ascontiguousarray(np.concatenate(keeps + [np.zeros(0, np.int64)]), dtype=np.int64)
    counts = np.zeros((npairs, T, 3), dtype=np.int64)
    sw = ScoreSweepIn(si, T, keep.ctypes.data)
    ctx._retire()   # a live Result of an earlier run keeps its host buffers
    _lib._check(_lib.lib.rgc_score_sweep(ctx._p, C.byref(sw), counts.ctypes.data))
    del hold
    return counts[:, inv.reshape(-1), :], H, W, (dict(ctx.kernel_times()) if timing else None)


def sweep_counts(pairs, conf_threshs, mrc_w=None, mrc_h=None, ctx=None, timing=False):
    """The three pixel counts (sum(gt), sum(pckr), sum(gt * pckr)) of every pair at every
    threshold of ``conf_threshs`` from one device call that paints each box once
    (``rgc_score_sweep``): an (n_pairs, T, 3) int64 array in the order the thresholds were
    given (any order, duplicates and +-inf allowed; NaN or an empty list: ValueError).  With
    ``timing`` also the kernel ms."""
    counts, _, _, ms = _sweep(pairs, conf_threshs, mrc_w, mrc_h, ctx, timing)
    return (counts, ms) if timing else counts


def score_sweep(pairs, conf_threshs, mrc_w=None, mrc_h=None, ctx=None, timing=False):
    """``score_pairs`` at every threshold of ``conf_threshs`` in one device call:
    ``score_sweep(pairs, ts)[i][j] == score_pairs(pairs, conf_thresh=ts[j])[i]``."""
    counts, H, W, ms = _sweep(pairs, conf_threshs, mrc_w, mrc_h, ctx, timing)
    out = [[_scores(c, int(H[i]), int(W[i])) for c in counts[i]] for i in range(len(H))]
    return (out, ms) if timing else out


def _sweep_rows(names, conf_threshs, counts, H, W):
    """Rows of particle_set_sweep.tsv: grouped by file, thresholds in the order given."""
    return [(m, repr(float(t))) + _scores(counts[i][j], int(H[i]), int(W[i]))
            for i, m in enumerate(names) for j, t in enumerate(conf_threshs)]


def _pooled_rows(conf_threshs, counts, H, W):
    """Rows of particle_set_sweep_pooled.tsv: per threshold, ``_scores`` of the pixel counts
    summed over all pairs (np.int64) on the summed mask area, then the three sums."""
    area = sum(int(h) * int(w) for h, w in zip(H, W))
    tot = np.asarray(counts, dtype=np.int64).reshape(-1, len(conf_threshs), 3).sum(
        axis=0, dtype=np.int64)
    return [(repr(float(t)),) + _scores(tot[j], area, 1) + tuple(tot[j])
            for j, t in enumerate(conf_threshs)]


def _write_tsv(path, header, rows):
    with open(path, "wt") as o:
        o.write("\t".join(header) + "\n")
        for e in rows:
            o.write("\t".join(str(v) for v in e) + "\n")


def write_sweep_tsv(path, names, conf_threshs, counts, H, W):
    _write_tsv(path, ["filename", "conf_thresh", "precision", "recall", "f1", "pos_frac"],
               _sweep_rows(names, conf_threshs, counts, H, W))


def write_sweep_pooled_tsv(path, conf_threshs, counts, H, W):
    _write_tsv(path, ["conf_thresh", "precision", "recall", "f1", "pos_frac", "gt_pixels",
                      "picked_pixels", "tp_pixels"], _pooled_rows(conf_threshs, counts, H, W))


# ------------------------------------------------------------------ particle-level matching
MATCH_XY_MAX = 1 << 30     # |round(x)|, |round(y)|
MATCH_SIDE_MAX = 1 << 25   # round(w), round(h): every area and every sum exact in int64 and f64


def iou_edge(a, b, t):
    """Host twin of the device edge test (``rgc_test_iou_edge``) on two integer rectangles
    (x0, x1, y0, y1): True iff both have a pixel and ``float(I) / float(U) > t``."""
    qa = (C.c_int32 * 4)(*[int(v) for v in a])
    qb = (C.c_int32 * 4)(*[int(v) for v in b])
    return bool(_lib.lib.rgc_test_iou_edge(qa, qb, float(t)))


def _match_rects(x, y, w, h):
    """(n, 4) int32 x0, x1, y0, y1 of the rectangles [x, x + w) x [y, y + h) after Python
    ``round()`` of each value, unclipped.  A box with round(w) < 1 or round(h) < 1 becomes the
    empty rectangle at its corner (counted, never matched).  ValueError: non-finite values
    (``_py_round``'s), |x|, |y| above 2^30, w, h above 2^25."""
    xi, yi, wi, hi = (_py_round(np.clip(_finite(v), -2.0 ** 62, 2.0 ** 62)) for v in (x, y, w, h))
    if len(xi) and (np.abs(xi).max() > MATCH_XY_MAX or np.abs(yi).max() > MATCH_XY_MAX):
        raise ValueError("box coordinates beyond +-2^30 after rounding")
    if len(xi) and (wi.max() > MATCH_SIDE_MAX or hi.max() > MATCH_SIDE_MAX):
        raise ValueError("box sizes beyond 2^25 after rounding")
    none = (wi < 1) | (hi < 1)
    wi, hi = np.where(none, 0, wi), np.where(none, 0, hi)
    return np.stack([xi, xi + wi, yi, yi + hi], axis=1).astype(np.int32)


def _finite(v):
    """``v`` as float64, with ``_py_round``'s ValueError for NaN or infinity."""
    v = np.asarray(v, dtype=np.float64)
    if not np.isfinite(v).all():
        raise ValueError("cannot convert float NaN or infinity to integer")
    return v


def _prf(n_gt, n_picked, tp):
    """(precision, recall, f1) of the counts as Python floats; 0.0 at a zero denominator."""
    n_gt, n_picked, tp = int(n_gt), int(n_picked), int(tp)
    prec = tp / n_picked if n_picked else 0.0
    rec = tp / n_gt if n_gt else 0.0
    f1 = 2 * prec * rec / (prec + rec) if prec + rec else 0.0
    return prec, rec, f1


def match_pairs(pairs, ji_thresh, conf_thresh=None, ctx=None, timing=False, assignment=False):
    """Particle-level true positives of every (gt_boxes, pckr_boxes) pair in one device call:
    an (n_pairs, 3) int64 array of n_gt, n_picked (picks with ``conf < conf_thresh`` dropped,
    as in ``score_pairs``) and tp, the size of a maximum-cardinality one-to-one matching in
    which a ground-truth box and a pick can be joined iff the IoU of their rounded, unclipped
    rectangles exceeds ``ji_thresh`` (finite, 0 <= t < 1).  With ``assignment`` also a list of
    int32 arrays, one per pair over its kept picks in the caller's order: the index of the
    pick's ground-truth box within the pair, or -1 (the same arrays on every run); with
    ``timing`` also the kernel ms, last.  Bad values raise ValueError before any device work."""
    t = _lib.check_ji_threshold(ji_thresh)
    gts, pks = [], []
    for gt, pk in pairs:
        g = _as_cols(gt)
        p = _as_cols(pk)
        if conf_thresh is not None:
            keep = ~(np.asarray(p[4], dtype=np.float64) < conf_thresh)
            p = tuple(np.asarray(c)[keep] for c in p)
        gts.append(_match_rects(*g[:4]))
        pks.append(_match_rects(*p[:4]))
    npairs = len(gts)
    z = np.zeros((0, 4), np.int32)
    boxes = np.ascontiguousarray(np.concatenate(gts + pks + [z]), dtype=np.int32)
    gt_off = np.cumsum([0] + [len(v) for v in gts]).astype(np.int64)
    pk_off = (gt_off[-1] + np.cumsum([0] + [len(v) for v in pks])).astype(np.int64)
    counts = np.zeros((npairs, 3), dtype=np.int64)
    match = np.full(int(pk_off[-1] - pk_off[0]), -1, dtype=np.int32)
    mi = ScoreMatchIn(npairs, gt_off.ctypes.data, pk_off.ctypes.data, boxes.ctypes.data, t,
                      _lib.F_TIMING if timing else 0)
    ctx = ctx or _ctx()
    ctx._retire()   # a live Result of an earlier run keeps its host buffers
    _lib._check(_lib.lib.rgc_score_match(ctx._p, C.byref(mi), counts.ctypes.data,
                                         match.ctypes.data if assignment else None))
    out = (counts,)
    if assignment:
        lo = pk_off - pk_off[0]
        out += ([match[lo[i]:lo[i + 1]].copy() for i in range(npairs)],)
    if timing:
        out += (dict(ctx.kernel_times()),)
    return out if len(out) > 1 else counts


def match_scores(pairs, ji_thresh, conf_thresh=None, ctx=None):
    """``match_pairs`` as scores: per pair (precision, recall, f1, tp, n_gt, n_picked) with
    precision = tp / n_picked, recall = tp / n_gt, f1 = 2 p r / (p + r), each 0.0 where its
    denominator is zero."""
    counts = match_pairs(pairs, ji_thresh, conf_thresh, ctx)
    return [_prf(g, k, tp) + (int(tp), int(g), int(k)) for g, k, tp in counts.tolist()]


_MATCH_COLS = ["ji_thresh", "n_gt", "n_picked", "tp", "precision", "recall", "f1"]


def _match_row(ji_thresh, c):
    g, k, tp = (int(v) for v in c)
    return (repr(float(ji_thresh)), g, k, tp) + _prf(g, k, tp)


def write_match_tsv(path, names, ji_thresh, counts):
    _write_tsv(path, ["filename"] + _MATCH_COLS,
               [(m,) + _match_row(ji_thresh, counts[i]) for i, m in enumerate(names)])


def write_match_pooled_tsv(path, ji_thresh, counts):
    """One row from the counts summed over all pairs."""
    tot = np.asarray(counts, dtype=np.int64).reshape(-1, 3).sum(axis=0, dtype=np.int64)
    _write_tsv(path, _MATCH_COLS, [_match_row(ji_thresh, tot)])


# ------------------------------------------- particle-level matching at every threshold
def match_sweep(pairs, ji_thresh, conf_threshs, ctx=None, timing=False):
    """``match_pairs`` at every confidence threshold of ``conf_threshs`` in one device call
    (``rgc_score_match_sweep``): an (n_pairs, T, 3) int64 array of n_gt, n_picked, tp with
    ``match_sweep(pairs, t, ts)[i, j] == match_pairs(pairs, t, conf_thresh=ts[j])[i]``, in the
    order the thresholds were given (any order, duplicates and +-inf allowed; NaN or an empty
    list: ValueError).  The pairs are laid out, their edges counted and listed once; the kernel
    goes from the strictest threshold to the loosest and augments the matching of the step before
    from the picks that are new.  A pick with a NaN confidence is kept at every threshold.  Every
    pick's coordinates are checked, whether a threshold keeps it or not.  No assignment is
    returned.  With ``timing`` also the kernel ms.  Bad values raise ValueError before any
    device work."""
    t = _lib.check_ji_threshold(ji_thresh)
    ts = _check_threshs(conf_threshs)
    uniq, inv = np.unique(ts, return_inverse=True)
    gts, pks, keeps = [], [], []
    for gt, pk in pairs:
        g = _as_cols(gt)
        p = _as_cols(pk)
        order, keep = _sweep_plan(np.asarray(p[4], dtype=np.float64), uniq)
        gts.append(_match_rects(*g[:4]))
        pks.append(_match_rects(*p[:4])[order])
        keeps.append(keep)
    npairs, T = len(gts), len(uniq)
    z = np.zeros((0, 4), np.int32)
    boxes = np.ascontiguousarray(np.concatenate(gts + pks + [z]), dtype=np.int32)
    gt_off = np.cumsum([0] + [len(v) for v in gts]).astype(np.int64)
    pk_off = (gt_off[-1] + np.cumsum([0] + [len(v) for v in pks])).astype(np.int64)
    keep = np.ascontiguousarray(np.concatenate(keeps + [np.zeros(0, np.int64)]), dtype=np.int64)
    counts = np.zeros((npairs, T, 3), dtype=np.int64)
    mi = ScoreMatchIn(npairs, gt_off.ctypes.data, pk_off.ctypes.data, boxes.ctypes.data, t,
                      _lib.F_TIMING if timing else 0)
    sw = ScoreMatchSweepIn(mi, T, keep.ctypes.data)
    ctx = ctx or _ctx()
    ctx._retire()   # a live Result of an earlier run keeps its host buffers
    _lib._check(_lib.lib.rgc_score_match_sweep(ctx._p, C.byref(sw), counts.ctypes.data))
    counts = counts[:, inv.reshape(-1), :]
    return (counts, dict(ctx.kernel_times())) if timing else counts


def match_curve(pairs, ji_thresh, conf_threshs, ctx=None):
    """``match_sweep`` as scores: per pair, per threshold in the order given,
    (precision, recall, f1, tp, n_gt, n_picked) as in ``match_scores``."""
    counts = match_sweep(pairs, ji_thresh, conf_threshs, ctx)
    return [[_prf(g, k, tp) + (int(tp), int(g), int(k)) for g, k, tp in c] for c in counts.tolist()]


def average_precision(counts):
    """Average precision of one precision / recall curve: ``counts`` is a (T, 3) array of
    n_gt, n_picked, tp per threshold, one pair's (``match_sweep(...)[i]``) or the sums over the
    pairs.  The distinct rows are taken in order of decreasing threshold, that is of increasing
    n_picked, so that recall R is non-decreasing, and with P, R from ``_prf`` (0.0 at a zero
    denominator) and R_-1 = 0

        AP = sum_i (R_i - R_(i-1)) * P_i

    the uninterpolated form: no precision envelope, no fixed recall grid.  A Python float."""
    rows = sorted({(int(k), int(tp), int(g))
                   for g, k, tp in np.asarray(counts).reshape(-1, 3).tolist()})
    ap, last = 0.0, 0.0
    for k, tp, g in rows:
        prec, rec, _ = _prf(g, k, tp)
        ap += (rec - last) * prec
        last = rec
    return float(ap)


_MATCH_SWEEP_COLS = ["ji_thresh", "conf_thresh", "n_gt", "n_picked", "tp", "precision", "recall",
                     "f1"]


def _match_sweep_rows(ji_thresh, conf_threshs, counts):
    """One pair's (or the pooled) rows, thresholds in the order given."""
    rows = []
    for t, c in zip(conf_threshs, counts):
        g, k, tp = (int(v) for v in c)
        rows.append((repr(float(ji_thresh)), repr(float(t)), g, k, tp) + _prf(g, k, tp))
    return rows


def write_match_sweep_tsv(path, names, ji_thresh, conf_threshs, counts):
    """Rows grouped by file, thresholds in the order given."""
    _write_tsv(path, ["filename"] + _MATCH_SWEEP_COLS,
               [(m,) + r for i, m in enumerate(names)
                for r in _match_sweep_rows(ji_thresh, conf_threshs, counts[i])])


def write_match_sweep_pooled_tsv(path, ji_thresh, conf_threshs, counts):
    """Per threshold one row from the counts summed over all pairs, then a comment line with
    the mean of the pairs' average precisions and the average precision of the pooled curve."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, len(conf_threshs), 3)
    tot = counts.sum(axis=0, dtype=np.int64)
    _write_tsv(path, _MATCH_SWEEP_COLS, _match_sweep_rows(ji_thresh, conf_threshs, tot))
    aps = [average_precision(c) for c in counts]
    mean = sum(aps) / len(aps) if aps else 0.0
    with open(path, "at") as o:
        o.write(f"# average_precision\t{mean}\t{average_precision(tot)}\n")


def get_segmentation_scores(gt_boxes, pckr_boxes, conf_thresh=None, mrc_w=None, mrc_h=None):
    """score_detections.py:16-48 for one pair (prec, rec, f1, pos_frac)."""
    return score_pairs([(gt_boxes, pckr_boxes)], conf_thresh, mrc_w, mrc_h)[0]


# ----------------------------------------------------------------------------- command line
def read_box_file(path):
    """BOX file -> (n, 5) float array x, y, w, h, conf, as the reference reads it with
    coord_converter.process_conversion([path], "box", "box") (tsv_to_df, coord_converter.py:
    200-243): leading lines are skipped up to the first one that does not start with "_" and
    contains a digit; whitespace-separated columns; rows without any numeric value dropped;
    a missing conf column becomes 1 (score_detections.py:118-120)."""
    import pandas as pd
    start = 0
    with open(path) as f:
        for i, line in enumerate(f):
            if not line.startswith("_") and re.search("[0-9]", line):
                start = i
                break
    try:
        df = pd.read_csv(path, sep=r"\s+", header=None, skip_blank_lines=True, skiprows=start)
    except pd.errors.EmptyDataError:
        return np.zeros((0, 5))

    def numeric(v):
        try:
            float(v)
            return True
        except (TypeError, ValueError):
            return False
    df = df[[any(numeric(v) for v in row.dropna()) for _, row in df.iterrows()]]
    cols = [df[c].to_numpy(dtype=np.float64) for c in df.columns[:5]]
    if len(cols) < 5:
        cols.append(np.ones(len(df)))
    return np.stack(cols[:5], axis=1) if len(df) else np.zeros((0, 5))


def _parser():
    ap = argparse.ArgumentParser(
        description="Score detections between ground truth and particle picker coordinate "
                    "sets, matching files by name (BOX format).")
    ap.add_argument("-g", help="Ground truth particle coordinate file(s)", nargs="+", required=True)
    ap.add_argument("-p", help="Particle picker coordinate file(s)", nargs="+", required=True)
    ap.add_argument("-c", help="Confidence threshold", type=float)
    ap.add_argument("--height", help="Micrograph height (pixels)", type=int, default=None)
    ap.add_argument("--width", help="Micrograph width (pixels)", type=int, default=None)
    ap.add_argument("--verbose", help="Print individual boxfile pair scores", action="store_true")
    ap.add_argument("--out_dir", help="file path to output directory", type=str)
    ap.add_argument("--sweep", help="Confidence thresholds to also score at, all from one pass "
                    "(writes particle_set_sweep.tsv and particle_set_sweep_pooled.tsv)",
                    type=float, nargs="+", metavar="T")
    ap.add_argument("--match_ji", help="Also score particle by particle: picks matched one to "
                    "one to ground-truth boxes whose IoU exceeds T (0 <= T < 1), at the -c "
                    "confidence threshold (at a list of thresholds: --match_sweep; the --sweep "
                    "thresholds are the pixel metric's); --height / --width do not apply "
                    "(writes particle_set_match.tsv and particle_set_match_pooled.tsv)",
                    type=float, metavar="T")
    ap.add_argument("--match_sweep", help="Confidence thresholds to also match at, all from one "
                    "device call: the particle-level precision / recall curve and its average "
                    "precision; needs --match_ji (writes particle_set_match_sweep.tsv and "
                    "particle_set_match_sweep_pooled.tsv)", type=float, nargs="+", metavar="T")
    return ap


def main(argv=None):
    ap = _parser()
    a = ap.parse_args(argv)
    if a.match_sweep is not None and a.match_ji is None:
        ap.error("--match_sweep needs --match_ji (the IoU cutoff of the matching)")
    if a.sweep is not None:
        _check_threshs(a.sweep)
    if a.match_ji is not None:
        _lib.check_ji_threshold(a.match_ji)
    if a.match_sweep is not None:
        _check_threshs(a.match_sweep)
    # score_detections.py:87-90, including its quirk: an existing --out_dir is ignored
    if a.out_dir is not None and not os.path.exists(a.out_dir):
        os.makedirs(a.out_dir)
    else:
        a.out_dir = os.path.dirname(a.p[0])
    gt_names = [Path(f).stem.lower() for f in a.g if f.endswith(".box")]
    pk_names = [Path(f).stem.lower() for f in a.p if f.endswith(".box")]
    matches = [g for g in gt_names if sum(p.startswith(g) for p in pk_names) > 0]
    if a.verbose:
        print(f"Found {len(matches)} boxfile matches\n")
    assert len(matches) > 0, "No paired ground truth and picker particle sets found"
    pairs = []
    for m in matches:
        gp = next(f for f in a.g if Path(f).stem.lower() == m)
        pp = next(f for f in a.p if Path(f).stem.lower().startswith(m))
        pairs.append((read_box_file(gp), read_box_file(pp)))
    scores = score_pairs(pairs, a.c, a.width, a.height)
    rows = []
    for m, (prec, rec, f1, pos) in zip(matches, scores):
        if a.verbose:
            print(f"{m} - precision: {prec:.3f} recall: {rec:.3f} F1-score: {f1:.3f}")
        rows.append((m, prec, rec, f1, pos))
    with open(os.path.join(a.out_dir, "particle_set_comp.tsv"), "wt") as o:
        o.write("\t".join(["filename", "precision", "recall", "f1", "pos_frac"]) + "\n")
        for e in rows:
            o.write("\t".join(str(v) for v in e) + "\n")
    if a.sweep is not None:
        counts, H, W, _ = _sweep(pairs, a.sweep, a.width, a.height)
        write_sweep_tsv(os.path.join(a.out_dir, "particle_set_sweep.tsv"), matches, a.sweep,
                        counts, H, W)
        write_sweep_pooled_tsv(os.path.join(a.out_dir, "particle_set_sweep_pooled.tsv"), a.sweep,
                               counts, H, W)
    if a.match_ji is not None:
        counts = match_pairs(pairs, a.match_ji, a.c)
        write_match_tsv(os.path.join(a.out_dir, "particle_set_match.tsv"), matches, a.match_ji,
                        counts)
        write_match_pooled_tsv(os.path.join(a.out_dir, "particle_set_match_pooled.tsv"),
                               a.match_ji, counts)
    if a.match_sweep is not None:
        counts = match_sweep(pairs, a.match_ji, a.match_sweep)
        write_match_sweep_tsv(os.path.join(a.out_dir, "particle_set_match_sweep.tsv"), matches,
                              a.match_ji, a.match_sweep, counts)
        write_match_sweep_pooled_tsv(
            os.path.join(a.out_dir, "particle_set_match_sweep_pooled.tsv"), a.match_ji,
            a.match_sweep, counts)


if __name__ == "__main__":
    main()
