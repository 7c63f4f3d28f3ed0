"""CPU oracle of the picker-agreement contract (include/repic_gc.h, rgc_agreement), written from
the contract text: numpy f64 operations in the order of ``oracle.cpu_ref.edges_vectorised``
(itself the reference's get_jaccard / calc_jaccard, get_cliques.py:40-46,59-69).

Two boxes of one micrograph and different pickers are joined iff ``|dx| <= B`` and the quotient
exceeds the threshold, strictly.  ``oracle`` looks, per box, only at the boxes of the other
segment within an x-window far wider than any rounding (a bisect on the sorted x); ``brute`` puts
every pair, non-finite coordinates included, through the formula and is the check of the window
and of "a non-finite box is joined to nothing".
"""
from __future__ import annotations

import types

import numpy as np


def _ji(x, y, a, b, box):
    """(prefilter, quotient) of box pairs, arrays broadcast; edges_vectorised's op order."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        pre = np.abs(x - a) <= box
        xo = np.maximum((np.minimum(x, a) + box) - np.maximum(x, a), 0.0)
        yo = np.maximum((np.minimum(y, b) + box) - np.maximum(y, b), 0.0)
        inter = xo * yo
        ji = inter / (np.float64(2 * box ** 2) - inter)
    return pre, ji


def pair_edges_window(px, py, qx, qy, box, t):
    """Joined pairs between two segments -> (i, j, ji) arrays, i / j indices in P / Q, in
    ascending (i, j)."""
    box = int(box)
    px, py, qx, qy = (np.asarray(v, np.float64) for v in (px, py, qx, qy))
    pf = np.flatnonzero(np.isfinite(px) & np.isfinite(py))
    qf = np.flatnonzero(np.isfinite(qx) & np.isfinite(qy))
    if not len(pf) or not len(qf):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    qs = qf[np.argsort(qx[qf], kind="stable")]
    sx = qx[qs]
    m = box + (np.abs(px[pf]) + box) * 1e-9
    lo = np.searchsorted(sx, px[pf] - m, "left")
    hi = np.searchsorted(sx, px[pf] + m, "right")
    cnt = hi - lo
    tot = int(cnt.sum())
    i = np.repeat(pf, cnt)
    pos = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    j = qs[pos]
    pre, ji = _ji(px[i], py[i], qx[j], qy[j], box)
    e = pre & (ji > t)
    i, j, ji = i[e], j[e], ji[e]
    o = np.lexsort((j, i))
    return i[o], j[o], ji[o]


def pair_edges_brute(px, py, qx, qy, box, t):
    """The same from the full matrix, every box through the formula."""
    box = int(box)
    px, py, qx, qy = (np.asarray(v, np.float64) for v in (px, py, qx, qy))
    if not len(px) or not len(qx):
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    pre, ji = _ji(px[:, None], py[:, None], qx[None, :], qy[None, :], box)
    i, j = np.nonzero(pre & (ji > t))
    return i, j, ji[i, j]


def oracle(n_mg, k, box_size, box_off, x, y, t=0.3, edges=pair_edges_window):
    """Every output of the contract -> a namespace with support, partner [N, k], partner_ji
    [N, k], pair_edges / pair_supported / pair_mutual [n_mg, k, k]."""
    off = np.asarray(box_off, np.int64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = int(off[-1]) if n_mg * k > 0 else 0
    sup = np.zeros(n, np.uint8)
    part = np.full((n, k), -1, np.int32)
    pji = np.zeros((n, k), np.float64)
    pe = np.zeros((n_mg, k, k), np.int64)
    ps = np.zeros((n_mg, k, k), np.int64)
    pm = np.zeros((n_mg, k, k), np.int64)
    t = float(t)
    for m in range(n_mg):
        for p in range(k):
            p0, p1 = int(off[m * k + p]), int(off[m * k + p + 1])
            for q in range(k):
                if q == p:
                    continue
                q0, q1 = int(off[m * k + q]), int(off[m * k + q + 1])
                i, j, ji = edges(x[p0:p1], y[p0:p1], x[q0:q1], y[q0:q1], box_size, t)
                pe[m, p, q] = len(i)
                if not len(i):
                    continue
                # per box the largest JI, ties to the lowest index
                o = np.lexsort((j, -ji, i))
                i, j, ji = i[o], j[o], ji[o]
                bi, first = np.unique(i, return_index=True)
                ps[m, p, q] = len(bi)
                sup[p0 + bi] |= np.uint8(1 << q)
                part[p0 + bi, q] = q0 + j[first]
                pji[p0 + bi, q] = ji[first]
    for m in range(n_mg):
        for p in range(k):
            p0, p1 = int(off[m * k + p]), int(off[m * k + p + 1])
            b = np.arange(p0, p1)
            for q in range(k):
                if q == p:
                    continue
                c = part[b, q]
                has = c >= 0
                pm[m, p, q] = int((part[c[has], p] == b[has]).sum())
    return types.SimpleNamespace(n_mg=n_mg, k=k, support=sup, partner=part, partner_ji=pji,
                                 pair_edges=pe, pair_supported=ps, pair_mutual=pm)


def oracle_device_call(ctx, batch, ji_threshold, partners=False, timing=False):
    """Drop-in for ``repic_amd.agreement.device_call`` without a device."""
    r = oracle(batch.n_mg, batch.k, batch.box_size, batch.box_off, batch.x, batch.y,
               ji_threshold)
    if not partners:
        r.partner = r.partner_ji = None
    return r, (0, 0), []


def pack(k, mgs):
    """(n_mg, box_off, x, y) from micrographs given as k (x, y) pairs of sequences each."""
    cnt, xs, ys = [], [], []
    for mg in mgs:
        assert len(mg) == k
        for sx, sy in mg:
            assert len(sx) == len(sy)
            cnt.append(len(sx))
            xs.extend(float(v) for v in sx)
            ys.extend(float(v) for v in sy)
    off = np.concatenate([[0], np.cumsum(np.array(cnt, np.int64))]).astype(np.int64)
    return len(mgs), off, np.array(xs, np.float64), np.array(ys, np.float64)


FIELDS = ("support", "partner", "partner_ji", "pair_edges", "pair_supported", "pair_mutual")


def assert_same(got, want, partners=True):
    """Every array exactly, partner_ji by bits."""
    for f in FIELDS:
        g, w = getattr(got, f), getattr(want, f)
        if f in ("partner", "partner_ji") and not partners:
            assert g is None, f
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (f, g.shape, w.shape, g.dtype, w.dtype)
        if f == "partner_ji":
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.argwhere(g != w)
        assert not len(bad), (f, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
