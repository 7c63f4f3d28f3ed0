"""Shared by the particle-level matching tests: the goldens of
tests/golden/make_score_match_golden.py and a numpy / scipy restatement of the metric
(int64 areas, one f64 division, maximum bipartite matching)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "score_match")


def cases():
    """-> (name, gt (n, 5), picks (n, 5), [(t, edge set of (gt, pick), matching size), ...])"""
    meta = json.load(open(os.path.join(GOLD, "meta.json")))
    arr = np.load(os.path.join(GOLD, "cases.npz"))
    for c in meta["cases"]:
        per_t = [(float.fromhex(h), {(int(g), int(p)) for g, p in e}, int(s))
                 for h, e, s in zip(c["thresh_hex"], c["edges"], c["sizes"])]
        yield c["name"], arr[c["name"] + "_gt"], arr[c["name"] + "_pk"], per_t


def case(name):
    return next(c for c in cases() if c[0] == name)


def rects(a):
    """(n, 4) int64 x0, x1, y0, y1 of (n, >= 4) boxes x, y, w, h: Python round() of each value
    (half to even), unclipped."""
    a = np.asarray(a, dtype=np.float64)
    if a.size == 0:
        return np.zeros((0, 4), np.int64)
    x, y, w, h = (np.array([round(float(v)) for v in a[:, k]], dtype=np.int64) for k in range(4))
    return np.stack([x, x + w, y, y + h], axis=1)


def edge_matrix(gr, pr, t):
    """bool [n_gt, n_pk]: U > 0 and float64(I) / float64(U) > t, boxes without a pixel never."""
    gr, pr = np.asarray(gr, np.int64).reshape(-1, 4), np.asarray(pr, np.int64).reshape(-1, 4)
    a, b = gr[:, None, :], pr[None, :, :]
    ix = np.maximum(0, np.minimum(a[..., 1], b[..., 1]) - np.maximum(a[..., 0], b[..., 0]))
    iy = np.maximum(0, np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 2], b[..., 2]))
    inter = ix * iy
    area = lambda r: (r[..., 1] - r[..., 0]) * (r[..., 3] - r[..., 2])  # noqa: E731
    union = area(a) + area(b) - inter
    ok = ((a[..., 1] > a[..., 0]) & (a[..., 3] > a[..., 2]) &
          (b[..., 1] > b[..., 0]) & (b[..., 3] > b[..., 2]) & (union > 0))
    q = inter.astype(np.float64) / np.where(ok, union, 1).astype(np.float64)
    return ok & (q > t)


def matching_size(E):
    """Size of a maximum matching of the bipartite graph E (bool [n_gt, n_pk])."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import maximum_bipartite_matching
    if E.size == 0 or not E.any():
        return 0
    return int((maximum_bipartite_matching(csr_matrix(E.astype(np.int8)), perm_type="column")
                >= 0).sum())


def kept(pk, conf_thresh):
    """The picks score_detections keeps: dropped iff conf < conf_thresh (NaN is kept)."""
    pk = np.asarray(pk, dtype=np.float64).reshape(-1, 5)
    return pk if conf_thresh is None else pk[~(pk[:, 4] < conf_thresh)]


def oracle(gt, pk, t, conf_thresh=None):
    """-> ((n_gt, n_picked, tp), E) of one pair of (n, 5) box arrays."""
    pk = kept(pk, conf_thresh)
    E = edge_matrix(rects(gt), rects(pk), t)
    return (len(gt), len(pk), matching_size(E)), E


def prf(n_gt, n_picked, tp):
    p = tp / n_picked if n_picked else 0.0
    r = tp / n_gt if n_gt else 0.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def check_assignment(assign, edges, tp, n_gt):
    """`assign` (per kept pick: gt index or -1) is a matching of size tp on `edges`, given as a
    set of (gt, pick) or a bool [n_gt, n_pk] matrix."""
    assign = np.asarray(assign)
    assert assign.dtype == np.int32
    used = assign[assign >= 0]
    assert len(used) == tp, (len(used), tp)
    assert len(set(used.tolist())) == len(used), "a ground-truth box is used twice"
    assert ((assign >= -1) & (assign < max(n_gt, 1))).all()
    for p, g in enumerate(assign.tolist()):
        if g >= 0:
            assert ((g, p) in edges) if isinstance(edges, set) else bool(edges[g, p]), (g, p)
