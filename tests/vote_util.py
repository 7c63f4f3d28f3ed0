"""Plain-Python model of ``repic consensus --min_pickers`` (include/repic_gc.h,
rgc_consensus_tiers): which boxes a list of picks explains, the pseudo-micrographs of a tier,
their columns by the CPU oracle (``oracle.cpu_ref.micrograph`` per picker subset) and the tier's
optimum by ``oracle.ilp_ref.milp``.

A batch is ``repic_amd.pipeline.Batch``-like: ``k``, ``box_size``, ``box_off``, ``id_base``,
``x``, ``y``, ``score``; box indices are batch indices throughout.
"""
from __future__ import annotations

import itertools
import math
import os
import types

import numpy as np
from scipy.sparse import coo_matrix

from nms_util import jaccard
from oracle import cpu_ref, ilp_ref


def explains(bx, by, cx, cy, box, t):
    """Pick (cx, cy) explains box (bx, by): the reference quotient exceeds t, strictly; a
    non-finite coordinate explains / is explained by nothing."""
    if not all(math.isfinite(v) for v in (bx, by, cx, cy)):
        return False
    return jaccard(bx, by, cx, cy, float(box)) > t


def mark_explained(box_tier, b, m, picks, tier, t):
    """``box_tier`` (in place): boxes of micrograph m still at 0 that a pick of ``picks``
    ((cx, cy) pairs, unrounded) explains get ``tier``."""
    k = b.k
    b0, b1 = int(b.box_off[m * k]), int(b.box_off[(m + 1) * k])
    if not len(picks):
        return
    px = np.array([p[0] for p in picks], np.float64)
    py = np.array([p[1] for p in picks], np.float64)
    box = float(b.box_size)
    for i in range(b0, b1):
        if box_tier[i] != 0:
            continue
        x, y = float(b.x[i]), float(b.y[i])
        # candidates by a loose window (numpy), the decision in Python floats
        near = np.flatnonzero((np.abs(px - x) <= box) & (np.abs(py - y) <= box))
        if any(explains(x, y, float(px[j]), float(py[j]), box, t) for j in near):
            box_tier[i] = tier


def subsets(k, t):
    """Picker subsets of size t in ascending order of the index tuple."""
    return list(itertools.combinations(range(k), t))


def mask_of(S):
    return sum(1 << p for p in S)


def pseudo_micrographs(b, m, box_tier, t):
    """The submitted pseudo-micrographs of micrograph m at tier t: [(S, [batch indices of the
    unexplained boxes of picker p, file order, for p in S])]; one with an empty segment is
    left out."""
    k = b.k
    out = []
    for S in subsets(k, t):
        segs = []
        for p in S:
            a, e = int(b.box_off[m * k + p]), int(b.box_off[m * k + p + 1])
            segs.append([i for i in range(a, e) if box_tier[i] == 0])
        if all(segs):
            out.append((S, segs))
    return out


class _Threshold:
    """The CPU oracle reads its module-level THRESHOLD at call time."""

    def __init__(self, t):
        self.t = t

    def __enter__(self):
        self.old = cpu_ref.THRESHOLD
        cpu_ref.THRESHOLD = self.t

    def __exit__(self, *a):
        cpu_ref.THRESHOLD = self.old


def _cliques(coords, box, t):
    """Every tuple of one box per picker (positions) that is pairwise joined."""
    n = len(coords)
    adj = {}
    for j, l in itertools.combinations(range(n), 2):
        for i1, i2, _ in cpu_ref.edges_vectorised(coords[j], coords[l], box):
            adj.setdefault((j, i1), set()).add((l, i2))
            adj.setdefault((l, i2), set()).add((j, i1))
    out = []

    def extend(chosen):
        p = len(chosen)
        if p == n:
            out.append(tuple(i for _, i in chosen))
            return
        cands = (range(len(coords[0])) if p == 0 else
                 sorted(i for (q, i) in adj.get(chosen[0], ()) if q == p))
        for i in cands:
            if all((p, i) in adj.get(c, ()) for c in chosen):
                extend(chosen + [(p, i)])
    extend([])
    return out


def subset_columns(b, m, S, segs, t):
    """The columns of one pseudo-micrograph by the CPU oracle: {members (batch indices, picker
    order of S): (w float32, conf float32, batch index of the consensus box)}; {} when the oracle
    raises NoEdges / NoCliques."""
    idb = int(b.id_base[m])
    coords, origin = [], []
    for seg in segs:
        coords.append([(float(b.x[i]), float(b.y[i]), float(b.score[i]), idb + len(origin) + j)
                       for j, i in enumerate(seg)])
        origin.extend(seg)
    methods = [f"picker{p}" for p in S]
    with _Threshold(t):
        try:
            o = cpu_ref.micrograph(coords, b.box_size, methods)
        except (cpu_ref.NoEdges, cpu_ref.NoCliques):
            return {}
        cl = _cliques(coords, b.box_size, t)
    # the oracle's rows are ranks of the clique vertices sorted by (x, y, id)
    key = lambda p, i: (coords[p][i][0], coords[p][i][1], coords[p][i][3])  # noqa: E731
    verts = sorted({key(p, i) for c in cl for p, i in enumerate(c)})
    A = o["A"].tocoo()
    assert A.shape == (len(verts), len(cl)), (A.shape, len(verts), len(cl))
    row_of = {v: r for r, v in enumerate(verts)}
    C = A.shape[1]
    orows = np.sort(A.row[np.argsort(A.col, kind="stable")].reshape(C, len(S)), axis=1)
    by_rows = {tuple(r.tolist()): j for j, r in enumerate(orows)}
    assert len(by_rows) == C
    out = {}
    for c in cl:
        j = by_rows[tuple(sorted(row_of[key(p, i)] for p, i in enumerate(c)))]
        cid = o["consensus"][j][2]
        off = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
        members = tuple(origin[int(off[p]) + i] for p, i in enumerate(c))
        out[members] = (np.float32(o["w"][j]), np.float32(o["conf"][j]), origin[cid - idb])
    return out


def tier_columns(b, m, box_tier, tier, t):
    """All columns of micrograph m at ``tier``: [(S, {members: (w, conf, cons)})] in subset
    order, over the boxes with box_tier == 0."""
    return [(S, subset_columns(b, m, S, segs, t))
            for S, segs in pseudo_micrographs(b, m, box_tier, tier)]


def tier_optimum(cols):
    """The value of the best packing of a tier's columns (HiGHS, zero gap): columns of all
    subsets jointly, rows = batch boxes, weights widened to f64."""
    members = [mem for _, d in cols for mem in d]
    w = np.array([float(d[mem][0]) for _, d in cols for mem in d], np.float64)
    if not members:
        return 0.0
    boxes = sorted({i for mem in members for i in mem})
    row = {v: r for r, v in enumerate(boxes)}
    rows = [row[i] for mem in members for i in mem]
    cs = [j for j, mem in enumerate(members) for _ in mem]
    A = coo_matrix((np.ones(len(rows), np.int64), (rows, cs)), shape=(len(boxes), len(members)))
    return ilp_ref.milp(A, w)[1]


def largest_component(cols):
    members = [mem for _, d in cols for mem in d]
    if not members:
        return 0
    boxes = sorted({i for mem in members for i in mem})
    row = {v: r for r, v in enumerate(boxes)}
    rows = [row[i] for mem in members for i in mem]
    cs = [j for j, mem in enumerate(members) for _ in mem]
    A = coo_matrix((np.ones(len(rows), np.int64), (rows, cs)), shape=(len(boxes), len(members)))
    _, lab = ilp_ref.components(A)
    return int(np.bincount(lab).max())


def load_dir(in_dir, n_first=None):
    """BOX directories -> (methods, bases, micrographs as k (x, y, score) triples), scores as
    the ingest hands them to the device (sigmoid where a file has a negative score)."""
    from repic_amd.ingest import sigmoid
    methods = sorted(d for d in os.listdir(in_dir) if os.path.isdir(os.path.join(in_dir, d)))
    bases = sorted(f[:-4] for f in os.listdir(os.path.join(in_dir, methods[0]))
                   if f.endswith(".box"))
    bases = bases[:n_first]
    mgs = []
    for base in bases:
        mg = []
        for p in methods:
            x, y, s = cpu_ref.parse_box(os.path.join(in_dir, p, base + ".box"))
            x, y, s = (np.asarray(v, np.float64) for v in (x, y, s))
            mg.append((x, y, sigmoid(s) if len(s) and s.min() < 0 else s))
        mgs.append(mg)
    return methods, bases, mgs


def hand_batch():
    """k = 3, box 10, one micrograph.  A: all three pickers; B: pickers 0 and 1; C: pickers 1 and
    2; D: picker 0 alone; picker 2 has a duplicate overlapping A.  Batch indices:
    picker 0: 0 A, 1 B, 2 D; picker 1: 3 A, 4 B, 5 C; picker 2: 6 A, 7 duplicate, 8 C."""
    x = np.array([100, 200, 400, 101, 201, 300, 100, 103, 300], np.float64)
    y = np.array([100, 200, 400, 100, 200, 300, 101, 103, 301], np.float64)
    s = np.array([0.9, 0.8, 0.7, 0.9, 0.8, 0.6, 0.9, 0.9, 0.6], np.float64)
    return types.SimpleNamespace(k=3, box_size=10, n_mg=1, box_off=np.array([0, 3, 6, 9], np.int64),
                                 id_base=np.array([0], np.int64), x=x, y=y, score=s)
