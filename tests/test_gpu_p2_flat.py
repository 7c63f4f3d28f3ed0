"""P2's flattened stencil walk (rgc_fused.hip: Span / stencil_walk / pairs_fill).

The count walks the two column ranges of a target grid in one loop and the fill replays the
count's bitmask over the same candidate order, so the cases here are small micrographs built
around that order: empty ranges in every position, a stencil at the grid's left and right
border, a box with 40 candidates (the 32-bit mask boundary) at 2, 3 and 4 edges (the
FILL_FAST boundary), waves that mix pickers, a nearly empty second round, and K = 5 / 8.

Every case runs on the integer (f32) layout and, with every coordinate shifted by 0.125, on
the fractional (f64) layout.  The device's (u, v, JI bits) edge set (RGC_F_EDGES hook) must
equal oracle/cpu_ref.edges_faithful's, and the per-micrograph outputs oracle/cpu_ref.micrograph's
(or its NoEdges / NoCliques outcome).  The range patterns the cases are built for are asserted
on the host model of the stencil (tools/p2_trip_model.box_ranges), not assumed.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

pytestmark = pytest.mark.gpu

LAYOUTS = [pytest.param(0.0, id="int"), pytest.param(0.125, id="frac")]


def _mg(pickers, shift, seed=0):
    """k lists of (x, y) -> k (x, y, score) triples, every coordinate moved by `shift`."""
    rng = np.random.default_rng(seed)
    out = []
    for pts in pickers:
        a = np.asarray(pts, np.float64).reshape(-1, 2)
        out.append((a[:, 0] + shift, a[:, 1] + shift, rng.uniform(0.3, 1.0, len(a))))
    return out


def _ranges(mg, box):
    """{(picker, file index): [len of range 0, 1, ...]} from the host model of the stencil."""
    from p2_trip_model import box_ranges
    ln, pk, order = box_ranges(mg, float(box))
    first = np.concatenate([[0], np.cumsum([len(t[0]) for t in mg])])
    return {(int(pk[t]), int(order[t] - first[pk[t]])): ln[t].reshape(-1).tolist()
            for t in range(len(pk))}


def _canon(rows, w, conf, cons):
    perm = np.lexsort(np.asarray(rows).T[::-1]) if len(rows) else np.zeros(0, int)
    return (np.asarray(rows)[perm], np.asarray(w)[perm].view(np.uint32),
            np.asarray(conf)[perm].view(np.uint32), [cons[i] for i in perm])


def _check(mg, box):
    """One micrograph: device edge set and outputs against the oracle.  Returns the edges."""
    from oracle import cpu_ref
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    k = len(mg)
    batch = Batch.pack(k, box, [mg])
    off = batch.box_off
    coords = [[(float(a), float(b), float(c), int(off[p]) + i)
               for i, (a, b, c) in enumerate(zip(*mg[p]))] for p in range(k)]
    want = set()
    for j in range(k):
        for l in range(j + 1, k):
            for (i1, i2, ji) in cpu_ref.edges_faithful(coords[j], coords[l], box):
                want.add((int(off[j]) + i1, int(off[l]) + i2, np.float64(ji).view(np.uint64).item()))
    ctx = _lib.Context(0)
    r = ctx.run(1, k, box, batch.box_off, batch.id_base, batch.x, batch.y, batch.score,
                _lib.F_HOST_OUTPUTS | _lib.F_EDGES)
    u, v, ji = ctx.last_edges()
    assert len(u) == int(r.n_edges)
    got = set(zip(u.tolist(), v.tolist(), ji.view(np.uint64).tolist()))
    assert len(got) == len(u)
    assert got == want
    res = run_batch(ctx, batch)[0]
    ctx.close()
    try:
        o = cpu_ref.micrograph(coords, box, [f"picker{p}" for p in range(k)])
    except cpu_ref.NoEdges:
        assert res.status == _lib.NO_EDGES and not want
        return want
    except cpu_ref.NoCliques:
        assert res.status == _lib.NO_CLIQUES and want
        return want
    assert res.status == _lib.OK
    assert (res.cc_max, res.cc_cnt) == (o["cc_max"], o["cc_cnt"])
    A = o["A"].tocoo()
    C = A.shape[1]
    orows = np.sort(A.row[np.argsort(A.col, kind="stable")].reshape(C, k), axis=1)
    assert res.n_vert == A.shape[0] and len(res.w) == C
    gcons = [(float(batch.x[g]), float(batch.y[g]), int(g)) for g in res.consensus]
    a = _canon(orows, o["w"], o["conf"], o["consensus"])
    b = _canon(res.rows, res.w, res.conf, gcons)
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3]
    return want


# B = 100 on a field of 864 x 540 pixels (the boxes at x = 0, 863 and y = 0, 539 fix it): 8
# columns 108 wide and 10 rows 54 tall, within the cell budget of a 64-box micrograph.
BOX = 100


@pytest.mark.parametrize("shift", LAYOUTS)
def test_empty_ranges_and_grid_borders(shift):
    p0 = [(226, 275),   # 0: left half of column 2 -> columns 1, 2, rows 4..6
          (600, 100),   # 1: nothing near it
          (520, 400),   # 2: right half of column 4 -> columns 4, 5, rows 6..8
          (0, 300),     # 3: leftmost half-column (first stencil column is -1)
          (863, 0),     # 4: rightmost half-column (second stencil column is gx)
          (300, 530)]   # 5: a 3-clique, so the outputs are compared too
    p1 = [(5, 303), (855, 5), (305, 533)]
    p2 = [(210, 275), (545, 405), (298, 539)]
    mg = _mg([p0, p1, p2], shift)
    rg = _ranges(mg, BOX)
    assert rg[(0, 0)] == [0, 0, 1, 0]
    assert rg[(0, 1)] == [0, 0, 0, 0]
    assert rg[(0, 2)] == [0, 0, 0, 1]
    assert rg[(0, 3)] == [0, 1, 0, 0]     # column -1 is no range; its own column holds (5, 303)
    assert rg[(0, 4)] == [1, 0, 0, 0]     # column gx is no range
    edges = _check(mg, BOX)
    assert len(edges) == 4 + 3


def _mask_case(edge_at, k, shift):
    """Picker-0 box P = (460, 275): columns 3, 4 (324..540), rows 4..6 (216..378).
    Picker 1 has 40 candidates in P's stencil, in stencil order: 30 in column 3 (10 per
    row), then 10 in P's own cell of column 4; the candidates `edge_at` are edges of P."""
    assert all(10 <= o < 20 or o >= 30 for o in edge_at)   # (P's row of column 3, or column 4)
    p1 = []
    for o in range(40):
        i = o % 10
        if o < 30:
            p1.append((431, 272 + i) if o in edge_at else (330 + i, 220 + 54 * (o // 10) + i))
        else:
            p1.append((462 + i, 271 + i) if o in edge_at else (535, 272 + i))
    p0 = [(460, 275), (0, 0), (100, 480)]
    p1 += [(105, 483)]
    pickers = [p0, p1]
    if k == 3:
        pickers.append([(863, 539), (98, 484)])
    else:
        p0.append((863, 539))
    return _mg(pickers, shift)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("edge_at", [(31, 38), (30, 33, 39), (12, 31, 32, 39), (33, 35, 37, 39)],
                         ids=["2edges", "3edges", "4edges", "4edges_past_mask"])
def test_mask_boundary(edge_at, k, shift):
    mg = _mask_case(edge_at, k, shift)
    rg = _ranges(mg, BOX)
    assert rg[(0, 0)][:2] == [30, 10] and sum(rg[(0, 0)][2:]) == 0
    edges = _check(mg, BOX)
    # P is box 0 of the batch; picker 1 starts at box len(p0)
    b1 = len(mg[0][0])
    assert sorted(v - b1 for (u, v, _) in edges if u == 0) == list(edge_at)


def _random_mg(k, per, shift, seed, size=2000, box=BOX):
    """`per` boxes per picker (a list gives each picker's count): true centres jittered per
    picker, as the synthetic configs, on integer pixels."""
    rng = np.random.default_rng(seed)
    per = [per] * k if np.isscalar(per) else per
    centres = rng.uniform(0, size, (max(per), 2))
    return _mg([np.rint(centres[:n] + rng.normal(0, 0.08 * box, (n, 2))) for n in per], shift, seed)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("per", [20, 171, 341, (25, 0, 25), (0, 25, 25), 1],
                         ids=["3x20", "n513", "n1023", "empty_picker1", "empty_picker0",
                              "one_box_each"])
def test_wave_composition(per, shift):
    """3 x 20: all pickers in one wave; 513 / 1023 boxes: the second boustrophedon round of a
    512-thread workgroup is one lane / nearly full; a picker without boxes; one box each."""
    size = 4096 if per in (171, 341) else 1000
    mg = _random_mg(3, per, shift, seed=11, size=size)
    edges = _check(mg, BOX)
    if per not in ((0, 25, 25), 1):
        assert edges


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("k", [5, 8])
def test_more_pickers(k, shift):
    """30 boxes per picker in 10 clusters: picker-0 boxes find candidates in several grids
    (2 (K - 1) = 8 and 14 ranges)."""
    rng = np.random.default_rng(k)
    centres = np.repeat(rng.uniform(0, 1500, (10, 2)), 3, axis=0)
    mg = _mg([np.rint(centres + rng.uniform(-45, 45, (30, 2))) for _ in range(k)], shift, k)
    rg = _ranges(mg, BOX)
    grids = max(sum(1 for j in range(k - 1) if v[2 * j] + v[2 * j + 1] > 0)
                for (p, _), v in rg.items() if p == 0)
    both = max(sum(1 for j in range(k - 1) if v[2 * j] > 0 and v[2 * j + 1] > 0)
               for (p, _), v in rg.items() if p == 0)
    assert grids == k - 1 and both >= 2
    assert _check(mg, BOX)
