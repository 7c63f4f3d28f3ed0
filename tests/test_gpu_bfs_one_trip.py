"""P4's clique enumeration around the one-trip form of a BFS level (rgc_fused.hip: BfsLevel::run,
bfs_cliques, bfs_one_trip).

A level (or the root pass) of at most NT entries, NT the threads of the instance, runs as one
body per thread around a one-barrier scan; a larger one takes the count / scan / fill form.  Both
must number the entries alike, so a micrograph may mix them level by level.  The instances with
K <= 3 and up to 768 threads select the one-trip form; the others keep the general form alone,
and their cases here hold them to the same outputs.

Cases are small clusters 300 px apart: one picker-0 box and a_p boxes of picker p = 1..K-1
within +-4 px of it, so every cross-picker pair of a cluster is an edge (JI >= 0.73): a cluster
(a_1, a_2, ...) gives a_1 level-2 entries, a_1 a_2 level-3 entries, and so on.  Lone boxes steer
the number of roots (the root pass runs over every picker-0 box) and the size class, which
decides the instance (K = 3, integer layout: 256 threads up to 512 boxes, 512 threads up to
1408; K = 5: 768 threads for 1409..2560; K = 4: 1024 threads, with the wide-entry HBM slot,
above 2560).  Every case asserts its level sizes on the oracle's edge list, and is compared bit
for bit with the oracle and the fused route with the multi-kernel route.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_p2_flat import BOX, LAYOUTS, _check, _mg
from test_gpu_p2_onepass import _fields, _routes_equal
from test_gpu_parity import _check_vs_oracle, _dense_clusters

pytestmark = pytest.mark.gpu

OFFS = [(dx, dy) for dx in range(-4, 5) for dy in range(-4, 5)]   # 81 distinct pixels
PITCH, COLS = 300, 40
# total boxes of a micrograph (integer layout) for which the host picks the instance
BOXES = {256: (1, 512), 512: (513, 1408), 768: (1409, 2560), 1024: (2561, 4608)}


def _slot(s):
    return PITCH * (s % COLS) + 10, PITCH * (s // COLS) + 10


def _clusters(spec, lone, k=3, shift=0.0):
    """spec: one tuple (a_1 .. a_{k-1}) per cluster; lone: boxes without neighbours per picker."""
    pk = [[] for _ in range(k)]
    s = 0
    for c in spec:
        cx, cy = _slot(s)
        s += 1
        pk[0].append((cx, cy))
        for p in range(1, k):
            assert c[p - 1] <= len(OFFS)
            pk[p] += [(cx + OFFS[i][0], cy + OFFS[i][1]) for i in range(c[p - 1])]
    for p in range(k):
        for _ in range(lone[p] if p < len(lone) else 0):
            pk[p].append(_slot(s))
            s += 1
    return _mg(pk, shift, seed=len(spec))


def _level_sizes(mg, box=BOX):
    """[roots, level 2, .., level k] of the level-synchronous enumeration, from the oracle's edges:
    the roots are the picker-0 boxes, level d + 1 the picker-d neighbours of a prefix's last
    member that are neighbours of every earlier member."""
    from oracle import cpu_ref
    k = len(mg)
    coords = [[(float(a), float(b), float(c), i) for i, (a, b, c) in enumerate(zip(*mg[p]))]
              for p in range(k)]
    nb = {}
    for j in range(k):
        for l in range(j + 1, k):
            for (i1, i2, _) in cpu_ref.edges_vectorised(coords[j], coords[l], box):
                nb.setdefault((j, i1, l), set()).add(i2)
    sizes = [len(coords[0])]
    level = [(r,) for r in range(len(coords[0]))]
    for d in range(1, k):
        nxt = []
        for pre in level:
            cand = nb.get((d - 1, pre[-1], d), set())
            for q in range(d - 1):
                cand = cand & nb.get((q, pre[q], d), set())
            nxt += [pre + (h,) for h in sorted(cand)]
        sizes.append(len(nxt))
        level = nxt
    return sizes


def _both(mg, k=3, get_cc=False):
    """Edges and outputs against the oracle, then the other route.  Returns the result."""
    _check(mg, BOX)
    if get_cc:
        _check_vs_oracle([mg], k, BOX, get_cc=True)
    return _routes_equal([mg], k, BOX, get_cc=get_cc)[0]


def _n(mg):
    return sum(len(t[0]) for t in mg)


def _k3_cases():
    """(id, NT, spec, lone, sizes) around NT roots, level-2 entries and cliques."""
    out = []
    for nt in (256, 512):
        g = nt // 16
        for d in (-1, 0, 1):
            # roots: 10 clusters of four cliques, the other picker-0 boxes alone
            out.append((f"roots{nt + d}", nt, [(2, 2)] * 10, (nt + d - 10, 0, 0),
                        [nt + d, 20, 40]))
            # level 2 and cliques together: clusters of 16 x 1, the last one 15 / 16 / 17
            out.append((f"level2_and_3_{nt + d}", nt, [(16, 1)] * (g - 1) + [(16 + d, 1)],
                        (0, 0, 0), [g, nt + d, nt + d]))
        # cliques alone: 4 x 4 clusters; level 2 far below NT
        fill = (0, 0, 300) if nt == 512 else (0, 0, 0)
        out.append((f"level3_{nt - 1}", nt, [(4, 4)] * (g - 1) + [(3, 5)], fill,
                    [g, 4 * g - 1, nt - 1]))
        out.append((f"level3_{nt}", nt, [(4, 4)] * g, fill, [g, 4 * g, nt]))
        out.append((f"level3_{nt + 1}", nt, [(4, 4)] * g + [(1, 1)], fill,
                    [g + 1, 4 * g + 1, nt + 1]))
        # level 2 in one trip, level 3 not
        out.append((f"level2_fits_level3_not_{nt}", nt, [(4, 4)] * (g + g // 4),
                    (0, 200, 0) if nt == 512 else (0, 0, 0),
                    [g + g // 4, 4 * (g + g // 4), 16 * (g + g // 4)]))
        # level 2 above NT (clusters without a picker-2 box add entries, no cliques), level 3 below
        m = g + 1
        out.append((f"level3_fits_level2_not_{nt}", nt, [(16, 1)] * 8 + [(16, 0)] * m, (0, 0, 0),
                    [8 + m, 16 * (8 + m), 128]))
    return [pytest.param(*c[1:], id=c[0]) for c in out]


@pytest.mark.parametrize("nt,spec,lone,sizes", _k3_cases())
def test_trip_boundary_k3(nt, spec, lone, sizes):
    mg = _clusters(spec, lone)
    assert BOXES[nt][0] <= _n(mg) <= BOXES[nt][1]
    assert _level_sizes(mg) == sizes
    r = _both(mg)
    assert len(r.w) == sizes[-1]


@pytest.mark.parametrize("shift", LAYOUTS)
def test_mixed_forms_both_layouts(shift):
    """Level 2 in one trip and level 3 not, and the reverse, in one batch, on both layouts."""
    a = _clusters([(4, 4)] * 40, (0, 200, 0), shift=shift)
    b = _clusters([(16, 1)] * 8 + [(16, 0)] * 25, (0, 0, 0), shift=shift)
    assert _level_sizes(a) == [40, 160, 640] and _level_sizes(b) == [33, 528, 128]
    _check_vs_oracle([a, b], 3, BOX)
    res = _routes_equal([a, b], 3, BOX)
    assert [len(r.w) for r in res] == [640, 128]


def _run_384():
    """(child process, RGC_DIAG_NT=384) the level-2 / clique boundary of the 384-thread
    instance, which the host's plan selects only when asked to."""
    for d in (-1, 0, 1):
        mg = _clusters([(16, 1)] * 23 + [(16 + d, 1)], (0, 0, 0))
        assert _level_sizes(mg) == [24, 384 + d, 384 + d]
        assert len(_both(mg).w) == 384 + d
        mg = _clusters([(2, 2)] * 10, (384 + d - 10, 0, 0))
        assert _level_sizes(mg) == [384 + d, 20, 40]
        assert len(_both(mg).w) == 40


def test_trip_boundary_384():
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, RGC_DIAG_NT="384", PYTHONPATH=os.pathsep.join(
        [root, os.path.join(root, "repic-copy_amd"), here, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c",
                        "import test_gpu_bfs_one_trip as t; t._run_384(); print('OK')"],
                       env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_trip_boundary_k5_768(d):
    """K = 5 on 768 threads: every level 2..5 at 767 (all within one trip), 768, and 769 (none)."""
    spec = [(4, 1, 1, 1)] * 191 + [(4 + d, 1, 1, 1)]
    mg = _clusters(spec, (0,) * 5, k=5)
    assert BOXES[768][0] <= _n(mg) <= BOXES[768][1]
    assert _level_sizes(mg) == [192] + [768 + d] * 4
    _check_vs_oracle([mg], 5, BOX)
    assert len(_routes_equal([mg], 5, BOX)[0].w) == 768 + d


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_trip_boundary_k4_1024(d):
    """K = 4 on 1024 threads (the wide-entry HBM slot): roots and every level at 1023 .. 1025."""
    spec = [(4, 1, 1)] * 255 + [(4 + d, 1, 1)]
    mg = _clusters(spec, (1024 + d - 256, 300, 0, 0), k=4)
    assert BOXES[1024][0] <= _n(mg) <= BOXES[1024][1]
    assert _level_sizes(mg) == [1024 + d] * 4
    _check_vs_oracle([mg], 4, BOX)
    assert len(_routes_equal([mg], 4, BOX)[0].w) == 1024 + d


def _wide_segment(shift):
    """One picker-0 box P and one picker-1 box Q 30 px right of it; 44 picker-2 boxes, every
    one an edge of Q: 40 near P (edges of P: cliques) and 4 about 40 px right of Q (JI with P
    below 0.2).  Q's level-2 entry has 44 candidates and 40 extensions, so at least 8 extensions
    lie past bit 31 whatever the sorted order."""
    p2 = []
    for i in range(44):
        x = 1068 + (i % 4) if i % 11 == 5 else 1027 + (i % 4)
        p2.append((x, 989 + i // 2))
    return _mg([[(1000, 1000), (10, 10)], [(1030, 1000), (3000, 2000)], p2], shift)


@pytest.mark.parametrize("shift", LAYOUTS)
def test_more_than_32_candidates(shift):
    mg = _wide_segment(shift)
    from oracle import cpu_ref
    c = [[(float(a), float(b), float(s), i) for i, (a, b, s) in enumerate(zip(*mg[p]))]
         for p in range(3)]
    assert len(cpu_ref.edges_vectorised(c[1], c[2], BOX)) == 44
    assert _level_sizes(mg) == [2, 1, 40]
    assert len(_both(mg).w) == 40


@pytest.mark.parametrize("k,per,n_clusters", [(3, 12, 3), (3, 10, 4), (5, 4, 2), (5, 3, 6)])
def test_level_overflow(k, per, n_clusters):
    """Dense clusters (per ** k cliques each): a level of few entries, expanded in one trip,
    overflows the queue region: K = 3 falls back to the DFS, K = 5 to root chunks rebuilt in
    P6."""
    mgs = [_dense_clusters(k, per, n_clusters, seed) for seed in range(2)]
    _check_vs_oracle(mgs, k, BOX)
    _check_vs_oracle(mgs, k, BOX, get_cc=True)
    _routes_equal(mgs, k, BOX)


def test_zero_valid_roots():
    """Edges between pickers 1 and 2 only: every root's list is empty (NoCliques); and no
    picker-0 box at all."""
    from repic_amd import _lib
    p12 = [(500 + 300 * i, 500) for i in range(5)]
    mg = _mg([[(10, 10), (2000, 10)], p12, [(x + 3, y - 2) for (x, y) in p12]], 0.0)
    assert _level_sizes(mg) == [2, 0, 0]
    assert len(_check(mg, BOX)) == 5
    assert _routes_equal([mg], 3, BOX)[0].status == _lib.NO_CLIQUES
    mg = _mg([[], p12, [(x + 3, y - 2) for (x, y) in p12]], 0.0)
    _check(mg, BOX)
    assert _routes_equal([mg], 3, BOX)[0].status == _lib.NO_CLIQUES


@pytest.mark.parametrize("get_cc", [False, True])
def test_one_root_and_empty_first_segment(get_cc):
    """One root with a clique; with a second root whose only edge goes to picker 2 (its first
    segment is empty: no level-2 entry)."""
    one = _clusters([(2, 3)], (0, 1, 1))
    assert _level_sizes(one) == [1, 2, 6]
    assert len(_both(one, get_cc=get_cc).w) == 6
    pk = [[(10, 10), (1000, 10)], [(12, 8), (14, 12)], [(9, 13), (1003, 8)]]
    two = _mg(pk, 0.0)
    assert _level_sizes(two) == [2, 2, 2]
    assert len(_both(two, get_cc=get_cc).w) == 2


def test_get_cc_counts_target_roots_only():
    """--get_cc: only the largest component's roots expand.  A 3 x 3 cluster (the target, 9
    cliques) among 100 single cliques and 160 lone roots: 261 roots on 256 threads, 109 cliques
    without --get_cc."""
    mg = _clusters([(3, 3)] + [(1, 1)] * 100, (160, 0, 0))
    assert _n(mg) <= 512 and _level_sizes(mg) == [261, 103, 109]
    assert len(_both(mg).w) == 109
    _check_vs_oracle([mg], 3, BOX, get_cc=True)
    assert len(_routes_equal([mg], 3, BOX, get_cc=True)[0].w) == 9


@pytest.mark.parametrize("d", [-1, 0, 1])
@pytest.mark.parametrize("nt", [256, 512])
def test_k2_last_level_is_level_2(nt, d):
    """K = 2: the root pass writes the cliques themselves.  Roots and cliques around NT."""
    g = nt // 16
    fill = 300 if nt == 512 else 0
    mg = _clusters([(16,)] * (g - 1) + [(16 + d,)], (fill, 0), k=2)
    assert BOXES[nt][0] <= _n(mg) <= BOXES[nt][1]
    assert _level_sizes(mg) == [g + fill, nt + d]
    assert len(_both(mg, k=2).w) == nt + d
    mg = _clusters([(2,)] * 10, (nt + d - 10, 300 if nt == 512 else 0), k=2)
    assert BOXES[nt][0] <= _n(mg) <= BOXES[nt][1]
    assert _level_sizes(mg) == [nt + d, 20]
    assert len(_both(mg, k=2).w) == 20


def test_dense_batch_repeats():
    """C2 micrographs, the boundary micrographs that mix both forms and an overflowing one,
    five times on one context: equal array by array."""
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch, run_batch
    cfg = synth.SynthConfig(**synth.CONFIGS["C2"], seed=9)
    mgs = synth.batch(cfg, 96)
    mgs += [_clusters([(4, 4)] * 40, (0, 200, 0)), _clusters([(16, 1)] * 8 + [(16, 0)] * 25, (0,) * 3),
            _clusters([(16, 1)] * 31 + [(17, 1)], (0,) * 3), _dense_clusters(3, 10, 4, seed=1)] * 4
    batch = Batch.pack(cfg.k, cfg.box, mgs)
    ctx = _lib.Context(0)
    runs = []
    for _ in range(5):
        res = run_batch(ctx, batch)
        runs.append([(_fields(r), r.rows.copy(), r.w.copy(), r.conf.copy(), r.consensus.copy())
                     for r in res])
    ctx.close()
    assert all(f[0][0] == _lib.OK for f in runs[0])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a[0] == b[0]
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y)
