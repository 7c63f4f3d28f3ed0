"""Inputs of tests/test_gpu_consensus_tiers_deep.py and the model's own cascade over them
(tests/test_consensus_tiers_models.py pins what each input is for, without a device).

* ``synth_batch``: seeded synthetic batches at k = 5 and k = 8 (cascades of 3 to 6 lower tiers)
* ``two_live`` / ``three_live`` / ``all_explained``: hand cases of the rule that ends the loop
* ``lattice_mg``: k = 3 micrographs whose tier-3 or tier-2 runs leave the fused kernel
* ``cascade``: tiers k .. M by the model alone, each tier's picks a HiGHS optimum

Nothing here loads the native library: ``pack`` is ``repic_amd.pipeline.Batch.pack`` restated.
"""
from __future__ import annotations

import types

import numpy as np
from scipy.sparse import coo_matrix

import vote_util as vu
from oracle import ilp_ref

ILP_BIG = 4096            # rgc_ilp.hip: the largest conflict component that is searched exactly
FUSED_MAX_BOXES = 4608    # rgc_run.cpp: a larger micrograph is deferred from the fused kernel


def pack(k, box, mgs, id_bases=None):
    """``Batch.pack``: micrographs (k (x, y, score) triples each) -> a Batch-like namespace."""
    counts = np.array([len(t[0]) for mg in mgs for t in mg], np.int64)
    assert len(counts) == len(mgs) * k
    box_off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=box_off[1:])
    if id_bases is None:
        id_bases = np.concatenate([[0], np.cumsum(counts.reshape(-1, k).sum(axis=1))[:-1]])
    cat = lambda j: np.ascontiguousarray(  # noqa: E731
        np.concatenate([t[j] for mg in mgs for t in mg]), np.float64)
    return types.SimpleNamespace(k=k, box_size=int(box), n_mg=len(mgs), box_off=box_off,
                                 id_base=np.ascontiguousarray(id_bases, np.int64),
                                 x=cat(0), y=cat(1), score=cat(2))


def micrographs(b):
    """The micrographs of a batch again, as ``pack`` takes them."""
    k = b.k
    return [[(b.x[a:e], b.y[a:e], b.score[a:e])
             for a, e in zip(b.box_off[m * k:(m + 1) * k], b.box_off[m * k + 1:(m + 1) * k + 1])]
            for m in range(b.n_mg)]


def one(b, m):
    """Micrograph m of a batch alone, its id base kept (the consensus tie-break hashes ids)."""
    return pack(b.k, b.box_size, [micrographs(b)[m]], id_bases=b.id_base[m:m + 1])


# ----------------------------------------------------------------------------- synthetic cascades
SYNTH_BOX = 64
# name: generator settings, micrographs, M, the tiers that have picks in every micrograph and the
# tiers without a column (both pinned by tests/test_consensus_tiers_models.py)
SYNTH = {
    "k5": dict(k=5, n_true=40, keep=0.6, seed=1, n_mg=2, M=2, populated=(5, 4, 3, 2), empty=()),
    "k8_m2": dict(k=8, n_true=30, keep=0.55, seed=2, n_mg=1, M=2, populated=(8, 6, 5, 4, 3, 2),
                  empty=(7,)),
    "k8_m6": dict(k=8, n_true=30, keep=0.8, seed=3, n_mg=1, M=6, populated=(8, 7, 6), empty=()),
}


def synth_config(name, frac=False):
    from repic_amd import synth
    c = SYNTH[name]
    return synth.SynthConfig(k=c["k"], n_true=c["n_true"], box=SYNTH_BOX, width=1024, height=1024,
                             keep=c["keep"], dup=0.1, frac=frac, seed=c["seed"])


def synth_batch(name, frac=False, n_mg=None, id_bases=None):
    from repic_amd import synth
    cfg = synth_config(name, frac)
    mgs = synth.batch(cfg, SYNTH[name]["n_mg"] if n_mg is None else n_mg)
    return pack(cfg.k, cfg.box, mgs, id_bases=id_bases)


# ----------------------------------------------------------------------------- the loop's end
def _hand(k, pickers):
    """One micrograph, box 10, from per-picker lists of (x, y, score)."""
    mg = [tuple(np.array([v[j] for v in p], np.float64) for j in range(3)) for p in pickers]
    assert len(mg) == k
    return mg


_A = [(100, 100, 0.9), (101, 100, 0.9), (100, 101, 0.9), (101, 101, 0.9)]   # a box per picker
_B = [(200, 200, 0.8), (201, 200, 0.7)]                                     # pickers 0, 1
_C = [(300, 300, 0.6), (301, 300, 0.5), (300, 301, 0.4)]                    # pickers 0, 1, 2


def two_live():
    """k = 4.  A by all four pickers, B by pickers 0 and 1; pickers 2 and 3 have their A box
    only.  Boxes: picker 0: 0 A, 1 B; picker 1: 2 A, 3 B; picker 2: 4 A; picker 3: 5 A.  After
    tier 4 pickers 0 and 1 are live: tier 3 submits nothing, tier 2 the subset {0, 1}."""
    return _hand(4, [[_A[0], _B[0]], [_A[1], _B[1]], [_A[2]], [_A[3]]])


TWO_LIVE_BOX_TIER = [4, 2, 4, 2, 4, 4]


def three_live():
    """``two_live`` and a triple C by pickers 0, 1 and 2: tier 3 submits {0, 1, 2}."""
    return _hand(4, [[_A[0], _B[0], _C[0]], [_A[1], _B[1], _C[1]], [_A[2], _C[2]], [_A[3]]])


def all_explained():
    """k = 5.  Two particles, each seen by all five pickers: after tier 5 no picker is live."""
    pk = [[(100 + (p & 1), 100 + (p >> 1), 0.9), (400 + (p >> 1), 200 + (p & 1), 0.5 + 0.05 * p)]
          for p in range(5)]
    return _hand(5, pk)


# ----------------------------------------------------------------------------- routes in a tier
def lattice_mg(per_picker, n_triples=50, n_pairs=60, seed=11):
    """k = 3, box 10: ``n_triples`` particles by all three pickers, ``n_pairs`` by each pair of
    pickers, the rest of a picker's ``per_picker`` boxes alone.  Each group has a slot of its own
    on a 40-pixel lattice (its boxes at most 1 pixel apart), so only planted groups overlap;
    every picker's file order is shuffled."""
    rng = np.random.default_rng(seed)
    k = 3
    pairs = [(0, 1), (0, 2), (1, 2)]
    alone = per_picker - n_triples - 2 * n_pairs
    assert alone >= 0
    groups = [(0, 1, 2)] * n_triples + [S for S in pairs for _ in range(n_pairs)]
    groups += [(p,) for p in range(k) for _ in range(alone)]
    slot = rng.permutation(len(groups))
    pts = [[] for _ in range(k)]
    for g, s in zip(groups, slot):
        x0, y0 = 40.0 * (s % 100) + 5.0, 40.0 * (s // 100) + 5.0
        for p in g:
            pts[p].append((x0 + (p & 1), y0 + (p >> 1), rng.uniform(0.3, 1.0)))
    mg = []
    for p in range(k):
        a = np.array(pts[p], np.float64)[rng.permutation(len(pts[p]))]
        assert len(a) == per_picker
        mg.append((a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()))
    return mg


def deferred_tier():
    """7200 boxes; every tier-2 pseudo-micrograph has 2 x 2350 = 4700 boxes: deferred."""
    return lattice_mg(2400)


def fused_tier():
    """4800 boxes (deferred at tier 3); tier-2 pseudo-micrographs of 2 x 1550 = 3100: fused."""
    return lattice_mg(1600, seed=12)


def hand_mg():
    """``vote_util.hand_batch``'s micrograph."""
    return micrographs(vu.hand_batch())[0]


# ----------------------------------------------------------------------------- the model's cascade
def tier_solution(cols):
    """A best packing of a tier's columns (HiGHS, zero gap; ``vote_util.tier_optimum``'s model):
    [(subset, members, consensus box)] of the chosen columns."""
    flat = [(S, mem, d[mem]) for S, d in cols for mem in d]
    if not flat:
        return []
    boxes = sorted({i for _, mem, _ in flat for i in mem})
    row = {v: r for r, v in enumerate(boxes)}
    rows = [row[i] for _, mem, _ in flat for i in mem]
    cs = [j for j, (_, mem, _) in enumerate(flat) for _ in mem]
    A = coo_matrix((np.ones(len(rows), np.int64), (rows, cs)), shape=(len(boxes), len(flat)))
    x, _ = ilp_ref.milp(A, np.array([float(v[0]) for _, _, v in flat], np.float64))
    return [(S, mem, v[2]) for (S, mem, v), xi in zip(flat, x) if xi]


def cascade(b, M, t=0.3):
    """Tiers k .. M of every micrograph by the model alone -> (facts, box_tier); facts[m][tier] =
    dict(live: pickers with an unexplained box before the tier, subsets: [(subset, boxes)]
    submitted, cols: columns per submitted subset, comp: the largest conflict component,
    picks: [(subset, members)])."""
    k = b.k
    box_tier = np.zeros(len(b.x), np.int32)
    facts = []
    for m in range(b.n_mg):
        f = {}
        for tier in range(k, M - 1, -1):
            live = sum(bool((box_tier[int(b.box_off[m * k + p]):int(b.box_off[m * k + p + 1])] == 0).any())
                       for p in range(k))
            pm = vu.pseudo_micrographs(b, m, box_tier, tier)
            cols = [(S, vu.subset_columns(b, m, S, segs, t)) for S, segs in pm]
            sol = tier_solution(cols)
            vu.mark_explained(box_tier, b, m, [(b.x[c], b.y[c]) for _, _, c in sol], tier, t)
            f[tier] = dict(live=live, subsets=[(S, sum(len(s) for s in segs)) for S, segs in pm],
                           cols=[len(d) for _, d in cols], comp=vu.largest_component(cols),
                           picks=[(S, mem) for S, mem, _ in sol])
        facts.append(f)
    return facts, box_tier
