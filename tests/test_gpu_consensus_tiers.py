"""``repic consensus --min_pickers`` on the GPU (rgc_consensus_tiers, rgc_vote_gather), against
the plain-Python model of tests/vote_util.py.

Checks go tier by tier, conditional on the device's own picks of the tiers above: the model marks
what those picks explain, builds the tier's pseudo-micrographs, gets their columns from the CPU
oracle and the tier's optimum from HiGHS, so a tie in one tier's optimum cannot cascade.

* a hand case (k = 3): A by all pickers, B and C by two, D by one, a duplicate over A
* the explain / count / gather kernels alone at their shape edges (wavefront, workgroup and
  LDS-tile sizes +- 1, empty and fully explained segments, JI == T, a non-finite coordinate)
* golden inputs (10017, k = 3, M = 2) and the synthetic k = 4 inputs (M = 2 and 3)
* per-micrograph status in a mixed batch
* the command: byte prefixes, _tiers.tsv, consensus_tiers.tsv, --dedup_ji, --num_particles, on both
  routes
"""
import argparse
import os
import types

import numpy as np
import pytest

import nms_util
import vote_util as vu
from golden_util import GOLDEN, load_case, make_inputs

pytestmark = pytest.mark.gpu

T7 = 60.0 / 140.0      # JI of two 10-boxes 4 apart in x: exactly this value, on both sides


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _tiers(ctx, b, M, t=None, **kw):
    return ctx.consensus_tiers(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                               M, ji_threshold=t, **kw)


def _plain(ctx, b, t=None, **kw):
    from repic_amd import _lib
    return ctx.consensus(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                         _lib.F_HOST_OUTPUTS | _lib.F_MEMBERS | kw.pop("flags", 0),
                         ji_threshold=t, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ----------------------------------------------------------------------------- hand case
def test_hand_case(ctx):
    b = vu.hand_batch()
    r = _tiers(ctx, b, 2)
    assert r.run.status.tolist() == [0] and r.pick_off.tolist() == [0, 3]
    assert r.ptier.tolist() == [3, 2, 2]                    # A, then B (conf 0.8), then C (0.6)
    assert r.pmask.tolist() == [7, 3, 6]
    assert r.pmember.tolist() == [[0, 3, 6], [1, 4, -1], [-1, 5, 8]]
    assert r.box_tier.tolist() == [3, 2, 0, 3, 2, 2, 3, 3, 2]   # the duplicate: 3; D: 0
    assert r.tier_cols.tolist() == [[2, 2]] and r.tier_picks.tolist() == [[1, 2]]
    assert r.sel_cnt.tolist() == [3]
    # exact coordinates, weights and confidences: the model's columns for those member sets
    tier = np.zeros(9, np.int32)
    d3 = vu.tier_columns(b, 0, tier, 3, 0.3)[0][1]
    w, conf, cons = d3[(0, 3, 6)]
    assert (r.px[0], r.py[0]) == (np.rint(b.x[cons]), np.rint(b.y[cons]))
    assert _bits(r.pw[:1]) == _bits(w) and _bits(r.pconf[:1]) == _bits(conf)
    vu.mark_explained(tier, b, 0, [(b.x[cons], b.y[cons])], 3, 0.3)
    cols2 = vu.tier_columns(b, 0, tier, 2, 0.3)
    for i, (S, mem) in ((1, ((0, 1), (1, 4))), (2, ((1, 2), (5, 8)))):
        w, conf, cons = dict(cols2)[S][mem]
        assert (r.px[i], r.py[i]) == (np.rint(b.x[cons]), np.rint(b.y[cons]))
        assert _bits(r.pw[i:i + 1]) == _bits(w) and _bits(r.pconf[i:i + 1]) == _bits(conf)
    # M = k: the plain call's picks
    r3, p = _tiers(ctx, b, 3), _plain(ctx, b)
    for f in ("pick_off", "px", "py", "pcol", "sel_cnt", "ilp_status"):
        assert np.array_equal(getattr(r3, f), getattr(p, f)), f
    assert np.array_equal(_bits(r3.pconf), _bits(p.pconf))
    assert r3.ptier.tolist() == [3] and r3.pmask.tolist() == [7] and r3.pmember.tolist() == [[0, 3, 6]]
    assert r3.box_tier.tolist() == [3, 0, 0, 3, 0, 0, 3, 3, 0]
    # --num_particles cuts the whole list, tier k first
    r1 = _tiers(ctx, b, 2, num_particles=2)
    assert r1.ptier.tolist() == [3, 2] and r1.tier_picks.tolist() == [[1, 1]]
    assert r1.box_tier.tolist() == r.box_tier.tolist()      # every pick still explains


def test_hand_case_byte_counts(ctx):
    """h2d_bytes / d2h_bytes of the tiered call, counted from what it copies on the hand case
    (n_mg = 1, k = 3, 9 boxes, host inputs): the plain call's bytes, then per lower tier the
    copies listed below.  Tier 2 submits 3 pseudo-micrographs (6 segments), has 2 columns and
    2 picks; tier 3 has 1 pick."""
    from repic_amd import _lib
    b = vu.hand_batch()
    r = _tiers(ctx, b, 2)
    p = ctx.consensus(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                      _lib.F_MEMBERS)
    n_mg, k, S, N, nq, t, nps, nc, np3, np2 = 1, 3, 3, 9, 3, 2, 6, 2, 1, 2
    mgout = nq * 20 + 8 + nq * 24                          # the run's per-micrograph block
    up = ((S + 1) * 8                                       # the batch's box_off
          + nps * 4 + (nps + 1) * 8                         # segment sources, pseudo-batch offsets
          + (nq * t + 1) * 4 + nq * 8                       # the run's offsets and id bases
          + (2 * nq + 1) * 8 + 2 * nq * 4 + (n_mg + 1) * 8  # pseudo-micrograph table, column offsets
          + nc)                                             # the packing, for the emit stage
    down = (np3 * (8 + 4 * k)                               # tier 3: pw, pmask, pmember
            + S * 4 + nps * 4                               # counts; gathered counts
            + mgout + 4                                     # the run's stats; the bad-index flag
            + nc * 10 + (n_mg + 1) * 8 + n_mg * 12 + np2 * 24   # solver columns, pick stage
            + np2 * (8 + 4 * k)                             # tier 2: pw, pmask, pmember
            + N * 4)                                        # box_tier
    assert r.h2d_bytes == p.h2d_bytes + up and r.d2h_bytes == p.d2h_bytes + down
    # M = k: the plain call, the batch's offsets, the picks' extras and box_tier
    r3 = _tiers(ctx, b, 3)
    assert r3.h2d_bytes == p.h2d_bytes + (S + 1) * 8
    assert r3.d2h_bytes == p.d2h_bytes + np3 * (8 + 4 * k) + N * 4


def test_refusals_keep_the_context_usable(ctx):
    from repic_amd import _lib
    b = vu.hand_batch()
    for M in (1, 4, 0):
        with pytest.raises(_lib.RGCError, match="min_pickers"):
            _tiers(ctx, b, M)
    with pytest.raises(_lib.RGCError, match="GET_CC"):
        _tiers(ctx, b, 2, flags=_lib.F_GET_CC)
    with pytest.raises(_lib.RGCError, match="MULTI_OUT"):
        _tiers(ctx, b, 2, flags=_lib.F_MULTI_OUT)
    assert _tiers(ctx, b, 2).ptier.tolist() == [3, 2, 2]


def test_timing_sections(ctx):
    b = vu.hand_batch()
    _tiers(ctx, b, 2, timing=True)
    names = [n for n, _ in ctx.kernel_times()]
    i = names.index("k_pick_emit")                           # tier k's sections come first
    rest = names[i + 1:]
    for n in ("k_vote_explain", "k_vote_gather", "k_vote_cols", "k_pick_emit"):
        assert n in rest, (n, names)
    assert rest.index("k_vote_explain") < rest.index("k_vote_gather") < rest.index("k_vote_cols")


# ----------------------------------------------------------------------------- explain / gather
# per micrograph: unexplained boxes per picker, picks (each sits exactly on one box of its own)
GATHER_SPECS = [((0, 1, 63), 5), ((64, 65, 255), 1), ((256, 257, 3000), 255), ((1, 1, 1), 256),
                ((5, 7, 9), 257), ((2, 3, 4), 600), ((0, 0, 0), 9), ((3, 2, 2), 0)]


@pytest.fixture(scope="module")
def gather_case():
    """k = 3, box 10: boxes on a 40-pixel lattice (no two overlap), explained ones interleaved
    with the others in file order.  The last micrograph adds a box 4 off a pick (JI == T7: not
    explained), one 3 off (explained) and a box with a NaN coordinate (explained by nothing)."""
    rng = np.random.default_rng(7)
    k = 3
    xs, ys, off, pick_off, pcx, pcy = [], [], [0], [0], [], []
    slot = 0
    for mi, (u, P) in enumerate(GATHER_SPECS):
        e = [P // k + (1 if p < P % k else 0) for p in range(k)]    # explained boxes per picker
        if mi == 0:
            e = [P, 0, 0]
        mpx, mpy = [], []
        for p in range(k):
            n = u[p] + e[p]
            s = slot + np.arange(n)
            slot += n
            x, y = 40.0 * (s % 100) + 0.25, 40.0 * (s // 100) + 0.5
            hit = np.zeros(n, bool)
            hit[rng.permutation(n)[:e[p]]] = True
            if mi == len(GATHER_SPECS) - 1 and p == 0:
                # one pick at (9000, 9000): boxes at +4 (JI == T7), +3 (explained), NaN
                x = np.concatenate([x, [9004.0, 9003.0, np.nan]])
                y = np.concatenate([y, [9000.0, 9000.0, 9000.0]])
                hit = np.concatenate([hit, [False, False, False]])
                mpx.append(9000.0), mpy.append(9000.0)
            xs.append(x), ys.append(y)
            mpx.extend(x[hit]), mpy.extend(y[hit])
            off.append(off[-1] + len(x))
        pcx.extend(mpx), pcy.extend(mpy)
        pick_off.append(len(pcx))
    x, y = np.concatenate(xs), np.concatenate(ys)
    b = types.SimpleNamespace(k=k, box_size=10, n_mg=len(GATHER_SPECS),
                              box_off=np.array(off, np.int64),
                              id_base=np.zeros(len(GATHER_SPECS), np.int64), x=x, y=y,
                              score=rng.random(len(x)))
    return b, np.array(pick_off, np.int64), np.array(pcx), np.array(pcy)


def test_vote_gather_shape_edges(ctx, gather_case):
    b, pick_off, pcx, pcy = gather_case
    tier, sub_mg, sub_mask, boff, origin, gx, gy, gs = ctx.vote_gather(
        b.k, 2, b.box_size, T7, b.box_off, b.x, b.y, b.score, pick_off, pcx, pcy)
    want = np.zeros(len(b.x), np.int32)
    w_mg, w_mask, w_off, w_origin = [], [], [0], []
    for m in range(b.n_mg):
        picks = list(zip(pcx[pick_off[m]:pick_off[m + 1]], pcy[pick_off[m]:pick_off[m + 1]]))
        vu.mark_explained(want, b, m, picks, 3, T7)
        for S, segs in vu.pseudo_micrographs(b, m, want, 2):
            w_mg.append(m), w_mask.append(vu.mask_of(S))
            for seg in segs:
                w_origin.extend(seg)
                w_off.append(len(w_origin))
    assert np.array_equal(tier, want)
    # what the specs say, not only what the model says
    for m, (u, P) in enumerate(GATHER_SPECS[:-1]):
        for p in range(3):
            a, e = b.box_off[m * 3 + p], b.box_off[m * 3 + p + 1]
            assert int((want[a:e] == 0).sum()) == u[p]
    e = int(b.box_off[(b.n_mg - 1) * 3 + 1])
    assert want[e - 3:e].tolist() == [0, 3, 0]              # JI == T: not explained; NaN: never
    assert sub_mg.tolist() == w_mg and sub_mask.tolist() == w_mask
    assert 0 in w_mg and w_mask[w_mg.index(0)] == 6 and w_mg.count(0) == 1   # an empty segment
    assert 6 not in w_mg                                     # all explained: nothing submitted
    assert boff.tolist() == w_off and origin.tolist() == w_origin
    o = np.array(w_origin, np.int64)
    assert np.array_equal(_bits(gx), _bits(b.x[o])) and np.array_equal(_bits(gy), _bits(b.y[o]))
    assert np.array_equal(_bits(gs), _bits(b.score[o]))
    assert np.isnan(gx).sum() == 2                           # the NaN box, in both its subsets


def test_vote_gather_starts_from_given_tiers_and_keeps_them(ctx, gather_case):
    b, pick_off, pcx, pcy = gather_case
    start = np.zeros(len(b.x), np.int32)
    start[::7] = 5
    tier = ctx.vote_gather(b.k, 3, b.box_size, T7, b.box_off, b.x, b.y, b.score, pick_off, pcx,
                           pcy, pick_tier=4, box_tier=start)[0]
    want = start.copy()
    for m in range(b.n_mg):
        picks = list(zip(pcx[pick_off[m]:pick_off[m + 1]], pcy[pick_off[m]:pick_off[m + 1]]))
        vu.mark_explained(want, b, m, picks, 4, T7)
    assert np.array_equal(tier, want) and (tier[::7] == 5).all()


# ----------------------------------------------------------------------------- goldens
def _check_tiers(ctx, b, M, t, flags=0):
    """Every tier of every micrograph against the model, given the device's picks above it."""
    from repic_amd import _lib
    from repic_amd.ilp import OPTIMAL
    k = b.k
    T = 0.3 if t is None else t
    r = _tiers(ctx, b, M, t, flags=flags)
    p = _plain(ctx, b, t, flags=flags)
    want_tier = np.zeros(len(b.x), np.int32)
    n_lower = 0
    for m in range(b.n_mg):
        p0, p1 = int(r.pick_off[m]), int(r.pick_off[m + 1])
        tiers = r.ptier[p0:p1]
        assert (np.diff(tiers) <= 0).all()                  # tier descending
        # tier k: the plain call's arrays, bit for bit
        q0, q1 = int(p.pick_off[m]), int(p.pick_off[m + 1])
        nk = q1 - q0
        assert (tiers[:nk] == k).all() and (tiers[nk:] < k).all()
        for f in ("px", "py", "pcol"):
            assert np.array_equal(getattr(r, f)[p0:p0 + nk], getattr(p, f)[q0:q1]), f
        assert np.array_equal(_bits(r.pconf[p0:p0 + nk]), _bits(p.pconf[q0:q1]))
        ok_k = p.run.status[m] == _lib.OK
        cl = int(p.run.clique_base[m]) + p.pcol[q0:q1] if ok_k else np.zeros(0, np.int64)
        assert np.array_equal(r.pmember[p0:p0 + nk], p.run.members[cl])
        assert np.array_equal(_bits(r.pw[p0:p0 + nk]), _bits(p.run.w[cl]))
        assert (r.pmask[p0:p0 + nk] == (1 << k) - 1).all()
        assert r.tier_cols[m, 0] == (p.run.clique_cnt[m] if ok_k else 0)
        used = set(r.pmember[p0:p0 + nk].reshape(-1).tolist())
        assert len(used) == nk * k
        cons = p.run.consensus[cl]
        vu.mark_explained(want_tier, b, m, list(zip(b.x[cons], b.y[cons])), k, T)
        st_ok = ok_k
        for tier in range(k - 1, M - 1, -1):
            idx = p0 + np.flatnonzero(tiers == tier)
            cols = vu.tier_columns(b, m, want_tier, tier, T)
            by_mask = {vu.mask_of(S): d for S, d in cols}
            assert r.tier_cols[m, k - tier] == sum(len(d) for d in by_mask.values())
            st_ok = st_ok or r.tier_cols[m, k - tier] > 0
            assert r.tier_picks[m, k - tier] == len(idx)
            assert (np.diff(r.pconf[idx]) <= 0).all()       # run_ilp's order
            picks = []
            for i in idx:
                mem = tuple(v for v in r.pmember[i].tolist() if v >= 0)
                mask = int(r.pmask[i])
                assert [v >= 0 for v in r.pmember[i].tolist()] == [bool((mask >> q) & 1) for q in range(k)]
                assert len(mem) == tier and not used & set(mem)      # one per picker, disjoint
                used |= set(mem)
                assert all(want_tier[v] == 0 for v in mem)           # unexplained before the tier
                for u in range(tier):
                    for v in range(u + 1, tier):
                        assert vu.explains(b.x[mem[u]], b.y[mem[u]], b.x[mem[v]], b.y[mem[v]],
                                           b.box_size, T)
                w, conf, cons = by_mask[mask][mem]
                assert _bits(r.pw[i:i + 1]) == _bits(w) and _bits(r.pconf[i:i + 1]) == _bits(conf)
                assert (r.px[i], r.py[i]) == (np.rint(b.x[cons]), np.rint(b.y[cons]))
                picks.append((b.x[cons], b.y[cons]))
            # the packing's value against HiGHS' optimum (tests/test_ilp.py's criterion)
            obj = float(r.pw[idx].astype(np.float64).sum())
            objr = vu.tier_optimum(cols)
            assert abs(obj - objr) <= 1e-12 * max(1.0, objr), (m, tier, obj, objr)
            assert vu.largest_component(cols) <= _lib.ilp_big_max()
            vu.mark_explained(want_tier, b, m, picks, tier, T)
            n_lower += len(idx)
        assert (r.run.status[m] == _lib.OK) == bool(st_ok)
        if st_ok:
            assert r.ilp_status[m] == OPTIMAL               # every component is searched exactly
        assert r.sel_cnt[m] == p1 - p0
    assert np.array_equal(r.box_tier, want_tier)
    return r, n_lower


def _pack(k, box, mgs):
    from repic_amd.pipeline import Batch
    return Batch.pack(k, box, mgs)


def test_golden_10017_two_of_three(ctx):
    methods, bases, mgs = vu.load_dir(os.path.join(GOLDEN, "inputs_10017"), 2)
    assert len(methods) == 3 and len(bases) == 2
    r, n_lower = _check_tiers(ctx, _pack(3, 180, mgs), 2, None)
    assert n_lower > 0 and (r.tier_picks[:, 1] > 0).all()


def test_golden_10017_multi_kernel_route(ctx):
    """The same checks with every run on the multi-kernel route.  (The two routes order their
    cliques differently, so where an optimum is not unique they may pick differently: each is
    checked against the model given its own picks, not against the other.)"""
    from repic_amd import _lib
    methods, bases, mgs = vu.load_dir(os.path.join(GOLDEN, "inputs_10017"), 3)
    r, n_lower = _check_tiers(ctx, _pack(3, 180, mgs[2:]), 2, None, flags=_lib.F_NO_FUSED)
    assert n_lower > 0


@pytest.mark.parametrize("M", [2, 3])
def test_synthetic_k4(ctx, M):
    from cases import CASES
    from repic_amd import synth
    from repic_amd.ingest import sigmoid
    case = CASES["syn_k4"]
    cfg = synth.SynthConfig(**case["synth"])
    mgs = [[(x, y, sigmoid(s) if s.min() < 0 else s) for (x, y, s) in mg]
           for mg in synth.batch(cfg, 2)]
    r, n_lower = _check_tiers(ctx, _pack(4, case["box"], mgs), M, None)
    assert n_lower > 0 and r.tier_cols.shape == (2, 4 - M + 1)


def test_other_threshold(ctx):
    methods, bases, mgs = vu.load_dir(os.path.join(GOLDEN, "inputs_10017"), 1)
    _check_tiers(ctx, _pack(3, 180, mgs), 2, 0.45)


# ----------------------------------------------------------------------------- status
def test_status_in_a_mixed_batch(ctx):
    from repic_amd import _lib
    f = lambda *v: np.array(v, np.float64)  # noqa: E731
    s = f(0.5)
    full = [(f(100), f(100), s), (f(101), f(100), s), (f(100), f(101), s)]
    pairs = [(f(100), f(100), s), (f(101), f(100), s), (f(500), f(500), s)]     # no 3-clique
    apart = [(f(100), f(100), s), (f(300), f(300), s), (f(500), f(500), s)]     # no edge
    b = _pack(3, 10, [full, pairs, apart, full])
    r = _tiers(ctx, b, 2)
    assert r.run.status.tolist() == [_lib.OK, _lib.OK, _lib.NO_EDGES, _lib.OK]
    assert np.diff(r.pick_off).tolist() == [1, 1, 0, 1]
    assert r.ptier.tolist() == [3, 2, 3] and r.pmask.tolist() == [7, 3, 7]
    assert r.tier_cols.tolist() == [[1, 0], [0, 1], [0, 0], [1, 0]]
    r3 = _tiers(ctx, b, 3)
    assert r3.run.status.tolist() == [_lib.OK, _lib.NO_CLIQUES, _lib.NO_EDGES, _lib.OK]
    assert np.diff(r3.pick_off).tolist() == [1, 0, 0, 1]
    assert _plain(ctx, b).run.status.tolist() == r3.run.status.tolist()


# ----------------------------------------------------------------------------- the command
def _run_cli(in_dir, out_dir, meta, **kw):
    from repic_amd.commands import consensus
    a = argparse.Namespace(in_dir=in_dir, out_dir=out_dir, box_size=meta["box"], multi_out=False,
                           get_cc=False, batch_boxes=1 << 25, threads=None, device=None,
                           listing=meta["listing"], num_particles=None, node_limit=0)
    for k_, v in kw.items():
        setattr(a, k_, v)
    consensus.main(a)
    out = {}
    for f in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, f), "rb") as fh:
            out[f] = fh.read()
    return out


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    """The golden directory through the command, once per option set."""
    root = tmp_path_factory.mktemp("tiers_cli")
    meta, _ = load_case("c1_10017")
    in_dir = make_inputs("c1_10017", str(root))
    runs = {}

    def get(name, **kw):
        if name not in runs:
            runs[name] = _run_cli(in_dir, str(root / name), meta, **kw)
        return runs[name]
    return get


def _box_files(out):
    return {f: v for f, v in out.items() if f.endswith(".box")}


def test_cli_min_pickers_k_is_the_plain_output(cli):
    from repic_amd.commands import consensus
    plain, m3 = cli("plainfused"), cli("m3", min_pickers=3)
    assert _box_files(m3) == _box_files(plain) and len(_box_files(plain)) == 12
    assert m3[consensus.SUMMARY] == plain[consensus.SUMMARY]
    assert set(m3) - set(plain) == {consensus.TIERS} | {f[:-4] + consensus.TIERS_SUFFIX
                                                        for f in _box_files(plain)}
    for f, v in _box_files(plain).items():
        lines = m3[f[:-4] + consensus.TIERS_SUFFIX].decode().splitlines()
        assert lines == ["3\tcrYOLO,deepPicker,topaz"] * v.count(b"\n")


@pytest.mark.parametrize("route", ["fused", "multi"])
def test_cli_min_pickers_2(cli, route):
    from repic_amd.commands import consensus
    nf = {"no_fused": True} if route == "multi" else {}
    plain, m2 = cli("plain" + route, **nf), cli("m2" + route, min_pickers=2, **nf)
    rows = [ln.split("\t") for ln in m2[consensus.TIERS].decode().splitlines()]
    assert "\t".join(rows[0]) + "\n" == consensus.tiers_header(3, 2)
    tab = {r[0]: [int(v) for v in r[1:]] for r in rows[1:]}
    summ = {r.split("\t")[0]: r.split("\t") for r in m2[consensus.SUMMARY].decode().splitlines()[1:]}
    names = {"crYOLO,deepPicker,topaz", "crYOLO,deepPicker", "crYOLO,topaz", "deepPicker,topaz"}
    more = 0
    for f, v in _box_files(plain).items():
        base = f[:-4]
        assert m2[f].startswith(v)                          # lines 1..n_k: the plain file
        lines = m2[base + consensus.TIERS_SUFFIX].decode().splitlines()
        n = m2[f].count(b"\n")
        assert len(lines) == n
        tiers = [int(ln.split("\t")[0]) for ln in lines]
        assert tiers == sorted(tiers, reverse=True) and tiers.count(3) == v.count(b"\n")
        assert all(ln.split("\t")[1] in names and
                   ln.split("\t")[1].count(",") == int(ln.split("\t")[0]) - 1 for ln in lines)
        c3, p3, c2, p2 = tab[base]
        assert (p3, p2) == (tiers.count(3), tiers.count(2)) and p3 + p2 == n
        assert summ[base][1] == "ok" and int(summ[base][2]) == c3 + c2 and int(summ[base][3]) == n
        more += p2
    assert more > 0


def test_cli_num_particles_keeps_the_first_lines(cli):
    m2, m2n = cli("m2fused", min_pickers=2), cli("m2n", min_pickers=2, num_particles=5)
    from repic_amd.commands import consensus
    for f, v in _box_files(m2).items():
        assert m2n[f] == b"".join(v.splitlines(keepends=True)[:5])
        t = f[:-4] + consensus.TIERS_SUFFIX
        assert m2n[t] == b"".join(m2[t].splitlines(keepends=True)[:5])


def test_cli_dedup_composes(cli):
    from repic_amd.commands import consensus
    m2, dd = cli("m2fused", min_pickers=2), cli("m2d", min_pickers=2, dedup_ji=0.3)
    dropped = 0
    for f, v in _box_files(m2).items():
        t = f[:-4] + consensus.TIERS_SUFFIX
        src = list(zip(v.splitlines(), m2[t].splitlines()))
        out = list(zip(dd[f].splitlines(), dd[t].splitlines()))
        assert len(dd[f].splitlines()) == len(dd[t].splitlines())
        # the written (line, tier line) pairs are a subsequence of the unsuppressed run's
        it = iter(src)
        assert all(any(o == s for s in it) for o in out)
        x, y, _ = nms_util.box_xys([ln.decode() for ln in dd[f].splitlines()])
        assert nms_util.nms_oracle(x, y, 180, 0.3).all()    # no two written lines have JI > 0.3
        xs, ys, _ = nms_util.box_xys([ln.decode() for ln in v.splitlines()])
        keep = nms_util.nms_oracle(xs, ys, 180, 0.3)
        assert [s for s, kp in zip(src, keep) if kp] == out  # a higher tier always wins
        dropped += len(src) - len(out)
    assert dropped > 0
