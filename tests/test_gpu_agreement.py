"""Picker agreement on the device (rgc_agreement, ``repic agreement``) against the numpy oracle of
tests/agree_util.py: every array exactly, ``partner_ji`` by bits.  The shapes are the smallest at
which the kernels can go wrong: empty and one-box segments, sizes around the 64-lane wave and the
256-thread workgroup against partners of other sizes, every picker count with its own unrolled
slot, coordinates at which the window's margin matters, and one dense pair with long windows."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import agree_util as au
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _check(ctx, k, mgs, box, t=0.3, partners=True):
    """One device call on micrographs given as k (x, y) pairs each, against the oracle."""
    n_mg, off, x, y = au.pack(k, mgs)
    got = ctx.agreement(n_mg, k, box, off, x, y, ji_threshold=t, partners=partners)
    want = au.oracle(n_mg, k, box, off, x, y, t)
    au.assert_same(got, want, partners)
    return got


def _rand_mg(rng, sizes, field, frac=False):
    out = []
    for n in sizes:
        xy = rng.uniform(0, field, (2, n)) if frac else rng.integers(0, field, (2, n)).astype(float)
        out.append((xy[0], xy[1]))
    return out


# ----------------------------------------------------------------------------- empty, degenerate
def test_no_micrographs_and_empty_segments(ctx):
    r = ctx.agreement(0, 3, 10, [0], [], [], partners=True)
    assert r.support.shape == (0,) and r.partner.shape == (0, 3) and r.partner_ji.shape == (0, 3)
    assert r.pair_edges.shape == r.pair_supported.shape == r.pair_mutual.shape == (0, 3, 3)
    assert ctx.agreement_bytes == (0, 0)
    e = ([], [])
    r = _check(ctx, 2, [[e, e], [e, e]], 10)
    assert r.support.shape == (0,) and not r.pair_edges.any() and ctx.agreement_bytes == (0, 0)
    # empty segments between full ones, and micrographs where one side is empty
    a, b = ([0, 50, 1], [0, 50, 0]), ([1, 51], [0, 50])
    r = _check(ctx, 3, [[e, e, e], [a, e, b], [e, a, e], [b, a, e], [e, e, e], [a, b, a]], 10)
    assert r.pair_edges[1].tolist() == [[0, 0, 3], [0, 0, 0], [3, 0, 0]]
    assert not r.pair_edges[2].any() and not r.pair_edges[0].any()


def test_k1_and_one_box_per_segment(ctx):
    r = _check(ctx, 1, [[([0, 1, 2], [0, 0, 0])], [([], [])], [([5], [5])]], 10)
    assert r.support.tolist() == [0, 0, 0, 0] and r.partner.tolist() == [[-1]] * 4
    assert not r.pair_edges.any() and r.pair_edges.shape == (3, 1, 1)
    r = _check(ctx, 3, [[([0], [0]), ([1], [0]), ([0], [1])], [([0], [0]), ([20], [0]), ([0], [9])]],
               10, 0.0)
    assert r.support.tolist() == [6, 5, 3, 4, 0, 1]
    assert r.pair_mutual[1].tolist() == [[0, 0, 1], [0, 0, 0], [1, 0, 0]]


# ----------------------------------------------------------------------------- the edge rule
def test_hand_cases_both_orders(ctx):
    # overlap 5 x 10 = 50 at box 10: JI == 1/3 in f64: not joined at T = 1/3, joined at 0.3
    for xa, xb in ((0, 5), (5, 0)):
        r = _check(ctx, 2, [[([xa], [0]), ([xb], [0])]], 10, 1 / 3)
        assert r.support.tolist() == [0, 0] and r.partner.tolist() == [[-1, -1], [-1, -1]]
        r = _check(ctx, 2, [[([xa], [0]), ([xb], [0])]], 10, 0.3)
        assert r.support.tolist() == [2, 1] and r.partner_ji[0, 1] == r.partner_ji[1, 0] == 1 / 3
        # |dx| == B: never joined
        for t in (0.0, 0.3):
            r = _check(ctx, 2, [[([xa * 2], [0]), ([xb * 2], [0])]], 10, t)
            assert not r.pair_edges.any()
    # identical boxes, up to the largest threshold below 1 and the largest box size
    r = _check(ctx, 2, [[([3.5], [7.25]), ([3.5], [7.25])]], 10, np.nextafter(1.0, 0.0))
    assert r.pair_edges[0].tolist() == [[0, 1], [1, 0]]     # JI == 1.0 is above it
    r = _check(ctx, 2, [[([3.5], [7.25]), ([3.5], [7.25])]], 2 ** 26, 0.999)
    assert r.partner_ji[0, 1] == 1.0 and r.pair_mutual[0].tolist() == [[0, 1], [1, 0]]
    # partner ties go to the lowest batch index, whatever the x order; mutual with ties
    r = _check(ctx, 2, [[([0], [0]), ([2, -2, 2], [0, 0, 0])]], 10)
    assert r.partner[:, 1].tolist() == [1, -1, -1, -1] and r.partner[:, 0].tolist() == [-1, 0, 0, 0]
    assert r.pair_mutual[0].tolist() == [[0, 1], [1, 0]]
    r = _check(ctx, 2, [[([2, -2, 2], [0, 0, 0]), ([0], [0])]], 10)
    assert r.partner[3].tolist() == [0, -1] and r.pair_supported[0].tolist() == [[0, 3], [1, 0]]
    r = _check(ctx, 2, [[([0, 0], [0, 0]), ([1, 1], [0, 0])]], 10)
    assert r.pair_mutual[0].tolist() == [[0, 1], [1, 0]] and r.pair_edges[0, 0, 1] == 4


def test_every_integer_offset(ctx):
    offs = [(dx, dy) for dx in range(-10, 11) for dy in range(-10, 11)]
    mgs = [[([0], [0]), ([dx], [dy])] for dx, dy in offs] + \
          [[([dx], [dy]), ([0], [0])] for dx, dy in offs]
    for t in (0.3, 0.0, 1 / 3):
        r = _check(ctx, 2, mgs, 10, t)
        area = np.array([(10 - abs(dx)) * (10 - abs(dy)) for dx, dy in offs] * 2)
        want = area / (200.0 - area) > t
        assert np.array_equal(r.pair_edges[:, 0, 1] == 1, want)


def test_non_finite_boxes(ctx):
    nan, inf = float("nan"), float("inf")
    xa = [0, nan, inf, -inf, 0, 0, 0, 1]
    ya = [0, 0, 0, 0, nan, inf, -inf, 0]
    r = _check(ctx, 2, [[(xa, ya), (xa, ya)]], 10, 0.0)
    assert r.support.tolist() == [2, 0, 0, 0, 0, 0, 0, 2] + [1, 0, 0, 0, 0, 0, 0, 1]
    # a segment with no finite box at all next to a full one
    r = _check(ctx, 2, [[([nan, inf], [0, 0]), ([0, 1], [0, 0])], [([0], [0]), ([1], [0])]], 10)
    assert not r.pair_edges[0].any() and r.pair_edges[1, 0, 1] == 1
    # non-finite boxes mixed into random segments
    rng = np.random.default_rng(11)
    mg = _rand_mg(rng, [300, 200, 257], 300)
    for x, y in mg:
        x[rng.integers(0, len(x), 20)] = rng.choice([nan, inf, -inf], 20)
        y[rng.integers(0, len(y), 20)] = rng.choice([nan, inf, -inf], 20)
    r = _check(ctx, 3, [mg], 40)
    assert r.pair_edges.sum() > 0


# ----------------------------------------------------------------------------- sizes, picker counts
def test_sizes_around_the_wave_and_the_workgroup(ctx):
    sizes = [1, 63, 64, 65, 255, 256, 257, 1000]
    rng = np.random.default_rng(3)
    mgs = [_rand_mg(rng, [sizes[i], sizes[(i + 3) % 8], sizes[(i + 5) % 8]], 400)
           for i in range(8)]
    r = _check(ctx, 3, mgs, 40)
    assert (r.pair_edges.sum(axis=(1, 2)) > 0).all() and (r.pair_mutual.sum(axis=(1, 2)) > 0).all()


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_picker_counts_on_synthetic_micrographs(ctx, k):
    from repic_amd import synth
    cfg = synth.SynthConfig(k=k, n_true=60, box=180, width=2048, height=2048, dup=0.1, seed=20 + k)
    mgs = [[(x, y) for x, y, _ in mg] for mg in synth.batch(cfg, 4)]
    r = _check(ctx, k, mgs, cfg.box)
    assert r.pair_mutual.sum() > 0 and int(r.support.max()) >= (1 << (k - 1))
    for t in (0.0, 0.6):
        _check(ctx, k, mgs, cfg.box, t)


def test_fractional_and_large_coordinates(ctx):
    rng = np.random.default_rng(5)
    _check(ctx, 3, [_rand_mg(rng, [300, 257, 100], 500, frac=True) for _ in range(2)], 50)
    # near 2^40 one ulp is 2^-12: boxes whose x distance is B less or more a few ulps, where
    # fl(min + B) - max is tiny or zero and only the window's margin keeps them in reach
    x0, B, u = 2.0 ** 40, 180.0, 2.0 ** -12
    xs = [x0 + B - j * u for j in range(5)] + [x0 - B + j * u for j in range(5)] + \
         [x0 + B + u, x0 - B - u, x0 + 1.5, x0 - 90.25]
    for t in (0.0, 0.3):
        r = _check(ctx, 2, [[([x0], [x0]), (xs, [x0] * len(xs))],
                            [(xs, [x0] * len(xs)), ([x0], [x0])]], 180, t)
        assert r.pair_edges[0, 0, 1] == r.pair_edges[1, 0, 1] == (10 if t == 0.0 else 2)
    big = _rand_mg(rng, [200, 200], 600, frac=True)
    _check(ctx, 2, [[(x + x0, y - x0) for x, y in big]], 60)


def test_one_dense_pair(ctx):
    """2 pickers x 5000 boxes on a 1024^2 field, box 64: windows of ~600 boxes and 20 trips of the
    workgroup."""
    rng = np.random.default_rng(9)
    r = _check(ctx, 2, [_rand_mg(rng, [5000, 5000], 1024)], 64)
    assert r.pair_edges[0, 0, 1] > 20000


# ----------------------------------------------------------------------------- the existing pipeline
def test_edges_of_the_consensus_graph(ctx):
    """On one batch, ``Context.run(..., F_EDGES)`` gives exactly the joined pairs: the per-pair
    counts, the per-box masks, and no edge above its ends' partner JI."""
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch
    k = 3
    cfg = synth.SynthConfig(k=k, n_true=60, box=180, width=2048, height=2048, dup=0.1, seed=7)
    b = Batch.pack(k, cfg.box, synth.batch(cfg, 6))
    ag = ctx.agreement(b.n_mg, k, cfg.box, b.box_off, b.x, b.y, partners=True)
    ctx.run(b.n_mg, k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score,
            _lib.F_HOST_OUTPUTS | _lib.F_EDGES)
    u, v, ji = ctx.last_edges()
    assert len(u) > 0 and len(set(zip(u.tolist(), v.tolist()))) == len(u)
    seg = np.searchsorted(b.box_off, np.arange(b.n_boxes), "right") - 1
    su, sv = seg[u], seg[v]
    assert np.array_equal(su // k, sv // k) and (su % k < sv % k).all()
    cnt = np.zeros((b.n_mg, k, k), np.int64)
    np.add.at(cnt, (su // k, su % k, sv % k), 1)
    np.add.at(cnt, (su // k, sv % k, su % k), 1)
    assert np.array_equal(cnt, ag.pair_edges)
    mask = np.zeros(b.n_boxes, np.uint8)
    np.bitwise_or.at(mask, u, (1 << (sv % k)).astype(np.uint8))
    np.bitwise_or.at(mask, v, (1 << (su % k)).astype(np.uint8))
    assert np.array_equal(mask, ag.support)
    assert (ji <= ag.partner_ji[u, sv % k]).all() and (ji <= ag.partner_ji[v, su % k]).all()
    # ... and each partner is one of those edges, with that JI
    e = {(a, c): j for a, c, j in zip(u.tolist(), v.tolist(), ji.view(np.uint64).tolist())}
    bb, qq = np.nonzero(ag.partner >= 0)
    for a, q in zip(bb.tolist(), qq.tolist()):
        c = int(ag.partner[a, q])
        assert e[(min(a, c), max(a, c))] == ag.partner_ji[a, q].view(np.uint64)


# ----------------------------------------------------------------------------- further checks
def test_two_calls_identical_and_partners_stay_on_the_device(ctx):
    rng = np.random.default_rng(13)
    k, mgs = 3, [_rand_mg(rng, [300, 200, 257], 300) for _ in range(3)]
    n_mg, off, x, y = au.pack(k, mgs)
    a = ctx.agreement(n_mg, k, 40, off, x, y, partners=True, timing=True)
    names = [n for n, _ in ctx.kernel_times()]
    assert names == ["k_agree_partner", "k_agree_mutual"]
    h2d, d2h = ctx.agreement_bytes
    n = int(off[-1])
    assert d2h == n + 24 * k * k * n_mg + 12 * k * n
    b = ctx.agreement(n_mg, k, 40, off, x, y, partners=True)
    for f in au.FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    c = ctx.agreement(n_mg, k, 40, off, x, y)
    assert c.partner is None and c.partner_ji is None
    assert ctx.agreement_bytes == (h2d, n + 24 * k * k * n_mg)
    au.assert_same(c, a, partners=False)


def _raw(c, n_mg, k, off, x, y, box, t, null=()):
    """rgc_agreement through ctypes, nothing checked on the way"""
    from repic_amd import _lib
    off = np.asarray(off, np.int64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ptr = {"off": off.ctypes.data, "x": x.ctypes.data, "y": y.ctypes.data}
    for f in null:
        ptr[f] = None
    ai = _lib.AgreeIn(n_mg, k, box, t, 0, ptr["off"], ptr["x"], ptr["y"])
    ao = _lib.AgreeOut()
    _lib._check(_lib.lib.rgc_agreement(c._p, C.byref(ai), C.byref(ao)))
    return ao


def test_refusals_leave_the_context_usable():
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch
    c = _lib.Context(0)
    good = [[([0, 50], [0, 50]), ([1, 51, 90], [0, 50, 90])]]

    def valid():
        r = _check(c, 2, good, 10)
        assert r.pair_edges[0].tolist() == [[0, 2], [2, 0]]
    try:
        valid()
        x = y = np.zeros(4)
        bad = [
            ("n_mg", (-1, 2, [0, 0, 0], x, y, 10, 0.3)),
            ("n_mg", (2 ** 28, 8, [0], x, y, 10, 0.3)),
            ("k must be", (1, 0, [0], x, y, 10, 0.3)),
            ("k must be", (1, 9, [0] * 10, x, y, 10, 0.3)),
            ("start at 0", (1, 2, [1, 2, 3], x, y, 10, 0.3)),
            ("non-decreasing", (1, 2, [0, 3, 2], x, y, 10, 0.3)),
            ("2\\^31 - 1 boxes", (1, 2, [0, 3, 2 ** 31], x, y, 10, 0.3)),
            ("box_size", (1, 2, [0, 2, 4], x, y, 0, 0.3)),
            ("box_size", (1, 2, [0, 2, 4], x, y, 2 ** 26 + 1, 0.3)),
            ("ji_threshold", (1, 2, [0, 2, 4], x, y, 10, 1.0)),
            ("ji_threshold", (1, 2, [0, 2, 4], x, y, 10, -0.1)),
            ("ji_threshold", (1, 2, [0, 2, 4], x, y, 10, float("nan"))),
        ]
        for match, a in bad:
            with pytest.raises(_lib.RGCError, match=match):
                _raw(c, *a)
            valid()
        for null in (("off",), ("x",), ("y",)):
            with pytest.raises(_lib.RGCError, match="null argument"):
                _raw(c, 1, 2, [0, 2, 4], x, y, 10, 0.3, null=null)
        valid()
        assert _lib.lib.rgc_agreement(c._p, None, None) < 0
        # null coordinates with no box to read are fine
        _raw(c, 1, 2, [0, 0, 0], x, y, 10, 0.3, null=("x", "y"))
        # a submitted run that awaits rgc_wait
        cfg = synth.SynthConfig(k=3, n_true=20, box=180, width=1024, height=1024, seed=5)
        b = Batch.pack(cfg.k, cfg.box, synth.batch(cfg, 2))
        c.submit(b.n_mg, cfg.k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score)
        with pytest.raises(_lib.RGCError, match="awaits rgc_wait"):
            _raw(c, 1, 2, [0, 2, 4], x, y, 10, 0.3)
        c.wait()
        valid()
    finally:
        c.close()


# ----------------------------------------------------------------------------- repic agreement
def test_cli_on_real_picker_files(tmp_path, monkeypatch):
    """The dispatcher's ``agreement`` on the committed picker files with --per_box, against the
    same command driven by the oracle: every file byte for byte."""
    from repic_amd import agreement as ag, main as repic_main
    from repic_amd.commands import agreement as ag_cmd
    in_dir = os.path.join(GOLDEN, "inputs_10017")
    dev, ora = str(tmp_path / "dev"), str(tmp_path / "ora")
    repic_main.main(["agreement", in_dir, dev, "180", "--per_box"])
    assert ag_cmd.LAST_RUN["micrographs"] == 12 and ag_cmd.LAST_RUN["d2h_bytes"] > 0
    monkeypatch.setattr(ag, "device_call", au.oracle_device_call)
    ag_cmd.main(argparse.Namespace(in_dir=in_dir, out_dir=ora, box_size=180, ji_threshold=0.3,
                                   per_box=True, batch_boxes=1 << 25, threads=None, device=None,
                                   listing=None))
    names = sorted(os.listdir(ora))
    assert sorted(os.listdir(dev)) == names and len(names) == 4 + 12
    for f in names:
        with open(os.path.join(dev, f), "rb") as a, open(os.path.join(ora, f), "rb") as b:
            assert a.read() == b.read(), f
    with open(os.path.join(dev, ag_cmd.MATRIX)) as f:
        rows = [ln.split("\t") for ln in f.read().splitlines()[1:]]
    assert rows[0] == ["crYOLO", "deepPicker", "8908", "3160", "3477", "2588"]
    assert rows[1] == ["crYOLO", "topaz", "8908", "8777", "10006", "7885"]
