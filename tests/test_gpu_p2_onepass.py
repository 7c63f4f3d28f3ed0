"""P2 in one pass (rgc_fused.hip): a wave-round counts the edges of one aligned block of 64
sorted positions, reserves the block's lists with one atomic on the workgroup's edge cursor and
writes them at once; fwd holds each box's list begin, bend each block's end.

The cases are the smallest micrographs at which that code can go wrong: box counts around the
64-position blocks, partly filled reversed (odd) rounds, forward degrees 0..9 side by side in one
wave, a box with an edge past its 32nd stencil candidate, both coordinate layouts, --get_cc,
the three edge-capacity regimes of a size class, and repeated runs.  Every micrograph is
compared bit for bit with the oracle (edge set with JI bits through RGC_F_EDGES, rows, w, conf,
consensus, cc_max / cc_cnt: the helpers of test_gpu_p2_flat.py / test_gpu_parity.py) and the
fused route with the multi-kernel route (F_NO_FUSED).

Positions are picker-major, so the boxes of the last picker that has boxes never hold a
forward list: "the last box having edges" is the last box being an edge's target while the
last position of a block holds a list (test_list_at_block_end).

Workgroup sizes (K = 3, integer layout): the host's plan picks the 256-thread instance where
LDS admits eight workgroups per CU (classes up to 512 boxes: most cases here), 512 threads
for the larger classes with three or more workgroups per CU and 768 threads for the classes
with two (1409..1536 boxes), so each of the three has its partly filled reversed round.
"""
import numpy as np
import pytest

from test_gpu_p2_flat import BOX, LAYOUTS, _check, _mask_case, _mg, _random_mg
from test_gpu_parity import _check_vs_oracle

pytestmark = pytest.mark.gpu


def _fields(r):
    return (r.status, r.cc_max, r.cc_cnt, r.n_vert, r.n_edges)


def _routes_equal(mgs, k, box, get_cc=False):
    """The fused route against the multi-kernel route, array by array (cliques in the
    canonical order of their rows: the two routes number a micrograph's cliques alike, but
    nothing here relies on it)."""
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    batch = Batch.pack(k, box, mgs)
    ctx = _lib.Context(0)
    a = run_batch(ctx, batch, get_cc=get_cc)
    b = run_batch(ctx, batch, get_cc=get_cc, no_fused=True)
    ctx.close()
    for ra, rb in zip(a, b):
        assert _fields(ra) == _fields(rb)
        if ra.status != _lib.OK:
            continue
        pa, pb = np.lexsort(ra.rows.T[::-1]), np.lexsort(rb.rows.T[::-1])
        assert np.array_equal(ra.rows[pa], rb.rows[pb])
        assert np.array_equal(ra.w[pa].view(np.uint32), rb.w[pb].view(np.uint32))
        assert np.array_equal(ra.conf[pa].view(np.uint32), rb.conf[pb].view(np.uint32))
        assert np.array_equal(ra.consensus[pa], rb.consensus[pb])
    return a


def _both(mg, box=BOX):
    """One micrograph: oracle (edges and outputs) and the other route.  Returns the edges."""
    edges = _check(mg, box)
    _routes_equal([mg], len(mg), box)
    return edges


def _line(sets, shift, seed=3):
    """Particles on a line, 300 px apart (no edges between particles), all in one grid row, so
    a picker's sorted positions follow the particle index; picker p has a box at the particles
    `sets[p]` (a few px off the centre: every pair of one particle is an edge)."""
    rng = np.random.default_rng(seed)
    return _mg([[(300 * i + int(rng.integers(-4, 5)), 10 + int(rng.integers(-4, 5))) for i in s]
                for s in sets], shift, seed)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129])
def test_block_edges(n, shift):
    """n boxes in all over three pickers: the last block holds 1, 63 or 64 boxes."""
    per = [(n + 2 - p) // 3 for p in range(3)]
    assert sum(per) == n
    edges = _both(_line([range(c) for c in per], shift))
    # particle i: (p0, p1), (p0, p2), (p1, p2) where the pickers have a box for it
    assert len(edges) == sum((per[0] > i) * ((per[1] > i) + (per[2] > i)) + (per[1] > i) * (per[2] > i)
                             for i in range(per[0]))


@pytest.mark.parametrize("shift", LAYOUTS)
def test_lists_across_a_block_boundary(shift):
    """3 x 40 boxes: positions 63 and 64 are picker-1 boxes 23 and 24, each with one edge; the
    lists of positions 0..63 and 64..119 are reserved by different waves."""
    assert len(_both(_line([range(40)] * 3, shift))) == 120


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("n0", [64, 128])
def test_list_at_block_end(n0, shift):
    """K = 2: picker 0 fills positions 0..n0-1, picker 1 has boxes at the first and the last
    particle: the last position of the last full block holds a list whose target is the very
    last box; every other box of that block holds none."""
    edges = _both(_line([range(n0), [0, n0 - 1]], shift))
    assert sorted((u, v) for (u, v, _) in edges) == [(0, n0), (n0 - 1, n0 + 1)]


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("extra", [1, 63, 65])
def test_reversed_round_512(extra, shift):
    """512 + 1 / 63 / 65 boxes: the second round of a 512-thread workgroup walks backwards with
    one lane, one partly filled block, and a full block plus one lane."""
    n = 512 + extra
    per = [(n + 2 - p) // 3 for p in range(3)]
    assert _both(_random_mg(3, per, shift, seed=5, size=3000))


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("extra", [1, 63, 65])
def test_reversed_round_256(extra, shift):
    """256 + 1 / 63 / 65 boxes (classes 320 and 384: the 256-thread instance)."""
    n = 256 + extra
    per = [(n + 2 - p) // 3 for p in range(3)]
    assert _both(_random_mg(3, per, shift, seed=4, size=2200))


def test_reversed_round_768():
    """1500 boxes (class 1536: two workgroups of 768 threads per CU): the second round holds
    732 boxes, walked backwards."""
    assert _both(_random_mg(3, 500, 0.0, seed=6, size=3000))


DEGREES = [0, 1, 2, 3, 4, 9]


def _degree_case(k, shift):
    """Six picker-0 boxes next to each other in position order with DEGREES forward edges, the
    targets dealt round-robin to pickers 1..k-1 (so K >= 3 walks several grids per box)."""
    rng = np.random.default_rng(k)
    pickers = [[] for _ in range(k)]
    for i, d in enumerate(DEGREES):
        pickers[0].append((300 * i, 20))
        for t in range(d):
            pickers[1 + t % (k - 1)].append((300 * i + int(rng.integers(-8, 9)),
                                             20 + int(rng.integers(-8, 9))))
    pickers[k - 1].append((2500, 400))   # (every picker has a box; opens a second grid row)
    return _mg(pickers, shift, k)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("k", [2, 3, 4, 5])
def test_degrees_side_by_side(k, shift):
    mg = _degree_case(k, shift)
    assert sum(len(t[0]) for t in mg) <= 64          # one block, one wave
    edges = _both(mg)
    deg = np.bincount([u for (u, _, _) in edges], minlength=len(DEGREES))[:len(DEGREES)]
    assert deg.tolist() == DEGREES


@pytest.mark.parametrize("k", [3, 4])
def test_get_cc_components_of_different_sizes(k):
    """--get_cc on the degree case: components of 2..10 nodes and a box without any edge."""
    mg = _degree_case(k, 0.0)
    _check_vs_oracle([mg], k, BOX, get_cc=True)
    _check_vs_oracle([mg], k, BOX, get_cc=True, no_fused=True)
    _routes_equal([mg], k, BOX, get_cc=True)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("k", [3, 4])
def test_edge_past_the_mask(k, shift):
    """A picker-0 box with 40 candidates in picker 1's grid and edges at candidates 33, 35, 37,
    39 (re-tested by the list write: no mask bit).  K = 3: the joined walk of both grids;
    K = 4: a fourth picker, one loop per grid, the second and third past the mask."""
    mg = _mask_case((33, 35, 37, 39), 3, shift)
    if k == 4:
        mg = mg + _mg([[(458, 277), (99, 482)]], shift, 4)
    edges = _both(mg)
    b1 = len(mg[0][0])
    got = sorted(v - b1 for (u, v, _) in edges if u == 0)
    assert got[:4] == [33, 35, 37, 39] and len(got) == 4 + (k - 3)


def test_mixed_layout_batch():
    """Integer and fractional micrographs in one batch (the f32 pass defers the fractional
    ones to the f64 pass on the device)."""
    mgs = [_degree_case(3, 0.0), _degree_case(3, 0.125), _line([range(40)] * 3, 0.125),
           _line([range(43)] * 3, 0.0), _random_mg(3, 200, 0.125, seed=8, size=1500),
           _random_mg(3, 200, 0.0, seed=9, size=1500)]
    _check_vs_oracle(mgs, 3, BOX)
    _routes_equal(mgs, 3, BOX)


def _n_edges(mg, box):
    B = float(box)
    E = 0
    for a in range(len(mg)):
        for b in range(a + 1, len(mg)):
            xo = np.maximum(B - np.abs(mg[a][0][:, None] - mg[b][0][None, :]), 0.0)
            yo = np.maximum(B - np.abs(mg[a][1][:, None] - mg[b][1][None, :]), 0.0)
            inter = xo * yo
            E += int((inter / (2 * B * B - inter) > 0.3).sum())
    return E


# 3 x 334 = 1002 boxes: size class 1024, integer layout.  fused_layout: header 640 B, 8 + 4
# (cnt) + 2 (pos) + 2 (vrank) + 8 (cell starts) + 2 (parents) + 2 + 2 (scell, citems) + 1
# (flags) = 31 B per box -> 31 * 1024 + 16 + 16 + 16 (paddings) = 31792 B, fwd 2 * (16 * 65 + 4)
# = 2088 -> 2096 B: 34528 B without dst.  plan_fused: with ecap = nmax that is 36576 B = 29
# allocation blocks of 1280 B, 128 / 29 = 4 workgroups per CU (registers allow 4 of 512
# threads), budget 32 blocks = 40960 B, ecap = (40960 - 34528) / 2 = 3216, ecap / 2 = 1608.
# The field's side sets the density: 1140, 2195, 2934 and 3866 edges for seed 11.
ECAP_1024 = 3216
REGIMES = [(4096, "sources"), (1400, "per_box"), (1100, "per_box"), (900, "deferred")]


@pytest.mark.parametrize("size,regime", REGIMES)
def test_capacity_regimes(size, regime):
    """2 E <= ecap: edge sources written behind the targets, edge-parallel union; ecap / 2 < E
    <= ecap: no room for the sources, union per box; E > ecap: status DEFER, served by a
    later pass of the host.  The regime is asserted on the host's edge count, and the deferral
    on the launches the host made (so a plan whose ecap left (2934, 3866) would fail here)."""
    mg = _random_mg(3, 334, 0.0, seed=11, size=size)
    E = _n_edges(mg, BOX)
    assert {"sources": E <= ECAP_1024 // 2,
            "per_box": ECAP_1024 // 2 + 64 < E <= ECAP_1024 - 64,
            "deferred": E > ECAP_1024 + 64}[regime], E
    assert len(_both(mg)) == E
    assert _deferred(mg) == (regime == "deferred")


def _deferred(mg):
    """Whether the fused kernel's first pass returned the micrograph with status DEFER: the host
    then launches the fused kernel again for it (the f64 layout's classes have a larger ecap;
    after that one workgroup per CU, then the multi-kernel route), and the timing hook lists
    every launch.  One integer micrograph that fits is one launch."""
    from repic_amd import _lib
    from repic_amd.pipeline import Batch
    batch = Batch.pack(3, BOX, [mg])
    ctx = _lib.Context(0)
    r = ctx.run(1, 3, BOX, batch.box_off, batch.id_base, batch.x, batch.y, batch.score,
                _lib.F_HOST_OUTPUTS | _lib.F_TIMING)
    launches = [n for n, _ in ctx.kernel_times() if n == "k_fused"]
    assert (np.asarray(r.status) == _lib.OK).all() and launches
    ctx.close()
    return len(launches) > 1


def test_repeated_runs_are_identical():
    """The lists' places in dst follow the waves' arrival order; no output may: the densest
    fused case five times in one process, array by array as the device wrote them."""
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    mgs = [_random_mg(3, 334, 0.0, seed=11, size=1100), _random_mg(3, 334, 0.0, seed=12, size=4096),
           _degree_case(4, 0.0)[:3]]
    batch = Batch.pack(3, BOX, mgs)
    ctx = _lib.Context(0)
    runs = []
    for _ in range(5):
        res = run_batch(ctx, batch, get_cc=True)
        runs.append([(_fields(r), r.rows.copy(), r.w.copy(), r.conf.copy(), r.consensus.copy())
                     for r in res])
    ctx.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert a[0] == b[0]
            for x, y in zip(a[1:], b[1:]):
                assert np.array_equal(x, y)
