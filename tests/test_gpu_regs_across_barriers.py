"""Values the fused kernel keeps in registers across barriers, or hands from one phase to the
next, instead of parking them in LDS (rgc_fused.hip):

* P1: the count pass's returning atomic gives a box's arrival ordinal within its bucket; key
  and ordinal of a thread's first boxes stay in one register up to the placement, the boxes
  behind them (512-thread instance, from 1025 boxes) park both in LDS.
* P2 writes `split`, the end of the first picker segment of every box's list, from the edges
  it counted in the first target grid; P3b no longer searches for it.
* P3b: one loop compresses, counts nodes and roots and takes the largest component from the
  size counter's returning atomic; the barrier behind it is gone where P4's root pass only
  reads.
* P5: bucket and ordinal of a thread's first positions stay in one register across the scan.

The cases are the smallest micrographs at which each of these can go wrong.  Every micrograph
is compared bit for bit with the oracle (edge set with JI bits through RGC_F_EDGES, rows, w,
conf, consensus, n_nodes, cc_cnt, cc_max) and the fused route with the multi-kernel route, on
the integer and the fractional (f64) layout; every case's oracle status is OK (asserted).  The
thread-count boundaries of the instances are test_gpu_two_in_flight.py's cases.
"""
import numpy as np
import pytest

from test_gpu_p2_flat import BOX, LAYOUTS, _check, _mask_case, _mg, _random_mg
from test_gpu_p2_onepass import ECAP_1024, _fields, _line, _routes_equal
from test_gpu_parity import _check_vs_oracle
from test_gpu_two_in_flight import _chain

pytestmark = pytest.mark.gpu


def _full(mg, get_cc=False):
    """Edges and outputs against the oracle (status OK), n_nodes against the edge set, then
    the other route.  Returns the edges."""
    from repic_amd import _lib
    from repic_amd.pipeline import Batch
    k = len(mg)
    edges = _check(mg, BOX)
    if get_cc:
        _check_vs_oracle([mg], k, BOX, get_cc=True)
    assert _routes_equal([mg], k, BOX, get_cc=get_cc)[0].status == _lib.OK
    batch = Batch.pack(k, BOX, [mg])
    ctx = _lib.Context(0)
    r = ctx.run(1, k, BOX, batch.box_off, batch.id_base, batch.x, batch.y, batch.score,
                _lib.F_HOST_OUTPUTS | (_lib.F_GET_CC if get_cc else 0))
    n_nodes = int(r.n_nodes[0])
    ctx.close()
    assert n_nodes == len({u for (u, _, _) in edges} | {v for (_, v, _) in edges})
    return edges


# ---------------------------------------------------------------------------------------- P1
def _cell_clump(n, k, shift, extra=()):
    """Picker 0: n boxes on distinct pixels of the grid cell at the field's origin (x < 100,
    y < 50; cells are >= 108 x 54 px), so their arrival ordinals run to n - 1 in one bucket
    counter; every other picker far from them.  Three particles elsewhere, one box per picker,
    give the cliques.  `extra`: further picker-0 boxes."""
    rng = np.random.default_rng(n + k)
    cells = [(x, y) for x in range(0, 100, 2) for y in range(0, 50, 2)]
    pick = rng.permutation(len(cells))[:n]
    parts = [(900, 300), (1500, 900), (1900, 1900)]
    pk = [[cells[i] for i in pick] + parts + list(extra)]
    for p in range(1, k):
        pk.append([(x + 3 * p, y - 2 * p) for (x, y) in parts] + [(400 + 150 * p, 1900)])
    return _mg(pk, shift, n)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("n", [70, 300])
def test_p1_ordinals_past_63_and_255(n, shift):
    assert len(_full(_cell_clump(n, 3, shift))) == 9


@pytest.mark.parametrize("k", [2, 5])
def test_p1_other_k(k):
    assert len(_full(_cell_clump(70, k, 0.0))) == 3 * k * (k - 1) // 2


@pytest.mark.parametrize("shift", LAYOUTS)
def test_p1_duplicate_coordinates(shift):
    """Boxes of one picker on the same pixel (same bucket, same coordinates): the placement
    orders them by local index, whatever their arrival order.  Picker 0 holds particle 0 four
    times and picker 1 holds it twice, so the copies are clique vertices whose rows and
    consensus depend on that order."""
    p0 = [(300, 300)] * 4 + [(900, 700), (900, 700), (40, 40)]
    p1 = [(303, 298)] * 2 + [(905, 703), (1500, 100)]
    p2 = [(298, 304), (897, 698), (897, 698), (1200, 1200)]
    edges = _full(_mg([p0, p1, p2], shift, 5))
    assert len(edges) == (4 * 2 + 4 + 2) + (2 + 2 * 2 + 2)


@pytest.mark.parametrize("shift", LAYOUTS)
def test_p1_non_finite_boxes(shift):
    """Non-finite boxes in every picker: the "none" bucket (key nkey, behind every grid) takes
    ordinals and a start of its own; they are no candidates and no nodes."""
    nan, inf = float("nan"), float("inf")
    mg = _random_mg(3, 60, 0.0, seed=21, size=900)
    bad = [[(nan, 10.0), (20.0, inf), (nan, nan)], [(-inf, 5.0)], [(7.0, nan), (inf, -inf)]]
    out = []
    for (x, y, s), b in zip(mg, bad):
        b = np.asarray(b)
        at = [0, len(x) // 2, len(x)][:len(b)]
        out.append((np.insert(x, at, b[:, 0]) + shift, np.insert(y, at, b[:, 1]) + shift,
                    np.insert(s, at, 0.5)))
    assert _full(out)


def _full_line(n, shift):
    """n boxes over three pickers, one box per picker and particle on a line (every particle a
    3-clique, so every box is a clique vertex)."""
    per = [(n + 2 - p) // 3 for p in range(3)]
    assert sum(per) == n
    return _line([range(c) for c in per], shift, seed=n)


@pytest.mark.parametrize("n,shift", [(1023, 0.0), (1024, 0.0), (1025, 0.0), (1025, 0.125),
                                     (1050, 0.0)])
def test_p1_p5_tail_behind_the_register_items(n, shift):
    """512 threads hold two boxes each in registers: at 1025 boxes the first box takes P1's
    path through pos[i] / citems[i] and the first position P5's path through vrank (the last
    positions are picker-2 boxes of cliques); at 1050 a part of a wave does."""
    edges = _full(_full_line(n, shift))
    assert len(edges) >= 3 * ((n - 2) // 3)


# ---------------------------------------------------------------------------------- P2 split
@pytest.mark.parametrize("get_cc", [False, True])
@pytest.mark.parametrize("shift", LAYOUTS)
def test_split_segments(shift, get_cc):
    """Picker-0 boxes whose edges go to picker 2 only (split = begin), to picker 1 only
    (split = end), to both, and a box with five edges (two in the first grid: the mask path);
    picker-1 boxes with and without a forward edge; picker-2 boxes with incoming edges only.
    The 3-cliques found through the splits are compared by _check."""
    p0 = [(300, 300), (800, 300), (1300, 300), (300, 900), (1800, 900)]
    p1 = [(803, 302), (1297, 303), (296, 903), (304, 897), (1500, 1500)]
    p2 = [(302, 297), (1303, 297), (299, 899), (303, 904), (297, 905), (1795, 903)]
    edges = _full(_mg([p0, p1, p2], shift, 2), get_cc=get_cc)
    deg = np.bincount([u for (u, _, _) in edges], minlength=10)[:10]
    assert deg.tolist() == [1, 1, 2, 5, 1, 0, 1, 3, 3, 0]


@pytest.mark.parametrize("shift", LAYOUTS)
def test_split_with_edges_past_the_mask(shift):
    """A picker-0 box with 40 candidates in its first grid, edges at candidates 33, 35, 37 and
    39 (counted, but without a mask bit) and one edge in the second grid: split = begin + 4."""
    mg = _mask_case((33, 35, 37, 39), 3, shift)
    x, y, s = mg[2]
    mg[2] = (np.append(x, 458 + shift), np.append(y, 277 + shift), np.append(s, 0.5))
    edges = _full(mg)
    b1, b2 = len(mg[0][0]), len(mg[0][0]) + len(mg[1][0])
    assert sorted(v - b1 for (u, v, _) in edges if u == 0) == [33, 35, 37, 39, b2 - b1 + len(x)]


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("k", [4, 5])
def test_split_empty_first_segment(k, shift):
    """K = 4 / 5: a picker-0 box without a picker-1 neighbour and with neighbours in every
    later picker (split = begin, a k-1 clique short of k), beside a full particle."""
    pk = [[(300, 300), (900, 900)]] + [[(900 + 2 * p, 900 - 3 * p)] for p in range(1, k)]
    for p in range(2, k):
        pk[p].append((300 + 3 * p, 300 - 2 * p))
    pk[1].append((1500, 200))
    edges = _full(_mg(pk, shift, k))
    assert len(edges) == k * (k - 1) // 2 + (k - 1) * (k - 2) // 2


@pytest.mark.parametrize("shift", LAYOUTS)
def test_split_block_without_edges(shift):
    """128 picker-0 boxes in position order: the first block of 64 positions holds no edge
    (split = fwd = 0 for all of them), the second holds lists with one and two segments."""
    edges = _full(_line([range(128), range(64, 128), range(100, 128)], shift))
    assert min(u for (u, _, _) in edges) == 64


@pytest.mark.parametrize("shift", LAYOUTS)
def test_split_in_the_reversed_round(shift):
    """758 boxes on 512 threads: the second round writes its block's lists in reversed lane
    order; lists to picker 1 only, picker 2 only and both alternate along the positions."""
    p1 = [i for i in range(350) if i % 3]
    p2 = [i for i in range(350) if i % 2 == 0]
    edges = _full(_line([range(350), p1, p2], shift))
    assert len(edges) == len(p1) + len(p2) + len(set(p1) & set(p2))


# --------------------------------------------------------------------------------------- P3b
@pytest.mark.parametrize("get_cc", [False, True])
@pytest.mark.parametrize("shift", LAYOUTS)
def test_one_component_of_300_nodes(shift, get_cc):
    """cc_max = 300 > 255 from the returned counter values; 256 threads, two positions each."""
    assert len(_full(_chain(300, shift), get_cc=get_cc)) == 2 * 300 - 3


@pytest.mark.parametrize("get_cc", [False, True])
@pytest.mark.parametrize("shift", LAYOUTS)
def test_components_tied_for_the_largest(shift, get_cc):
    """Six components of three nodes, two of two and two boxes without an edge."""
    edges = _full(_line([range(10), range(8), range(6)], shift), get_cc=get_cc)
    assert len(edges) == 3 * 6 + 2


@pytest.mark.parametrize("get_cc", [False, True])
@pytest.mark.parametrize("shift", LAYOUTS)
def test_largest_component_in_second_items(shift, get_cc):
    """3 x 100 particles (256 threads): the last particle has eight picker-2 boxes, positions
    299..306, each a thread's second item; its component of ten nodes is the largest."""
    mg = _line([range(100)] * 3, shift)
    x, y, s = mg[2]
    dx = np.array([-6, -4, -2, 2, 4, 6, 8.0])
    mg[2] = (np.append(x, x[-1] + dx), np.append(y, y[-1] + dx[::-1]), np.append(s, 0.4 + dx / 40))
    edges = _full(mg, get_cc=get_cc)
    assert len(edges) == 3 * 99 + 1 + 2 * 8


@pytest.mark.parametrize("get_cc", [False, True])
def test_per_box_union_on_u16_parents(get_cc):
    """ecap / 2 < E <= ecap: no edge sources, the unions run per box on the u16 parents and
    the finds of P3b's loop compress those."""
    E = len(_full(_random_mg(3, 334, 0.0, seed=11, size=1100), get_cc=get_cc))
    assert ECAP_1024 // 2 < E <= ECAP_1024


# ---------------------------------------------------------------------------------------- P5
def _vlines(xs, n, shift, doubles=0):
    """n particles 300 px apart in y, particle j on the vertical line x = xs[j % len(xs)], one
    box per picker (3 n clique vertices); the first `doubles` particles hold a second picker-0
    box (one more vertex each)."""
    pk = [[], [], []]
    for j in range(n):
        for p in range(3):
            pk[p].append((xs[j % len(xs)], 300 * j + 5 * p))
        if j < doubles:
            pk[0].append((xs[j % len(xs)], 300 * j + 7))
    return _mg(pk, shift, n)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("xs", [(0,), (0, 2, 1000)], ids=["one_bucket", "shared_word"])
def test_p5_vertices_in_one_bucket(xs, shift):
    """90 clique vertices: on one line all in x bucket 0 (ordinals to 89); on lines at x = 0, 2
    and 1000 in buckets 0 and 1 (one counter word) and the last."""
    assert len(_full(_vlines(xs, 30, shift))) == 90


@pytest.mark.parametrize("v", [511, 512, 513])
def test_p5_vertex_counts_around_512(v):
    n, doubles = {511: (170, 1), 512: (170, 2), 513: (171, 0)}[v]
    assert 3 * n + doubles == v
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    mg = _vlines((0, 700, 1400, 2100), n, 0.0, doubles)
    assert len(_full(mg)) == 3 * n + 2 * doubles
    ctx = _lib.Context(0)
    assert run_batch(ctx, Batch.pack(3, BOX, [mg]))[0].n_vert == v
    ctx.close()


# ----------------------------------------------------------------------------------- repeats
def test_dense_batch_five_times():
    """64 micrographs of about 900 boxes five times on one context: equal array by array (the
    arrival ordinals of P1 and P5 and the lists' places differ from run to run; no output may)."""
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch, run_batch
    cfg = synth.SynthConfig(**synth.CONFIGS["C2"], seed=14)
    batch = Batch.pack(cfg.k, cfg.box, synth.batch(cfg, 64))
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
