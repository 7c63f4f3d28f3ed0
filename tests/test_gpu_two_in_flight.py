"""The staged per-box, per-edge and per-vertex loops of the fused kernel's P1, P2c, P3, P5 and
P6a (rgc_fused.hip).

Each loop is a plain `for (i = tid; i < n; i += FWG)` loop (P1: the RB register boxes, then
the HBM tail) whose iteration is staged: the loads at known addresses first, then the flag
test, then the action.  A thread's second item, and any item behind it, goes through the same
body again.  (The module's name dates from the form that ran two items of a thread at once,
measured and not selected.)  The cases are the smallest micrographs at which that can go
wrong: total box counts around the places where a thread gains or loses its second item in each
instance (256 threads: RB = 4, classes up to 512 boxes; 512 threads: RB = 2; 768 threads:
classes 1409..1536), a thread's items in one packed counter word (P1's cell counters, P5's
x-bucket counters), its edges in one component, the per-box union of the capacity regime
without edge sources, K = 2 and K = 5, and repeated runs of a dense batch.  Every micrograph
is compared bit for bit with the oracle (edge set with JI bits through RGC_F_EDGES, rows, w,
conf, consensus, cc_max / cc_cnt) and the fused route with the multi-kernel route; every
case's oracle status is OK (asserted).
"""
import numpy as np
import pytest

from test_gpu_p2_flat import BOX, LAYOUTS, _check, _mg, _random_mg
from test_gpu_p2_onepass import ECAP_1024, _fields, _routes_equal
from test_gpu_parity import _check_vs_oracle

pytestmark = pytest.mark.gpu


def _both(mg, k=3, get_cc=False):
    """Edges and outputs against the oracle (status OK), then the other route.  Returns the
    edges."""
    from repic_amd import _lib
    edges = _check(mg, BOX)
    if get_cc:
        _check_vs_oracle([mg], k, BOX, get_cc=True)
    assert _routes_equal([mg], k, BOX, get_cc=get_cc)[0].status == _lib.OK
    return edges


def _per(n, k=3):
    per = [(n + k - 1 - p) // k for p in range(k)]
    assert sum(per) == n
    return per


# field sides: about the density of the other files' cases (a few edges per ten boxes), so
# every case has cliques and stays far below its class's edge capacity
@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("n,size", [(255, 2200), (256, 2200), (257, 2200), (511, 3000),
                                    (512, 3000), (513, 3000), (575, 3000), (1023, 4096),
                                    (1024, 4096), (1025, 4096), (1409, 4500), (1535, 4500),
                                    (1536, 4500)])
def test_round_boundaries(n, size, shift):
    """256 threads: the second item appears at 257 boxes (255, 256: none), 511 / 512 are the
    last sizes of the instance; 512 threads: one lane, one wave and all lanes but one hold a
    second item (513, 575, 1023), all (1024), and the loop behind the pair runs (1025);
    768 threads: the ends of its classes."""
    assert _both(_random_mg(3, _per(n), shift, seed=n, size=size))


def _clump(rows, shift):
    """Picker 0: 600 boxes on distinct pixels of one grid column and `rows` grid rows (cells are
    >= 108 x 54 px), so boxes i and i + 512 of the picker share a cell counter (rows = 1: one
    u16 half; rows = 3: three consecutive keys, so two of them share a word); pickers 1 and 2 far
    from it.  Three particles elsewhere give the cliques."""
    rng = np.random.default_rng(rows)
    cells = [(x, y) for x in range(0, 100, 2) for y in range(0, 54 * rows - 4, 2)]
    pick = rng.permutation(len(cells))[:600]
    parts = [(900, 300), (1500, 900), (1900, 1900)]
    p0 = [cells[i] for i in pick] + parts
    p1 = [(x + 3, y - 2) for (x, y) in parts] + [(1000, 1500)]
    p2 = [(x - 4, y + 5) for (x, y) in parts] + [(400, 1900)]
    return _mg([p0, p1, p2], shift, rows)


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("rows", [1, 3])
def test_items_share_a_cell_counter(rows, shift):
    assert len(_both(_clump(rows, shift))) == 9


def _lines(xs, shift):
    """200 particles 300 px apart in y, particle j on the vertical line x = xs[j % len(xs)],
    one box per picker: every third particle's boxes coincide (ties on x and y, ranked by id),
    the others differ in y only.  600 clique vertices: vertices u and u + 512 of the dense list
    share an x bucket (one line: every vertex in bucket 0; lines at x = 0, 2 and 1000: buckets
    0 and 1, one counter word, and the last)."""
    pk = [[], [], []]
    for j in range(200):
        for p in range(3):
            pk[p].append((xs[j % len(xs)], 300 * j + (0 if j % 3 == 0 else 5 * p)))
    return _mg(pk, shift, len(xs))


@pytest.mark.parametrize("shift", LAYOUTS)
@pytest.mark.parametrize("xs", [(0,), (0, 2, 1000)], ids=["one_bucket", "adjacent_buckets"])
def test_vertices_share_an_x_bucket(xs, shift):
    assert len(_both(_lines(xs, shift))) == 600


def _chain(n, shift):
    """n boxes 25 px apart on a line, box j of picker j % 3: edges (j, j + 1) and (j, j + 2),
    2 n - 3 in all, one component, n - 2 triangles."""
    pk = [[], [], []]
    for j in range(n):
        pk[j % 3].append((25 * j, 40))
    return _mg(pk, shift, n)


@pytest.mark.parametrize("get_cc", [False, True])
@pytest.mark.parametrize("shift", LAYOUTS)
def test_edges_of_a_thread_in_one_component(shift, get_cc):
    """1197 edges on 512 threads (2 E <= ecap: the edge-parallel union): edges e and e + 512
    unite the same tree concurrently.  cc_cnt = 1 and cc_max = 600 by _check_vs_oracle."""
    assert len(_both(_chain(600, shift), get_cc=get_cc)) == 2 * 600 - 3


@pytest.mark.parametrize("get_cc", [False, True])
def test_per_box_union_regime(get_cc):
    """ecap / 2 < E <= ecap (test_gpu_p2_onepass.REGIMES "per_box"): no room for the edge
    sources, the staged source loop (P2c) unites per box on the u16 parents."""
    mg = _random_mg(3, 334, 0.0, seed=11, size=1400)
    E = len(_both(mg, get_cc=get_cc))
    assert ECAP_1024 // 2 < E <= ECAP_1024


@pytest.mark.parametrize("k,n,size", [(2, 513, 2000), (5, 515, 2500), (5, 1025, 3600)])
def test_other_instances(k, n, size):
    assert _both(_random_mg(k, _per(n, k), 0.0, seed=k, size=size), k=k)


def test_dense_batch_repeats():
    """256 micrographs of about 900 boxes (C2) five times on one context: equal array by array
    (the arrival orders of the LDS atomics differ from run to run; no output may)."""
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch, run_batch
    cfg = synth.SynthConfig(**synth.CONFIGS["C2"], seed=7)
    batch = Batch.pack(cfg.k, cfg.box, synth.batch(cfg, 256))
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
