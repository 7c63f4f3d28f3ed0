"""The set-packing solver (rgc_ilp.hip, ilp_core / ilp_solve_rec of rgc_ilp_host.cpp) on models built
to put one conflict component on each size at which it takes another path, and on the inputs
its ABI allows but get_cliques never produces (tests/ilp_models.py).

Tier A ("must prove"): the restatement of the documented search (oracle/ilp_search_ref.py)
finishes each model within half of the device's node budget (tests/test_ilp_search_model.py)
and bounds the device's node count from above, so the device must end OPTIMAL with gap 0, at
HiGHS' objective, and with the restatement's x bit for bit: the first optimal leaf in
heaviest-first order, also where weights tie and HiGHS may return another optimum.

Tier B ("honest status"): models the search does not finish.  Any status may come back; what
it claims is checked against HiGHS (and the chain DP) with the tolerances of tests/test_ilp.py.
"""
import ctypes as C

import numpy as np
import pytest
from scipy.sparse import coo_matrix

import ilp_models as M
from test_ilp import highs

pytestmark = pytest.mark.gpu

RTOL = 1e-12
STATUS_NAME = {0: "NODE_LIMIT", 1: "OPTIMAL", 2: "GAP_OK", 3: "HEURISTIC"}


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_SOLO = {}


def _solve(ctx, mats, ws, node_limit=0):
    """[(x, status, relative gap, exact per column, gap per column)] of one solve_batch call."""
    from repic_amd.ilp import solve_batch
    xs, st, rel, cols = solve_batch(ctx, mats, ws, node_limit=node_limit, statuses=True,
                                    gaps=True, columns=True)
    return [(x.copy(), s, g, ex.copy(), gp.copy()) for x, s, g, (ex, gp) in zip(xs, st, rel, cols)]


def solo(ctx, name):
    """A model solved alone (kmax = its own row count), once per test process."""
    if name not in _SOLO:
        A, w = M.model(name)
        _SOLO[name] = _solve(ctx, [A], [w], M.node_limit(name))[0]
    return _SOLO[name]


def _objective(w, x):
    return float(np.asarray(w, np.float64)[x == 1].sum())


def _assert_proven(A, w, res, x_want):
    """Tier A's demands on one model's result."""
    from oracle import ilp_ref
    from repic_amd.ilp import OPTIMAL
    x, st, rel, ex, gp = res
    assert np.all(ex == OPTIMAL), np.unique(ex)
    assert st == OPTIMAL
    assert ilp_ref.is_packing(A, x)
    obj, objr = _objective(w, x), highs(A, w)[1]
    assert abs(obj - objr) <= RTOL * max(1.0, objr), (obj, objr)
    assert np.array_equal(x, x_want), (np.flatnonzero(x), np.flatnonzero(x_want))
    assert rel == 0.0 and not gp.any()


@pytest.mark.parametrize("name", M.TIER_A)
def test_gpu_ilp_tier_a_proves_the_first_optimal_leaf(ctx, name):
    from oracle import ilp_search_ref
    A, w = M.model(name)
    x_want, _, nodes, proven = ilp_search_ref.solve(A, w)
    assert proven and 2 * nodes <= ilp_search_ref.node_budget(A.shape[1])
    _assert_proven(A, w, solo(ctx, name), x_want)
    dp = M.chain_reference(name)
    if dp is not None:
        assert abs(_objective(w, solo(ctx, name)[0]) - dp) <= RTOL * max(1.0, dp)


def test_gpu_ilp_singletons_chosen_iff_weight_positive(ctx):
    from repic_amd.ilp import OPTIMAL
    A = coo_matrix((np.ones(3, np.int64), ([0, 1, 2], [0, 0, 0])), shape=(3, 1))
    for wv, want in ((0.0, 0), (0.5, 1), (np.float32(1e-30), 1)):
        x, st, rel, ex, gp = _solve(ctx, [A], [np.array([wv], np.float32)])[0]
        assert x.tolist() == [want] and ex.tolist() == [OPTIMAL] and st == OPTIMAL
        assert rel == 0.0 and not gp.any()


def _assert_honest(name, A, w, res, dp=None):
    """Tier B's demands: whatever status comes back, its claim holds against the optimum."""
    from oracle import ilp_ref
    from repic_amd.ilp import GAP_OK, OPTIMAL
    x, st, rel, ex, gp = res
    assert ilp_ref.is_packing(A, x)
    obj, opt = _objective(w, x), highs(A, w)[1]
    if dp is not None:
        assert abs(dp - opt) <= RTOL * max(1.0, opt), (dp, opt)
    g = (opt - obj) / opt
    print(f"{name}: {A.shape[1]} columns, status {STATUS_NAME[st]}, reported gap {rel:.3e}, "
          f"true gap {g:.3e}, column statuses {sorted(STATUS_NAME[s] for s in set(ex.tolist()))}")
    assert len(set(ex.tolist())) == 1   # one component: one status
    assert g >= -RTOL
    if st == OPTIMAL:
        assert g <= RTOL and rel == 0.0
    elif st == GAP_OK:
        assert g <= 1e-4
    else:
        assert g <= rel + RTOL, (g, rel)
    if dp is not None:
        gd = (dp - obj) / dp
        assert -RTOL <= gd <= (RTOL if st == OPTIMAL else 1e-4 if st == GAP_OK else rel + RTOL)


@pytest.mark.parametrize("name", M.TIER_B)
def test_gpu_ilp_tier_b_status_is_honest(ctx, name):
    A, w = M.model(name)
    _assert_honest(name, A, w, solo(ctx, name), M.chain_reference(name))


def test_gpu_ilp_batch_invariance_with_mixed_row_counts(ctx):
    """All Tier A and Tier B models in one batch, then in reversed order: kmax = 8 holds for
    the 2-, 3- and 5-row models too (the pad-with-the-last-row paths of ilp_rows_step and of
    both bounds), the LDS row-info limit moves to n <= 1820, and every model's x, statuses
    and gaps are those of its solo solve.  (chain64-limit64 is chain64-uniform under another
    node_limit, which is per call: it is left to its solo test.)"""
    names = [n for n in M.TIER_A + M.TIER_B if M.node_limit(n) == 0]
    assert {int(M.model(n)[0].tocsc().getnnz(axis=0).max()) for n in names} >= {2, 3, 5, 8}
    for order in (names, names[::-1]):
        got = _solve(ctx, [M.model(n)[0] for n in order], [M.model(n)[1] for n in order])
        for n, (x, st, rel, ex, gp) in zip(order, got):
            xs, sts, rels, exs, gps = solo(ctx, n)
            assert np.array_equal(x, xs), n
            assert st == sts and np.array_equal(ex, exs), (n, st, sts)
            assert rel == rels and np.array_equal(gp, gps), (n, rel, rels)


def test_gpu_ilp_ragged_columns_in_a_kmax8_batch(ctx):
    """Columns of 1..8 rows side by side (about a third of each cluster's columns lost one or
    two rows): HiGHS' objective and, as in Tier A (the restatement proves each within half
    the budget), OPTIMAL with the restatement's x."""
    from oracle import ilp_ref, ilp_search_ref
    probs = M.ragged_models()
    deg = np.concatenate([A.tocsc().getnnz(axis=0) for A, _ in probs])
    assert deg.min() == 1 and deg.max() == 8 and all(A.shape[1] <= 129 for A, _ in probs)
    got = _solve(ctx, [A for A, _ in probs], [w for _, w in probs])
    for (A, w), (x, st, rel, ex, gp) in zip(probs, got):
        assert ilp_ref.is_packing(A, x)
        obj, objr = _objective(w, x), highs(A, w)[1]
        assert abs(obj - objr) <= RTOL * max(1.0, objr), (obj, objr)
        x_want, _, nodes, proven = ilp_search_ref.solve(A, w)
        assert proven and 2 * nodes <= ilp_search_ref.DEFAULT_NODES
        _assert_proven(A, w, (x, st, rel, ex, gp), x_want)


def test_gpu_ilp_rows_without_columns(ctx):
    """Two of every three rows unused, and fifty unused rows at the end: the same result as
    the dense numbering."""
    for name in ("n65-uniform", "n64-tied", "n129-tied"):
        A, w = M.model(name)
        A = A.tocoo()
        B = coo_matrix((A.data, (A.row * 3 + 1, A.col)), shape=(3 * A.shape[0] + 50, A.shape[1]))
        x, st, rel, ex, gp = _solve(ctx, [B], [w])[0]
        xs, sts, rels, exs, gps = solo(ctx, name)
        assert np.array_equal(x, xs) and st == sts and rel == rels
        assert np.array_equal(ex, exs) and np.array_equal(gp, gps)


def test_gpu_ilp_zero_weight_columns_among_positive_ones(ctx):
    from oracle import ilp_ref, ilp_search_ref
    probs = M.zero_weight_models()
    assert all((w == 0).any() and (w > 0).any() for _, w in probs)
    for A, w in probs:
        res = _solve(ctx, [A], [w])[0]
        assert ilp_ref.is_packing(A, res[0])
        obj, objr = _objective(w, res[0]), highs(A, w)[1]
        assert abs(obj - objr) <= RTOL * max(1.0, objr), (obj, objr)
        x_want, _, nodes, proven = ilp_search_ref.solve(A, w)
        assert proven and 2 * nodes <= ilp_search_ref.DEFAULT_NODES
        _assert_proven(A, w, res, x_want)


def test_gpu_ilp_no_columns(ctx):
    from repic_amd.ilp import OPTIMAL, solve_batch
    for shape in ((0, 0), (7, 0)):
        A = coo_matrix(shape, dtype=np.int64)
        (x, st, rel, ex, gp), = _solve(ctx, [A], [np.zeros(0, np.float32)])
        assert x.shape == ex.shape == gp.shape == (0,) and x.dtype == np.uint8
        assert st == OPTIMAL and rel == 0.0
    assert solve_batch(ctx, [], []) == ([], [])
    # an empty model between two others keeps its place
    A, w = M.model("n2-tied")
    got = _solve(ctx, [A, coo_matrix((4, 0), dtype=np.int64), A], [w, np.zeros(0, np.float32), w])
    assert len(got[1][0]) == 0 and np.array_equal(got[0][0], got[2][0])
    assert np.array_equal(got[0][0], solo(ctx, "n2-tied")[0])


def test_gpu_ilp_many_tiny_components(ctx):
    """3,000 components of one column (some of weight 0) or of two columns sharing a box."""
    from repic_amd.ilp import OPTIMAL
    rng = np.random.default_rng(5)
    rows, cols, want, r, c = [], [], [], 0, 0
    w = []
    for i in range(3000):
        if i % 2 == 0:
            wv = np.float32(0.0) if i % 10 == 0 else np.float32(rng.uniform(0.1, 1.0))
            rows += [r, r + 1, r + 2]
            cols += [c] * 3
            want.append(1 if wv > 0 else 0)
            w.append(wv)
            r, c = r + 3, c + 1
        else:
            a, b = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), 2)
            rows += [r, r + 1, r + 1, r + 2]
            cols += [c, c, c + 1, c + 1]
            want += [1, 0] if a >= b else [0, 1]   # ties: the lower column comes first
            w += [a, b]
            r, c = r + 3, c + 2
    w = np.array(w, np.float32)
    A = coo_matrix((np.ones(len(rows), np.int64), (rows, cols)), shape=(r, c))
    x, st, rel, ex, gp = _solve(ctx, [A], [w])[0]
    assert np.all(ex == OPTIMAL) and st == OPTIMAL and rel == 0.0 and not gp.any()
    assert np.array_equal(x, np.array(want, np.uint8))
    closed = float(np.asarray(w, np.float64)[np.array(want) == 1].sum())
    assert _objective(w, x) == closed


def _raw_solve(ctx, col_ptr, row_idx, w, n_rows):
    """rgc_ilp_solve on raw CSC arrays (solve_batch only builds valid ones)."""
    from repic_amd import _lib
    from repic_amd.ilp import IlpIn
    col_ptr = np.ascontiguousarray(col_ptr, np.int64)
    row_idx = np.ascontiguousarray(row_idx, np.int32)
    w = np.ascontiguousarray(w, np.float64)
    nc = len(col_ptr) - 1
    x, ex, gp = np.zeros(nc, np.uint8), np.zeros(nc, np.uint8), np.zeros(nc, np.float64)
    si = IlpIn(nc, n_rows, col_ptr.ctypes.data, row_idx.ctypes.data, w.ctypes.data, 0, 0,
               gp.ctypes.data, 0.0)
    ctx._retire()
    _lib._check(_lib.lib.rgc_ilp_solve(ctx._p, C.byref(si), x.ctypes.data, ex.ctypes.data))
    return x, ex, gp


def test_gpu_ilp_validation_errors_leave_the_context_usable(ctx):
    from repic_amd import _lib
    from repic_amd.ilp import OPTIMAL
    w2 = [0.5, 0.25]
    bad = [
        ([1, 2, 3], [0, 1, 1], w2, 3, "col_ptr must start at 0"),
        ([0, 2, 2], [0, 1], w2, 3, "every column needs at least one row"),
        ([0, 9, 10], list(range(9)) + [0], w2, 9, "columns of more than 8 rows"),
        ([0, 2, 3], [0, 3, 1], w2, 3, "row index out of range"),
        ([0, 2, 3], [0, -1, 1], w2, 3, "row index out of range"),
    ]
    for col_ptr, row_idx, w, n_rows, msg in bad:
        with pytest.raises(_lib.RGCError, match=msg):
            _raw_solve(ctx, col_ptr, row_idx, w, n_rows)
        # the same context solves a valid model afterwards: two columns sharing row 1
        x, ex, gp = _raw_solve(ctx, [0, 2, 4], [0, 1, 1, 2], w2, 3)
        assert x.tolist() == [1, 0] and ex.tolist() == [OPTIMAL] * 2 and not gp.any()
    A, w = M.model("n65-tied")
    res = _solve(ctx, [A], [w])[0]
    assert np.array_equal(res[0], solo(ctx, "n65-tied")[0]) and res[1] == OPTIMAL
