"""CPU checks of the test infrastructure behind tests/test_gpu_ilp_edges.py: the restatement of
the device's branch and bound (oracle/ilp_search_ref.py) is an exact solver on the generators of
tests/ilp_models.py, every "must prove" model finishes in it within HALF of the device's node
budget for its size (the restatement's node count bounds the device's from above, so the GPU
test may demand OPTIMAL), and the committed HiGHS optima cover the large models.
"""
import numpy as np
import pytest

import ilp_models as M
from test_ilp import LIVE_MAX_COLS, highs

RTOL = 1e-12


def _close(a, b):
    return abs(a - b) <= RTOL * max(1.0, abs(b))


def _small_models():
    """Components of at most 18 columns from each generator, weight mode and option."""
    out = []
    for mode in (M.UNIFORM, M.TIED):
        for seed in range(3):
            out += [M.cluster((2, 2, 2), 2, mode, seed), M.cluster((3, 2, 2), 3, mode, seed),
                    M.cluster((2, 2, 2, 2), 2, mode, seed, zero_frac=0.3),
                    M.cluster((3, 3, 2), 0, mode, seed, ragged=True),
                    M.cluster((2, 2, 2, 2, 1, 1, 1, 1), 2, mode, seed, ragged=True),
                    M.cluster((4, 4), 0, mode, seed, subset=11),
                    M.chain(18, 3, 1, mode, seed), M.chain(17, 5, 2, mode, seed),
                    M.chain(18, 8, 3, mode, seed), M.bridged((2, 2, 2), 2, mode, seed),
                    M.bridged((2, 2), 3, mode, seed)]
    return out


def test_restatement_matches_brute_force_on_small_components():
    from oracle import ilp_ref, ilp_search_ref
    n = 0
    for A, w in _small_models():
        bf = ilp_ref.brute_force(A, w)
        assert bf is not None
        x, obj, nodes, proven = ilp_search_ref.solve(A, w)
        assert proven and ilp_ref.is_packing(A, x)
        assert _close(obj, bf[1]), (obj, bf[1])
        assert _close(obj, ilp_ref.milp(A, w)[1])
        assert _close(float(np.asarray(w, np.float64)[x == 1].sum()), obj)
        n += 1
    assert n >= 60


def test_chain_dp_matches_brute_force_and_milp():
    from oracle import ilp_ref
    for k, stride in ((3, 1), (5, 2), (8, 3), (4, 4), (2, 1)):
        for mode in (M.UNIFORM, M.TIED):
            A, w = M.chain(18, k, stride, mode, seed=k)
            dp = M.chain_optimum(w, k, stride)
            assert _close(dp, ilp_ref.brute_force(A, w)[1])
            assert _close(dp, ilp_ref.milp(A, w)[1])
    for name in M.TIER_A + M.TIER_B:
        dp = M.chain_reference(name)
        if dp is not None:
            assert _close(dp, highs(*M.model(name))[1]), name


def test_generators_give_one_component_of_the_listed_size():
    from oracle import ilp_ref
    for name in M.TIER_A + M.TIER_B:
        A, w = M.model(name)
        assert w.dtype == np.float32
        assert ilp_ref.components(A)[0] == 1, name
        if name in M.TIER_A:
            assert A.shape[1] == M.TIER_A_SIZES[name.rsplit("-", 1)[0]], name
    assert M.model("partial4097")[0].shape[1] == 4097 == M.model("chain4097")[0].shape[1]
    # the batch of all models mixes 2-, 3-, 5- and 8-row columns
    ks = {int(M.model(n)[0].tocsc().getnnz(axis=0).max()) for n in M.TIER_A}
    assert {2, 3, 5, 8} <= ks and max(ks) == 8
    # every size at which the solver takes another path, in both weight modes
    for size in (1, 2, 63, 64, 65, 127, 128, 129, 256, 1024, 1025, 2048, 2049, 3276, 3277, 4096):
        for mode in (M.UNIFORM, M.TIED):
            assert any(n.endswith(mode) and M.model(n)[0].shape[1] == size for n in M.TIER_A)
    # either side of the wave solver's LDS row-info limit, n (K + 1) <= 16384, at two K
    for a, b, K in (("n2048k7", "n2049k7", 7), ("n3276k4", "n3277k4", 4)):
        assert M.TIER_A_SIZES[a] * (K + 1) <= 16384 < M.TIER_A_SIZES[b] * (K + 1)
        assert int(M.model(a + "-tied")[0].tocsc().getnnz(axis=0).max()) == K


_SLOW = {"n2048k7", "n2049k7", "n3276k4", "n3277k4", "n4096"}


@pytest.mark.parametrize("name", [pytest.param(n, marks=pytest.mark.slow)
                                  if n.rsplit("-", 1)[0] in _SLOW else n for n in M.TIER_A])
def test_must_prove_model_finishes_within_half_the_device_budget(name):
    """The condition that makes the GPU test's demand (OPTIMAL, x bit for bit) legitimate."""
    from oracle import ilp_ref, ilp_search_ref
    A, w = M.model(name)
    x, obj, nodes, proven = ilp_search_ref.solve(A, w)
    budget = ilp_search_ref.node_budget(A.shape[1])
    print(f"{name}: {A.shape[1]} columns, {nodes} nodes of {budget}")
    assert proven and 2 * nodes <= budget, (nodes, budget)
    assert ilp_ref.is_packing(A, x)
    assert _close(obj, highs(A, w)[1]), (obj, highs(A, w)[1])


def test_restatement_matches_milp_on_ragged_and_zero_weight_models():
    """The degenerate inputs of the GPU module: 1..8 rows per column, zero weights."""
    from oracle import ilp_ref, ilp_search_ref
    for A, w in M.ragged_models() + M.zero_weight_models():
        x, obj, nodes, proven = ilp_search_ref.solve(A, w)
        print(A.shape, "nodes", nodes, "components", ilp_ref.components(A)[0])
        assert proven and ilp_ref.is_packing(A, x)
        assert _close(obj, ilp_ref.milp(A, w)[1])


def test_node_budget_is_the_documented_scaling():
    from oracle import ilp_search_ref as S
    assert S.DEFAULT_NODES == 1 << 14
    assert [S.node_budget(n) for n in (2, 64, 65, 1024)] == [1 << 14] * 4
    assert S.node_budget(1025) == (1 << 14) * 16 // 17
    assert S.node_budget(4096) == (1 << 14) * 16 // 64
    assert S.node_budget(2048, 1000) == 500


def test_restatement_reports_an_exhausted_budget():
    from oracle import ilp_ref, ilp_search_ref
    A, w = M.model("chain64-uniform")
    x, obj, nodes, proven = ilp_search_ref.solve(A, w, node_limit=64)
    assert not proven and nodes == 65 and ilp_ref.is_packing(A, x)
    assert obj <= M.chain_reference("chain64-uniform") * (1 + RTOL)


def test_large_models_are_in_the_highs_fixture():
    import make_ilp_golden
    tab = make_ilp_golden.load()
    names = M.fixture_models()
    big = [n for n in M.TIER_A + M.TIER_B if M.model(n)[0].shape[1] > LIVE_MAX_COLS]
    assert len(big) == 12 and set(big) <= set(names)
    for name in names:
        A, w = M.model(name)
        obj, sel = tab[make_ilp_golden.model_key(A, w)]
        assert _close(float(np.asarray(w, np.float64)[sel].sum()), obj), name
