"""The inputs of tests/test_gpu_large_route_edges.py sit on their edges: asserted from the
oracle alone (oracle/cpu_vec.py: its edge list, components and cliques), since the route a
micrograph takes on the device is not observable.  A builder that drifts off its edge fails
here, without a GPU."""
import numpy as np
import pytest

import large_route_models as lm


def _pin(model, d_max=None, get_cc=False):
    """The model's intended degree, box count and clique count hold on the oracle."""
    d, res = lm.oracle_facts(model, get_cc)
    assert d == (model.d_max if d_max is None else d_max)
    assert res["status"] == "ok" and len(res["members"]) >= 1
    if not get_cc and model.n_cliques is not None:
        assert len(res["members"]) == model.n_cliques
    return res


@pytest.mark.parametrize("k", range(2, 9))
def test_thin_shapes_sit_on_both_sides_of_the_bitmap_width(k):
    batch = lm.thin_batch(k)
    want = [d for d in (63, 64, 65) for _ in lm.thin_shapes(k, d)]
    assert [m.d_max for m in batch] == want
    assert {m.route for m in batch} == {"level", "dfs"}
    for m, d in zip(batch, want):
        x, y, s, pick, counts = m.flat()
        res = _pin(m)
        assert (m.route == "dfs") == (d > lm.RB_W)
        assert len(res["members"]) <= lm.REF_MAX_CLIQUES
        # the cluster's own cliques, and ordinary roots of 2..7 neighbours beside it
        root_deg = np.bincount(res["members"][:, 0], minlength=len(x))
        assert root_deg.max() == d - (k - 2)
        from oracle import cpu_vec
        u, _, _ = cpu_vec.edges(x, y, pick, m.box)
        deg0 = np.bincount(u[pick[u] == 0], minlength=len(x))[:counts[0]]
        assert set(range(2, 8)) <= set(deg0.tolist()) and (deg0 == 0).any()
        _pin(m, get_cc=True)   # the cluster is the largest component: same route


@pytest.mark.parametrize("name", sorted(lm.DENSE) + sorted(lm.DENSE_VEC))
def test_dense_shapes(name):
    m = lm.dense_mg(name)
    res = _pin(m)
    cap = lm.VEC_MAX_CLIQUES if name in lm.DENSE_VEC else lm.REF_MAX_CLIQUES
    assert len(res["members"]) <= cap
    assert m.d_max == int(name.split("_d")[1]) if "_d" in name else m.d_max == 65
    _pin(m, get_cc=True)
    if name == "k3_two_roots":   # two roots above the width, 1056 cliques each
        assert (np.bincount(res["members"][:, 0]) == 1056).sum() == 2


def test_dense_shape_sizes():
    n = {name: lm.dense_mg(name).n_cliques for name in list(lm.DENSE) + list(lm.DENSE_VEC)}
    # the clusters' cliques; the ordinary particles add fewer than two hundred
    for name, c in (("k3_d64", 1024), ("k3_d65", 1056), ("k4_d64", 9702), ("k4_d66", 10648),
                    ("k8_d64", 870), ("k8_d65", 900), ("k3_two_roots", 2112), ("k5_d65", 20992)):
        assert c <= n[name] < c + 200


@pytest.mark.parametrize("odd_level,odd_dfs", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_parity_batches(odd_level, odd_dfs):
    batch = lm.parity_batch(odd_level, odd_dfs)
    assert [m.route for m in batch] == ["dfs", "level", "dfs", "level", "level"]
    c = {"dfs": 0, "level": 0}
    for m in batch[:4]:
        res = _pin(m)
        c[m.route] += len(res["members"])
    assert (c["level"] % 2, c["dfs"] % 2) == (odd_level, odd_dfs) and min(c.values()) > 0
    d, res = lm.oracle_facts(batch[4])
    assert res["status"] == "no_cliques" and res["n_edges"] > 0 and d <= 7


def test_get_cc_decides_the_route():
    for k in (2, 3):
        m = lm.getcc_dfs_mg(k)
        _pin(m, 65)
        _pin(m, 65, get_cc=True)
    m = lm.getcc_level_mg()
    _pin(m, 65)
    res = _pin(m, 2, get_cc=True)    # the chain's roots only
    assert res["cc_max"] == 80 and len(res["members"]) == 79


def test_deferred_dfs_micrograph():
    m = lm.deferred_dfs_mg()
    assert m.n_boxes == 4700 > lm.FUSED_MAX_BOXES
    res = _pin(m, 65)
    assert len(res["members"]) <= lm.REF_MAX_CLIQUES


# ------------------------------------------------------------------------------ size edges
def _pin_size(model, n_boxes, get_cc=False):
    assert model.n_boxes == n_boxes
    d, res = lm.oracle_facts(model, get_cc)
    assert res["status"] == "ok" and 1 <= len(res["members"]) <= lm.VEC_MAX_CLIQUES
    assert d <= lm.RB_W   # the level route
    return res


@pytest.mark.parametrize("k,n", [(3, 65535), (3, 65536), (8, 65536)])
def test_wide_bin_micrographs(k, n):
    _pin_size(lm.wide_mg(k, n), n)
    assert (n > lm.BIN_U16_MAX) == (n == 65536)
    _pin_size(lm.small_mg(k), 900)
    if k == 8:   # the u32 variant's budget: 4095 cells per picker, saturated
        assert lm.bin_budget(n, True) // k == 4095 and 2 * n + 64 > 32760


@pytest.mark.parametrize("n", [32731, 32732])
def test_budget_saturation_micrographs(n):
    _pin_size(lm.budget_mg(n), n)
    assert (lm.bin_budget(n) == lm.BIN_BUDGET_CAP) == (n == 32732)
    assert lm.bin_budget(n) == min(2 * n + 64, 65528)


@pytest.mark.parametrize("n", [39936, 39937])
def test_union_find_batches(n):
    batch = lm.union_batch(n)
    assert (max(m.n_boxes for m in batch) > lm.UF_LDS_MAX) == (n == 39937)
    assert 1900 <= batch[1].n_boxes <= 2100
    for m, nb in zip(batch, (n, batch[1].n_boxes)):
        res = _pin_size(m, nb)
        assert res["cc_max"] == m.chain >= 1200     # the chain alone is the largest component
        sel = _pin_size(m, nb, get_cc=True)
        assert len(sel["members"]) == m.chain - 1   # --get_cc selects it: its edges (k = 2)


def test_fused_limit_batch():
    batch = lm.fused_limit_batch()
    assert [m.n_boxes for m in batch] == [4608, 4609, 900, 4700]
    assert [m.n_boxes > lm.FUSED_MAX_BOXES for m in batch] == [False, True, False, True]
    for m in batch:
        _pin_size(m, m.n_boxes)
    x = batch[3].mg[1][0]
    assert (x != np.rint(x)).all() and all((t[0] == np.rint(t[0])).all() for t in batch[1].mg)
