"""The large-micrograph route (rgc_kernels.hip, rgc_cliques.hip, run_multi in rgc_run_large.cpp)
at the sizes and degrees where it selects another path, both sides of each:

* a valid picker-0 root of more than RB_W = 64 forward neighbours sends its micrograph to the
  thread-per-root DFS (k5_cliques<K, FILL>, K = 2..8), whose cliques follow the level route's
  (dfs_base = C1; without members k5_epilogue starts at epi_lo = C1); exactly 64 is the level
  route's full-width bitmap;
* a micrograph of more than 65535 boxes switches its batch to k1_bin<true>; 2 n + 64 reaches
  the key budget's cap at n = 32732; a batch whose largest micrograph has more than 39936
  boxes runs the global-memory union-find; more than 4608 boxes defers a micrograph from the
  fused kernel (k_gather / k_remap).

The route is not observable: tests/test_large_route_models.py pins every input used here on
its edge with the oracle alone.  Every device output is compared bit for bit with the oracle
(_check_vs_oracle: oracle/cpu_ref.py; _check_vs_vec: oracle/cpu_vec.py, members on and off).
"""
import numpy as np
import pytest

import large_route_models as lm
from test_gpu_parity import _check_vs_oracle, _check_vs_vec, _dense_clusters

pytestmark = pytest.mark.gpu


def _mgs(models):
    return [m.mg for m in models]


def _device(mgs, k, box, id_bases=None, **kw):
    """One run; per micrograph every output in the canonical order of its rows (a clique's
    sorted vertex ranks), box indices local to the micrograph."""
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    batch = Batch.pack(k, box, mgs, id_bases=id_bases)
    ctx = _lib.Context(0)
    res = run_batch(ctx, batch, **kw)
    ctx.close()
    out = []
    for m, r in enumerate(res):
        b0 = int(batch.box_off[m * k])
        p = np.lexsort(r.rows.T[::-1]) if len(r.rows) else np.zeros(0, int)
        out.append(dict(stat=(r.status, r.cc_max, r.cc_cnt, r.n_vert, r.n_edges),
                        rows=r.rows[p], w=r.w[p].view(np.uint32),
                        conf=r.conf[p].view(np.uint32), consensus=r.consensus[p] - b0,
                        members=None if r.members is None else r.members[p] - b0))
    return out, batch


def _same(a, b):
    assert a["stat"] == b["stat"]
    for f in ("rows", "w", "conf", "consensus", "members"):
        assert (a[f] is None) == (b[f] is None), f
        assert a[f] is None or np.array_equal(a[f], b[f]), f


# ------------------------------------------------------------------- A. DFS route, 64 neighbours
@pytest.mark.parametrize("k", range(2, 9))
def test_gpu_thin_shapes_both_sides_of_the_bitmap_width(k):
    """(1, d) for k = 2; the wide picker first and last for k >= 3; d = 63, 64, 65, a
    micrograph each in one batch: DFS and level micrographs together, C1 and C2 non-zero."""
    mgs = _mgs(lm.thin_batch(k))
    _check_vs_oracle(mgs, k, lm.BOX_A, no_fused=True)
    _check_vs_oracle(mgs, k, lm.BOX_A, no_fused=True, get_cc=True)


@pytest.mark.parametrize("names", [("k3_d64", "k3_d65"), ("k4_d64", "k4_d66"),
                                   ("k8_d64", "k8_d65"), ("k3_two_roots", "k3_d64")])
def test_gpu_dense_shapes_against_reference_oracle(names):
    models = [lm.dense_mg(n) for n in names]
    _check_vs_oracle(_mgs(models), models[0].k, lm.BOX_A, no_fused=True)


@pytest.mark.parametrize("names", [("k3_d64", "k3_d65", "k3_two_roots"), ("k4_d64", "k4_d66"),
                                   ("k8_d64", "k8_d65"), ("k5_d65",)])
def test_gpu_dense_shapes_against_vectorised_oracle(names):
    """Members on and off (k5_leaf_epi for the level cliques, k5_epilogue from epi_lo = C1 for
    the DFS ones), --get_cc off and on."""
    models = [lm.dense_mg(n) for n in names]
    for get_cc in (False, True):
        n = _check_vs_vec(_mgs(models), models[0].k, lm.BOX_A, get_cc=get_cc, no_fused=True)
        assert get_cc or n == sum(m.n_cliques for m in models)


@pytest.mark.parametrize("odd_level,odd_dfs", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_gpu_output_placement_by_parity_and_order(odd_level, odd_dfs):
    """Micrographs DFS, level, DFS, level, one with edges and no clique, the level cliques (C1)
    and the DFS cliques (C2) of each parity; then the micrographs reversed (ids kept): every
    micrograph's outputs equal its own from the first order."""
    models = lm.parity_batch(odd_level, odd_dfs)
    mgs, k, box = _mgs(models), 3, lm.BOX_A
    _check_vs_vec(mgs, k, box, no_fused=True, allow_empty=True)
    for members in (True, False):
        fwd, batch = _device(mgs, k, box, no_fused=True, members=members)
        c = {"dfs": 0, "level": 0}
        for m, f in zip(models, fwd):
            c[m.route] += len(f["w"])
        assert (c["level"] % 2, c["dfs"] % 2) == (odd_level, odd_dfs)
        rev, _ = _device(mgs[::-1], k, box, id_bases=batch.id_base[::-1].copy(), no_fused=True,
                         members=members)
        for a, b in zip(fwd, rev[::-1]):
            _same(a, b)


def test_gpu_get_cc_decides_the_route():
    """(a) the d = 65 cluster is the largest component: the DFS with the target filter;
    (b) k = 2, a chain of 80 boxes is: the d = 65 root is not valid, the micrograph takes the
    level route and k5n_build skips that root."""
    for k in (2, 3):
        mgs = _mgs([lm.getcc_dfs_mg(k), lm.thin_batch(k)[0]])
        _check_vs_oracle(mgs, k, lm.BOX_A, no_fused=True, get_cc=True)
    mgs = _mgs([lm.getcc_level_mg(), lm.thin_batch(2)[2]])
    _check_vs_oracle(mgs, 2, lm.BOX_A, no_fused=True, get_cc=True)
    _check_vs_oracle(mgs, 2, lm.BOX_A, no_fused=True)


@pytest.mark.parametrize("names", [("k3_d64", "k3_d65"), ("k4_d64", "k4_d66")])
def test_gpu_multi_out_dfs_and_level(names):
    """--multi_out turns the fused leaf epilogue off: k5_leaf_fill and the DFS fill in one
    run, and every clique's node order from the exact pass."""
    models = [lm.dense_mg(n) for n in names]
    _check_vs_oracle(_mgs(models), models[0].k, lm.BOX_A, no_fused=True, multi_out=True)


def test_gpu_deferred_micrograph_reaches_the_dfs():
    """Default route: 4700 boxes with a (1, 32, 33) cluster are deferred from the fused kernel
    (between two micrographs that are not: k_gather / k_remap) and take the DFS."""
    mgs = [_dense_clusters(3, 4, 5, seed=1), lm.deferred_dfs_mg().mg, lm.thin_batch(3)[0].mg]
    _check_vs_oracle(mgs, 3, lm.BOX_A)
    _check_vs_oracle(mgs, 3, lm.BOX_A, get_cc=True)


# ------------------------------------------------------------------------------ B. size edges
def _vec_both(models, **kw):
    for get_cc in (False, True):
        _check_vs_vec(_mgs(models), models[0].k, lm.BOX_B, get_cc=get_cc, no_fused=True, **kw)


@pytest.mark.parametrize("k,n", [(3, 65535), (3, 65536), (8, 65536)])
def test_gpu_wide_bin(k, n):
    """65536 boxes switch the batch (the 900-box micrograph too) to k1_bin's u32 counters and
    the 32760-key budget; 65535 is the u16 counters' largest micrograph."""
    _vec_both([lm.wide_mg(k, n), lm.small_mg(k)])


def test_gpu_wide_bin_small_micrograph_unchanged():
    """The 900-box micrograph's outputs are the same beside 65535 and beside 65536 boxes."""
    small = lm.small_mg(3)
    got = []
    for n in (65535, 65536):
        big = lm.wide_mg(3, n)
        # the small micrograph first: its ids (the consensus tie-break) are the same
        f, _ = _device([small.mg, big.mg], 3, lm.BOX_B, no_fused=True, members=True)
        got.append(f[0])
    assert len(got[0]["w"]) > 200
    _same(got[0], got[1])


@pytest.mark.parametrize("n", [32731, 32732])
def test_gpu_bin_budget_saturation(n):
    _vec_both([lm.budget_mg(n)])


@pytest.mark.parametrize("n", [39936, 39937])
def test_gpu_union_find_lds_limit(n):
    """Each micrograph's largest component is a serpentine chain of thousands of boxes (path
    compression; --get_cc selects it: k4_target).  The unions and the walks over their trees
    run concurrently, so the --get_cc run is repeated: every run gives the same outputs."""
    models = lm.union_batch(n)
    _vec_both(models)
    runs = [_device(_mgs(models), 2, lm.BOX_B, get_cc=True, no_fused=True, members=True)[0]
            for _ in range(4)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            _same(a, b)


def test_gpu_fused_limit_and_deferral():
    """[4608, 4609, 900, 4700 with fractional x] on the default route: the deferred set is
    {1, 3} (not the identity) and one deferred micrograph takes the f64 epilogue; then all four
    on the multi-kernel route: every micrograph's outputs equal the default route's."""
    models = lm.fused_limit_batch()
    mgs = _mgs(models)
    for get_cc in (False, True):
        _check_vs_vec(mgs, 3, lm.BOX_B, get_cc=get_cc)
        for members in (True, False):
            a, _ = _device(mgs, 3, lm.BOX_B, get_cc=get_cc, members=members)
            b, _ = _device(mgs, 3, lm.BOX_B, get_cc=get_cc, members=members, no_fused=True)
            for u, v in zip(a, b):
                _same(u, v)
