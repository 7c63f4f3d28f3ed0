"""Set-packing models that put a conflict component on the sizes and inputs at which the device
solver (rgc_ilp.hip) changes behaviour.  Shared by tests/test_ilp_search_model.py (CPU),
tests/test_gpu_ilp_edges.py (GPU) and tests/golden/make_ilp_golden.py (their HiGHS optima).

Every generator is seeded, draws f32 weights and returns (A, w): A a scipy COO matrix (boxes x
columns) whose columns form ONE conflict component unless ``ragged`` is set.
"""
from __future__ import annotations

import itertools
import zlib

import numpy as np
from scipy.sparse import coo_matrix

UNIFORM, TIED = "uniform", "tied"


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def draw_weights(n, mode, rng, zero_frac=0.0):
    """uniform: f32 in [0.1, 1]; tied: from {0.25, 0.5, 0.75}; zero_frac: that share set to 0."""
    if mode == UNIFORM:
        w = rng.uniform(0.1, 1.0, n).astype(np.float32)
    elif mode == TIED:
        w = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), n)
    else:
        raise ValueError(mode)
    if zero_frac > 0.0:
        w[rng.random(n) < zero_frac] = 0.0
    return w


def _matrix(cols, n_rows, ragged_rng=None):
    """COO matrix of a list of row tuples; with ragged_rng about a third of the columns lose
    one or two of their rows (never the last one left)."""
    if ragged_rng is not None:
        out = []
        for c in cols:
            c = list(c)
            if ragged_rng.random() < 1 / 3:
                for _ in range(int(ragged_rng.integers(1, 3))):
                    if len(c) > 1:
                        c.pop(int(ragged_rng.integers(len(c))))
            out.append(tuple(c))
        cols = out
    ri = np.fromiter(itertools.chain.from_iterable(cols), np.int64)
    ci = np.repeat(np.arange(len(cols)), [len(c) for c in cols])
    return coo_matrix((np.ones(len(ri), np.int64), (ri, ci)), shape=(n_rows, len(cols)))


def _cluster_cols(per_sizes, row0):
    """Every combination of one box per picker: prod(per_sizes) columns on sum(per_sizes)
    boxes numbered from row0.  Returns (columns, boxes per picker)."""
    boxes, r = [], row0
    for p in per_sizes:
        boxes.append(list(range(r, r + p)))
        r += p
    return list(itertools.product(*boxes)), boxes


def cluster(per_sizes, n_pendant=0, weights=UNIFORM, seed=0, zero_frac=0.0, ragged=False,
            subset=None):
    """A whole dense cluster (per_sizes[p] near-duplicate boxes of picker p) plus n_pendant
    pendant columns (one cluster box, k - 1 private boxes).  subset: keep only that many of the
    cluster's columns, drawn at random (a partial cluster)."""
    k = len(per_sizes)
    rng = _rng("cluster", tuple(per_sizes), n_pendant, weights, seed, zero_frac, ragged, subset)
    cols, boxes = _cluster_cols(per_sizes, 0)
    if subset is not None:
        keep = np.sort(rng.choice(len(cols), subset, replace=False))
        cols = [cols[i] for i in keep]
    r = sum(per_sizes)
    for i in range(n_pendant):
        p = i % k
        hub = boxes[p][(i // k) % per_sizes[p]]
        priv = list(range(r, r + k - 1))
        r += k - 1
        cols.append(tuple(priv[:p] + [hub] + priv[p:]))
    w = draw_weights(len(cols), weights, rng, zero_frac)
    return _matrix(cols, r, rng if ragged else None), w


def chain(n, k, stride=1, weights=UNIFORM, seed=0):
    """Column j covers boxes j * stride .. j * stride + k - 1."""
    rng = _rng("chain", n, k, stride, weights, seed)
    cols = [tuple(range(j * stride, j * stride + k)) for j in range(n)]
    return _matrix(cols, (n - 1) * stride + k), draw_weights(n, weights, rng)


def chain_optimum(w, k, stride=1):
    """Exact optimum of chain(n, k, stride): columns j < j' conflict iff (j' - j) * stride < k,
    so a packing is a set of columns at least d = ceil(k / stride) apart."""
    w = np.asarray(w, np.float64)
    d = -(-k // stride)
    best = [0.0] * (len(w) + 1)   # best[j]: optimum over the first j columns
    for j in range(len(w)):
        best[j + 1] = max(best[j], float(w[j]) + best[max(j + 1 - d, 0)])
    return best[-1]


def hubbed_chain(n_chain, n_pendant, weights=UNIFORM, seed=0):
    """chain(n_chain, 3) plus n_pendant pendant columns that all hold the chain's first box
    (and two private boxes each), so at most one of them fits a packing."""
    rng = _rng("hubbed_chain", n_chain, n_pendant, weights, seed)
    cols = [tuple(range(j, j + 3)) for j in range(n_chain)]
    r = n_chain + 2
    for _ in range(n_pendant):
        cols.append((0, r, r + 1))
        r += 2
    return _matrix(cols, r), draw_weights(len(cols), weights, rng)


def bridged(per_sizes, n_clusters, weights=UNIFORM, seed=0):
    """n_clusters dense clusters in a row, neighbours joined by one bridge column (one box of
    each, k - 2 private boxes)."""
    k = len(per_sizes)
    assert k >= 2
    rng = _rng("bridged", tuple(per_sizes), n_clusters, weights, seed)
    cols, firsts, r = [], [], 0
    for _ in range(n_clusters):
        cc, boxes = _cluster_cols(per_sizes, r)
        cols += cc
        firsts.append((boxes[0][0], boxes[-1][-1]))
        r += sum(per_sizes)
    for q in range(n_clusters - 1):
        priv = list(range(r, r + k - 2))
        r += k - 2
        cols.append(tuple([firsts[q][1], firsts[q + 1][0]] + priv))
    return _matrix(cols, r), draw_weights(len(cols), weights, rng)


# ------------------------------------------------------------------------------ the test models
# Tier A ("must prove"): name -> (per_sizes, pendants).  One model per size at which the solver
# takes another path, each in both weight modes:
#   1 (shortcut), 2 (smallest searched), 63 / 64 / 65 (thread solver's full mask; first wave
#   component, W = 2), 127 / 128 / 129 (last-word mask of the wave solver), 256, 1024 / 1025
#   (node budget scaled by 16 / W above), 2048 / 2049 at K = 7 and 3276 / 3277 at K = 4 (row
#   info in LDS or in global scratch: n (K + 1) <= 16384), 4096 (largest searched).
# Row counts 2, 3, 5 and 8 all occur, so a batch of all of them has kmax = 8.
_CHAIN_K, _CHAIN_STRIDE = 3, 1
TIER_A_SHAPES = {
    "n1": ((1, 1, 1), 0),
    "n2": ((2, 1), 0),
    "n63": ((7, 3, 3), 0),
    "n64": ((4, 4, 4), 0),
    "n64k8": ((2, 2, 2, 2, 2, 2, 1, 1), 0),
    "n65": ((4, 4, 4), 1),
    "n127": ((5, 5, 5), 2),
    "n128": ((2, 2, 2, 2, 8), 0),
    "n129": ((4, 4, 8), 1),
    "n256": ((4, 4, 4, 4), 0),
    "n1024": ((4, 4, 4, 4, 4), 0),
    "n1025": ((4, 4, 4, 4, 4), 1),
    "n2048k7": ((4, 4, 4, 4, 2, 2, 2), 0),
    "n2049k7": ((4, 4, 4, 4, 2, 2, 2), 1),
    "n3276k4": ((4, 9, 7, 13), 0),
    "n3277k4": ((4, 9, 7, 13), 1),
    "n4096": ((4, 4, 4, 4, 4, 4), 0),
}
TIER_A_SIZES = {"n1": 1, "n2": 2, "n63": 63, "n64": 64, "n64k8": 64, "n65": 65, "n127": 127,
                "n128": 128, "n129": 129, "n256": 256, "n1024": 1024, "n1025": 1025,
                "n2048k7": 2048, "n2049k7": 2049, "n3276k4": 3276, "n3277k4": 3277,
                "n4096": 4096}
TIER_A = [f"{name}-{mode}" for name in TIER_A_SHAPES for mode in (UNIFORM, TIED)]
# Two short chains with tied weights, which the thread solver proves in under 1,000 nodes: the
# cover bound is loose on chains, so the search reaches further leaves of the optimal value
# and the result depends on the incumbent being replaced only by a strictly greater one (no
# cluster model above notices that rule).
TIER_A_CHAINS = {"chain28": 28, "chain32": 32}
TIER_A_SIZES.update(TIER_A_CHAINS)
TIER_A += [f"{name}-{TIED}" for name in TIER_A_CHAINS]
# The same for the wavefront solver: a 28-column tied chain with 37 pendants on its first box,
# 65 columns (W = 2) proven in about 7,000 nodes (the seed is one at which the restatement
# with a ">=" incumbent returns another packing).
TIER_A_SIZES["hub65"] = 65
TIER_A.append(f"hub65-{TIED}")

# Tier B ("honest status"): models the cover bound does not finish: name -> (builder, chain
# parameters (k, stride) or None, node_limit).
TIER_B_SPECS = {}
for _n in (64, 65, 128):
    for _mode in (UNIFORM, TIED):
        TIER_B_SPECS[f"chain{_n}-{_mode}"] = (
            lambda n=_n, mode=_mode: chain(n, _CHAIN_K, _CHAIN_STRIDE, mode), True, 0)
TIER_B_SPECS["bridged1027"] = (lambda: bridged((4, 4, 4, 4), 4, UNIFORM), False, 0)
TIER_B_SPECS["partial4097"] = (lambda: cluster((5, 5, 5, 5, 5, 2), 0, UNIFORM, subset=4097),
                               False, 0)
TIER_B_SPECS["chain4097"] = (lambda: chain(4097, _CHAIN_K, _CHAIN_STRIDE, UNIFORM), True, 0)
TIER_B_SPECS["chain64-limit64"] = (lambda: chain(64, _CHAIN_K, _CHAIN_STRIDE, UNIFORM), True, 64)
TIER_B = list(TIER_B_SPECS)

_CACHE = {}


def model(name):
    """(A, w) of a Tier A or Tier B model, built once per process."""
    if name not in _CACHE:
        if name in TIER_B_SPECS:
            _CACHE[name] = TIER_B_SPECS[name][0]()
        else:
            shape, mode = name.rsplit("-", 1)
            if shape == "hub65":
                _CACHE[name] = hubbed_chain(28, 37, mode, seed=8)
            elif shape in TIER_A_CHAINS:
                _CACHE[name] = chain(TIER_A_CHAINS[shape], _CHAIN_K, _CHAIN_STRIDE, mode)
            else:
                per, pend = TIER_A_SHAPES[shape]
                _CACHE[name] = cluster(per, pend, mode)
    return _CACHE[name]


def node_limit(name):
    """The node_limit a model is solved with (0: the library default)."""
    return TIER_B_SPECS[name][2] if name in TIER_B_SPECS else 0


def chain_reference(name):
    """The DP optimum of a chain model, None for the other models."""
    if (TIER_B_SPECS[name][1] if name in TIER_B_SPECS
            else name.rsplit("-", 1)[0] in TIER_A_CHAINS):
        return chain_optimum(model(name)[1], _CHAIN_K, _CHAIN_STRIDE)
    return None


def ragged_models():
    """Clusters of at most 129 columns with 1..8 rows per column, both weight modes."""
    return [cluster(per, pend, mode, ragged=True)
            for per, pend in (((4, 4, 4), 1), ((2, 2, 2, 2, 2, 2, 1, 1), 0), ((5, 5, 5), 2),
                              ((4, 4, 8), 1))
            for mode in (UNIFORM, TIED)]


def zero_weight_models():
    """Clusters in which about 30 % of the columns weigh exactly 0 and share boxes with the
    positive ones."""
    return [cluster(per, pend, mode, zero_frac=0.3)
            for per, pend in (((4, 4, 4), 0), ((4, 4, 4), 1), ((4, 4, 8), 1))
            for mode in (UNIFORM, TIED)]


def fixture_models():
    """The models whose HiGHS optimum is committed (make_ilp_golden.py): all above 200 columns,
    so neither the CPU nor the GPU tests wait on a live MILP of any size that takes HiGHS more
    than milliseconds (tests/test_ilp.py LIVE_MAX_COLS only bounds what MAY be solved live)."""
    return [n for n in TIER_A + TIER_B if model(n)[0].shape[1] > 200]
