"""Inputs that sit on the routing and size edges of the large-micrograph route (rgc_kernels.hip,
rgc_cliques.hip, run_multi in rgc_run_large.cpp), shared by tests/test_large_route_models.py (which
pins every input on its edge with the oracle alone) and tests/test_gpu_large_route_edges.py.

The route a micrograph takes is not reported by the ABI; it is a pure function of the box
counts and of the edge list:

* a micrograph with a valid picker-0 root (forward edges, in the --get_cc component when that
  is on) of more than RB_W = 64 forward neighbours takes the thread-per-root DFS, every other
  the level route;
* a batch with a micrograph of more than 65535 boxes bins with u32 counters (key budget
  32760), every other with u16 pairs (key budget min(2 n + 64, 65528): saturated from
  n = 32732);
* a batch whose largest micrograph has more than 39936 boxes runs the global-memory
  union-find, every other the LDS one;
* a micrograph of more than 4608 boxes is deferred from the fused kernel.

Cluster inputs (part A): every box of a cluster lies within +-3 px of its centre on integer
coordinates (B = 100: JI >= 0.79), so the boxes of different pickers are pairwise adjacent,
a picker-0 box of the cluster has sum(sizes[1:]) forward neighbours and the cluster holds
prod(sizes) cliques.  Clusters, particles and lone boxes sit on a 400-px grid, so nothing else
is adjacent.  Synthetic inputs (part B): particles uniform in a square, every picker's box
jittered by +-6 px, integer coordinates, B = 64.
"""
import numpy as np

RB_W = 64
FUSED_MAX_BOXES = 4608
UF_LDS_MAX = 39936
BIN_U16_MAX = 65535
BIN_BUDGET_CAP = 65528
BOX_A, BOX_B = 100, 64
PITCH, COLS = 400, 40
CHAIN_STEP = {100: 40, 64: 26}   # 0.4 B: JI 0.43 between consecutive boxes, 0.11 two apart


def bin_budget(n, wide=False):
    """rgc_kernels.h bin_budget."""
    return min(2 * n + 64, 32760 if wide else BIN_BUDGET_CAP)


class Model:
    """One micrograph: ``mg`` = k (x, y, score) triples; what the builder intends: ``n_boxes``,
    ``n_cliques`` (None: not known in closed form), ``d_max`` (largest forward degree of a
    picker-0 box), ``chain`` (boxes of its chain)."""

    def __init__(self, mg, box, n_cliques, d_max, chain=0):
        self.mg, self.k, self.box = mg, len(mg), box
        self.n_boxes = sum(len(t[0]) for t in mg)
        self.n_cliques, self.d_max, self.chain = n_cliques, d_max, chain

    @property
    def route(self):
        return "dfs" if self.d_max > RB_W else "level"

    def flat(self):
        """(x, y, score, picker of each box, counts) in picker-major file order."""
        x, y, s = (np.concatenate([t[i] for t in self.mg]) for i in range(3))
        counts = [len(t[0]) for t in self.mg]
        return x, y, s, np.repeat(np.arange(self.k), counts), counts


def _slot(i):
    return 200 + PITCH * (i % COLS), 200 + PITCH * (i // COLS)


def cluster_mg(k, clusters, seed, n_sparse=24, n_single=0, n_lone=3, chain=0, complete=True,
               pad_to=0):
    """``clusters``: per-picker sizes of each cluster.  Besides them, ``n_sparse`` ordinary
    particles whose picker-0 box has 2..7 forward neighbours (with a clique wherever that
    covers every picker, unless ``complete`` is off: then no particle has a box of the last
    picker), ``n_single`` particles of one box per picker (one clique each), ``n_lone`` lone
    picker-0 boxes and one lone box per other picker, and for k = 2 a straight chain of
    ``chain`` boxes alternating picker 0 / 1 (chain - 1 cliques).  ``pad_to``: lone boxes of
    alternating pickers up to that box count."""
    rng = np.random.default_rng(seed)
    pk = [[] for _ in range(k)]
    slot, n_cl, d_max = 0, 0, 0

    def put(sizes):
        nonlocal slot
        cx, cy = _slot(slot)
        slot += 1
        for p, n in enumerate(sizes):
            for _ in range(n):
                pk[p].append((cx + int(rng.integers(-3, 4)), cy + int(rng.integers(-3, 4))))

    for sizes in clusters:
        assert len(sizes) == k and sizes[0] >= 1
        put(sizes)
        n_cl += int(np.prod(sizes, dtype=np.int64))
        d_max = max(d_max, sum(sizes[1:]))
    for j in range(n_sparse):
        t = 2 + j % 6
        sizes = [1] + [0] * (k - 1)
        last = k - 1 if complete else k - 2
        if last == 0:
            break
        if t >= last:
            for p in range(1, last + 1):
                sizes[p] = 1
            for i in range(t - last):
                sizes[1 + (j + i) % last] += 1
        else:
            for i in range(t):
                sizes[1 + (j + i) % last] = 1
        put(sizes)
        n_cl += int(np.prod(sizes, dtype=np.int64))
        d_max = max(d_max, t)
    for _ in range(n_single):
        put([1] * k)
        n_cl += 1
        d_max = max(d_max, k - 1)
    for _ in range(n_lone):
        put([1] + [0] * (k - 1))
    for p in range(1, k):
        put([0] * p + [1] + [0] * (k - 1 - p))
    n = sum(len(q) for q in pk) + chain
    for i in range(max(0, pad_to - n)):
        p = i % k
        put([0] * p + [1] + [0] * (k - 1 - p))
    if chain:
        assert k == 2
        y0 = _slot(slot + 3 * COLS)[1]
        for i in range(chain):
            pk[i % 2].append((200 + CHAIN_STEP[BOX_A] * i, y0))
        n_cl += chain - 1
        d_max = max(d_max, 2)
    mg = []
    for p in range(k):
        xy = np.array(pk[p], np.float64).reshape(-1, 2)
        mg.append((xy[:, 0].copy(), xy[:, 1].copy(), rng.uniform(0.3, 1.0, len(xy))))
    return Model(mg, BOX_A, n_cl, d_max, chain)


# ------------------------------------------------------------------------------ part A cases
def thin_shapes(k, d):
    """Clusters with a picker-0 root of d forward neighbours and d - (k - 2) cliques: the wide
    picker first (the DFS's depth 1) and, for k >= 3, last (its leaf)."""
    if k == 2:
        return [(1, d)]
    w = d - (k - 2)
    return [(1, w) + (1,) * (k - 2), (1,) * (k - 1) + (w,)]


def thin_batch(k):
    """Every thin shape of k at d = 63, 64, 65 as a micrograph of its own: DFS and level
    micrographs share the batch."""
    out = []
    for d in (63, 64, 65):
        for i, sizes in enumerate(thin_shapes(k, d)):
            out.append(cluster_mg(k, [sizes], seed=1000 * k + 10 * d + i))
    return out


# (k, sizes of the clusters): d = 64 / 65 pairs; (2, 32, 33): two DFS roots, consecutive ranges
DENSE = {
    "k3_d64": (3, [(1, 32, 32)]), "k3_d65": (3, [(1, 32, 33)]),
    "k4_d64": (4, [(1, 22, 21, 21)]), "k4_d66": (4, [(1, 22, 22, 22)]),
    "k8_d64": (8, [(1, 30, 29, 1, 1, 1, 1, 1)]), "k8_d65": (8, [(1, 30, 30, 1, 1, 1, 1, 1)]),
    "k3_two_roots": (3, [(2, 32, 33)]),
}
DENSE_VEC = {"k5_d65": (5, [(1, 8, 8, 8, 41)])}   # 20,992 cliques: vectorised oracle only
REF_MAX_CLIQUES, VEC_MAX_CLIQUES = 11000, 100000   # what bounds the oracles' time


def dense_mg(name):
    k, clusters = {**DENSE, **DENSE_VEC}[name]
    return cluster_mg(k, clusters, seed=sum(map(ord, name)))


def parity_batch(odd_level, odd_dfs):
    """k = 3 micrographs in the order DFS, level, DFS, level, one with edges and no clique;
    the level micrographs' cliques (C1) and the DFS ones' (C2) have the parities asked for
    (a particle of one clique goes to the first micrograph of a route where needed)."""
    def fit(shapes, seed, odd):
        for extra in (0, 1):
            ms = [cluster_mg(3, [shapes[0]], seed, n_single=extra),
                  cluster_mg(3, [shapes[1]], seed + 1)]
            if sum(m.n_cliques for m in ms) % 2 == int(odd):
                return ms
        raise AssertionError
    dfs = fit(thin_shapes(3, 65), 31, odd_dfs)
    lvl = fit(thin_shapes(3, 64), 41, odd_level)
    empty = cluster_mg(3, [], 51, complete=False)
    return [dfs[0], lvl[0], dfs[1], lvl[1], empty]


def getcc_dfs_mg(k):
    """The cluster with the d = 65 root is the largest component: with --get_cc the DFS runs
    with the target filter."""
    return cluster_mg(k, [thin_shapes(k, 65)[0] if k == 2 else (1, 32, 33)], seed=61 + k)


def getcc_level_mg():
    """k = 2: a chain of 80 boxes is the largest component (the cluster has 66), so with
    --get_cc the d = 65 root is not valid and the micrograph takes the level route."""
    return cluster_mg(2, [(1, 65)], seed=71, chain=80)


def deferred_dfs_mg():
    """4700 boxes (above the fused kernel's 4608) with one (1, 32, 33) cluster."""
    return cluster_mg(3, [(1, 32, 33)], seed=81, n_sparse=48, pad_to=4700)


# ------------------------------------------------------------------------------ part B cases
def _chain_path(n, step, x0, y0, row):
    """Serpentine path of n points ``step`` apart: rows of ``row`` points joined by 6 vertical
    steps (rows 6 steps apart: 2.4 B, no overlap)."""
    pts, x, y, dx = [], x0, y0, step
    while len(pts) < n:
        for _ in range(row):
            pts.append((x, y))
            x += dx
        x -= dx
        for _ in range(5):
            y += step
            pts.append((x, y))
        y += step
        dx = -dx
    return pts[:n]


def synth_mg(k, n_boxes, n_true, seed, side=16000, chain=0, frac_picker=None):
    """``n_true`` particle centres uniform in a ``side``-px square, each picker's box jittered
    by +-6 px, integer coordinates; filler boxes bring the last picker to ``n_boxes`` in all;
    k = 2: a serpentine chain of ``chain`` boxes alternating picker 0 / 1 below the square
    (the largest component).  ``frac_picker``: that picker's x shifted by 0.5."""
    rng = np.random.default_rng(seed)
    cx = rng.integers(0, side, n_true)
    cy = rng.integers(0, side, n_true)
    fill = n_boxes - k * n_true - chain
    assert fill >= 0
    path = _chain_path(chain, CHAIN_STEP[BOX_B], 0, side + 500, 400) if chain else []
    assert not chain or k == 2
    mg = []
    for p in range(k):
        x = cx + rng.integers(-6, 7, n_true)
        y = cy + rng.integers(-6, 7, n_true)
        if p == k - 1 and fill:
            x = np.concatenate([x, rng.integers(0, side, fill)])
            y = np.concatenate([y, rng.integers(0, side, fill)])
        if chain:
            q = np.array(path[p::2], np.int64).reshape(-1, 2)
            x, y = np.concatenate([x, q[:, 0]]), np.concatenate([y, q[:, 1]])
        x, y = x.astype(np.float64), y.astype(np.float64)
        if frac_picker == p:
            x = x + 0.5
        mg.append((x, y, rng.uniform(0.3, 1.0, len(x))))
    return Model(mg, BOX_B, None, None, chain)


def small_mg(k, seed=5):
    """The 900-box companion of the wide batches."""
    return synth_mg(k, 900, 290 if k == 3 else 900 // k - 10, seed, side=4000)


def wide_mg(k, n_boxes):
    """65535 / 65536 boxes: one over switches the whole batch to k1_bin's u32 counters."""
    return synth_mg(k, n_boxes, n_boxes // k - 5, seed=100 + k)


def budget_mg(n_boxes):
    """k = 2; 2 n + 64 reaches the key budget's cap 65528 at n = 32732."""
    return synth_mg(2, n_boxes, n_boxes // 2 - 7, seed=200)


def union_batch(n_boxes):
    """k = 2: a micrograph of ``n_boxes`` (39936: LDS union-find; 39937: global memory) and one
    of about 2000, each with a serpentine chain as its largest component."""
    return [synth_mg(2, n_boxes, (n_boxes - 3001) // 2 - 3, seed=300, chain=3001),
            synth_mg(2, 2003, 400, seed=301, side=5000, chain=1200)]


def fused_limit_batch():
    """k = 3: 4608 boxes (the fused kernel's last size), 4609 (deferred), 900, and 4700 with
    fractional x in picker 1 (deferred, f64 epilogue): the deferred set is {1, 3}."""
    return [synth_mg(3, 4608, 1530, seed=400, side=5000),
            synth_mg(3, 4609, 1530, seed=401, side=5000),
            synth_mg(3, 900, 290, seed=402, side=2500),
            synth_mg(3, 4700, 1560, seed=403, side=5000, frac_picker=1)]


# ------------------------------------------------------------------------------ oracle facts
def oracle_facts(model, get_cc=False):
    """From the oracle alone: the forward degree of every picker-0 box (edges (u, v) per u),
    with ``get_cc`` of those in the component the oracle selects only; and the oracle's
    result.  -> (largest forward degree, result dict)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    from oracle import cpu_vec
    x, y, s, pick, counts = model.flat()
    u, v, _ = cpu_vec.edges(x, y, pick, model.box)
    n = len(x)
    deg = np.bincount(u[pick[u] == 0], minlength=n)
    res = cpu_vec.micrograph(x, y, s, counts, model.box, get_cc=get_cc)
    if get_cc:
        _, lab = connected_components(coo_matrix((np.ones(len(u)), (u, v)), shape=(n, n)),
                                      directed=False)
        nodes = np.unique(np.concatenate([u, v]))
        size = np.bincount(lab[nodes], minlength=lab.max() + 1)
        big = np.nonzero(size == size.max())[0]
        assert len(big) == 1, "the largest component must be unique (no tie-break here)"
        if res["status"] == "ok":   # the oracle's selection is that component
            assert (lab[res["members"]] == big[0]).all()
        deg = np.where(lab == big[0], deg, 0)
    return int(deg.max()), res
