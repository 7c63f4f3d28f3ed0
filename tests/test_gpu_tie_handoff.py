"""Near-ties leave the fused kernel by clique slot: a clique whose f32 weighted degrees cannot
decide the consensus (and every clique under --multi_out) is written to its micrograph's own
segment of the tie list, counted per micrograph, and decided exactly by k_fused_ties.

Every case is held to the CPU oracle through the parity tests' helpers, and goes through both
rgc_run and rgc_submit / rgc_wait on HBM-resident inputs (twice: the second submission of a
batch with fractional micrographs runs their f64 pass on the device), which must agree byte
for byte per micrograph.  The shapes are the smallest at which the hand-off can go wrong: full
segments (every clique an exact tie), empty ones beside them, the in-kernel insertion-order
path of a graph with 2 K >= nodes, two fused passes in one run, counts left over on a reused
context, and a micrograph whose epilogue runs in several chunks.
"""
import itertools

import numpy as np
import pytest

from test_gpu_ji_threshold import _Hip
from test_gpu_parity import _canon, _dense_clusters, _oracle_mg

pytestmark = pytest.mark.gpu

BOX = 100


# ----------------------------------------------------------------------------- inputs
def _lattice(k, nx=5, ny=5, step=300, offs=None, frac=False, seed=0):
    """nx x ny sites, one box of every picker per site; picker p sits at the site + offs[p]
    (default: all on the site itself, so all JIs are 1 and every clique is a k-way exact tie).
    frac: quarter-pixel coordinates (not integers: the f64 layout)."""
    rng = np.random.default_rng(seed)
    sx, sy = np.meshgrid(np.arange(nx) * step + 200.0, np.arange(ny) * step + 200.0)
    sx, sy = sx.ravel(), sy.ravel()
    offs = offs if offs is not None else [0] * k
    mg = []
    for p in range(k):
        o = rng.permutation(len(sx))          # file order differs from picker to picker
        x = sx[o] + offs[p] + (0.25 if frac else 0.0)
        y = sy[o] + (0.75 if frac else 0.0)
        mg.append((x, y, rng.uniform(0.3, 1.0, len(x))))
    return mg


def _no_ties(k, **kw):
    """the lattice with every picker at its own x offset (0, 3, 7, 12): the middle pickers'
    degrees are the largest by > 1e-2, no clique comes near a tie"""
    return _lattice(k, offs=[0, 3, 7, 12][:k], **kw)


def _no_cliques(k):
    """edges between pickers 0 and 1 only: a graph, but no k-clique"""
    mg = _lattice(k, nx=2, ny=2)
    mg[k - 1] = tuple(np.asarray(v) + (5000.0 if i < 2 else 0.0) for i, v in enumerate(mg[k - 1]))
    if k == 4:
        mg[2] = tuple(np.asarray(v) + (9000.0 if i < 2 else 0.0) for i, v in enumerate(mg[2]))
    return mg


def _ji(xa, ya, xb, yb, B):
    xo = max((min(xa, xb) + B) - max(xa, xb), 0.0)
    yo = max((min(ya, yb) + B) - max(ya, yb), 0.0)
    inter = xo * yo
    return inter / (2.0 * B * B - inter)


def _oracle_ties(mg, o, k, box=BOX):
    """Per oracle clique (column of its constraint matrix): the picker-0 member's file index and
    whether its largest f64 weighted degree (reference op order) is shared.  Every box of these
    inputs is a clique vertex, so row r of the matrix is the r-th box by (x, y, id)."""
    boxes = []
    for p, (x, y, _) in enumerate(mg):
        boxes += [(float(a), float(b), p, i) for i, (a, b) in enumerate(zip(x, y))]
    # ids grow with (picker, file index), so sorting by (x, y, picker, index) is the row order
    boxes.sort()
    A = o["A"].tocoo()
    assert A.shape[0] == len(boxes)
    C = A.shape[1]
    rows = A.row[np.argsort(A.col, kind="stable")].reshape(C, k)
    out = []
    for cl in rows:
        mem = sorted((boxes[r] for r in cl), key=lambda t: t[2])
        assert [t[2] for t in mem] == list(range(k))
        deg = []
        for i in range(k):
            d = 0.0
            for q in range(k):
                if q != i:
                    d = d + _ji(mem[i][0], mem[i][1], mem[q][0], mem[q][1], float(box))
            deg.append(d)
        out.append((mem[0][3], sorted(deg)[-1] == sorted(deg)[-2]))
    return out


# ----------------------------------------------------------------------------- both paths
def _snap_run(r, n_mg, k, multi):
    out = []
    for m in range(n_mg):
        c0 = int(r.clique_base[m])
        c1 = c0 + int(r.clique_cnt[m])
        d = {"stat": (int(r.status[m]), int(r.cc_max[m]), int(r.cc_cnt[m]), int(r.n_vert[m]),
                      int(r.n_edges_mg[m]), c1 - c0)}
        for f in ("rows", "w", "conf", "consensus", "members") + (("order",) if multi else ()):
            d[f] = np.array(getattr(r, f)[c0:c1])
        out.append(d)
    return out


def _snap_dev(hip, r, n_mg, k, multi):
    C = int(r.n_cliques)
    spec = [("rows", np.int32, k), ("w", np.float32, 1), ("conf", np.float32, 1),
            ("consensus", np.int32, 1), ("members", np.int32, k)]
    if multi:
        spec.append(("order", np.uint8, k))
    arr = {}
    for f, dt, w in spec:
        v = hip.down(getattr(r, f), C * w, dt)
        arr[f] = v.reshape(C, w) if w > 1 else v
    out = []
    for m in range(n_mg):
        c0 = int(r.clique_base[m])
        c1 = c0 + int(r.clique_cnt[m])
        d = {"stat": (int(r.status[m]), int(r.cc_max[m]), int(r.cc_cnt[m]), int(r.n_vert[m]),
                      int(r.n_edges_mg[m]), c1 - c0)}
        for f, _, _ in spec:
            d[f] = arr[f][c0:c1].copy()
        out.append(d)
    return out


def _same(a, b, what):
    assert len(a) == len(b)
    for m, (u, v) in enumerate(zip(a, b)):
        assert u["stat"] == v["stat"], (what, m, u["stat"], v["stat"])
        for f in u:
            if f != "stat":
                assert u[f].tobytes() == v[f].tobytes(), (what, m, f)


def _oracles(mgs, k, get_cc, multi):
    from oracle import cpu_ref
    methods = [f"picker{p}" for p in range(k)]
    out, idb = [], 0
    for mg in mgs:
        try:
            out.append(_oracle_mg(mg, BOX, methods, idb, get_cc, multi))
        except cpu_ref.NoCliques:
            out.append(None)
        idb += sum(len(t[0]) for t in mg)
    return out


def _check(ctx, hip, mgs, k, oracles, get_cc=False, multi=False):
    """rgc_run against the oracle (as test_gpu_parity._check_vs_oracle compares), then two
    submit / wait rounds on device inputs against rgc_run, byte for byte."""
    from repic_amd import _lib
    from repic_amd.pipeline import Batch
    batch = Batch.pack(k, BOX, mgs)
    n_mg = batch.n_mg
    fl = _lib.F_MEMBERS | (_lib.F_GET_CC if get_cc else 0) | (_lib.F_MULTI_OUT if multi else 0)
    r = ctx.run(n_mg, k, BOX, batch.box_off, batch.id_base, batch.x, batch.y, batch.score,
                fl | _lib.F_HOST_OUTPUTS)
    run = _snap_run(r, n_mg, k, multi)
    for m, (mg, o) in enumerate(zip(mgs, oracles)):
        g = run[m]
        if o is None:
            assert g["stat"][0] == _lib.NO_CLIQUES and g["stat"][5] == 0
            continue
        assert g["stat"][0] == _lib.OK
        assert (g["stat"][1], g["stat"][2]) == (o["cc_max"], o["cc_cnt"])
        A = o["A"].tocoo()
        C = A.shape[1]
        orows = np.sort(A.row[np.argsort(A.col, kind="stable")].reshape(C, k), axis=1)
        assert g["stat"][3] == A.shape[0] and g["stat"][5] == C
        idb = int(batch.id_base[m]) - int(batch.box_off[m * k])

        def tup(b):
            return (float(batch.x[b]), float(batch.y[b]), idb + int(b))
        gcons, ocons = [tup(b) for b in g["consensus"]], o["consensus"]
        if multi:
            ocons = [list(row) for row in ocons[1:1 + C]]
            gcons = [[tup(mem[p]) for p in od if p != k - 1] + [tup(mem[k - 1])]
                     for mem, od in zip(g["members"].tolist(), g["order"].tolist())]
        a = _canon(orows, o["w"], o["conf"], ocons)
        b = _canon(g["rows"], g["w"], g["conf"], gcons)
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert a[3] == b[3]
    dx, dy, ds = hip.up(batch.x), hip.up(batch.y), hip.up(batch.score)
    meta = (hip.up(batch.box_off.astype(np.int32)), hip.up(batch.id_base.astype(np.int64)))
    for rnd in range(2):
        ctx.submit(n_mg, k, BOX, batch.box_off, batch.id_base, dx, dy, ds,
                   fl | _lib.F_DEVICE_INPUTS, dev_meta=meta)
        _same(run, _snap_dev(hip, ctx.wait(), n_mg, k, multi), f"submit {rnd}")
    return run


@pytest.fixture
def dev():
    from repic_amd import _lib
    hip, ctx = _Hip(), _lib.Context(0)
    yield ctx, hip
    ctx.close()
    hip.free()


# ----------------------------------------------------------------------------- the cases
@pytest.mark.parametrize("mode", ["plain", "multi_out", "get_cc"])
@pytest.mark.parametrize("frac", [False, True])
@pytest.mark.parametrize("k", [3, 4])
def test_lattice_every_clique_an_exact_tie(dev, k, frac, mode):
    """5 x 5 sites, all k boxes of a site at the same place: 25 cliques, each a k-way exact tie,
    so the micrograph's tie segment is full (tie_cnt == C).  Integer coordinates take the f32
    layout, quarter-pixel ones the f64 layout."""
    ctx, hip = dev
    mgs = [_lattice(k, frac=frac, seed=1), _lattice(k, frac=frac, seed=2)]
    kw = dict(get_cc=mode == "get_cc", multi=mode == "multi_out")
    oracles = _oracles(mgs, k, kw["get_cc"], kw["multi"])
    if mode == "plain":
        for mg, o in zip(mgs, oracles):
            t = _oracle_ties(mg, o, k)
            assert len(t) == 25 and all(tie for _, tie in t)
    run = _check(ctx, hip, mgs, k, oracles, **kw)
    assert [g["stat"][5] for g in run] == ([25, 25] if mode != "get_cc" else [1, 1])


@pytest.mark.parametrize("k", [3, 4])
def test_batch_no_ties_all_ties_no_cliques(dev, k):
    """Three micrographs in one launch: an empty segment, a full one, and a micrograph whose
    epilogue never runs -- disjoint segments, zero counts."""
    ctx, hip = dev
    mgs = [_no_ties(k, seed=3), _lattice(k, seed=4), _no_cliques(k)]
    oracles = _oracles(mgs, k, False, False)
    assert oracles[2] is None
    assert not any(tie for _, tie in _oracle_ties(mgs[0], oracles[0], k))
    assert all(tie for _, tie in _oracle_ties(mgs[1], oracles[1], k))
    _check(ctx, hip, mgs, k, oracles)
    _check(ctx, hip, mgs, k, _oracles(mgs, k, False, True), multi=True)


@pytest.mark.parametrize("multi", [False, True])
def test_triangle_takes_the_in_kernel_insertion_order_path(dev, multi):
    """2 K >= nodes (one tied triangle, K = 3): networkx iterates in graph insertion order,
    which only the fused kernel's LDS graph has; nothing is handed off.  Beside it a set-order
    micrograph, so both forms run in one launch."""
    ctx, hip = dev
    tri = [(np.array([500.0]), np.array([500.0]), np.array([0.5 + 0.1 * p])) for p in range(3)]
    mgs = [tri, _lattice(3, nx=2, ny=2, seed=5), tri]
    _check(ctx, hip, mgs, 3, _oracles(mgs, 3, False, multi), multi=multi)


def test_integer_and_fractional_micrographs_in_one_batch(dev):
    """Ties in the f32 pass and in the f64 pass of one run: the ties launch behind each pass
    decides that pass's entries only (rgc_run: two launches; the second submission: the f64
    pass on the device, one ties launch behind both)."""
    ctx, hip = dev
    mgs = [_lattice(3, seed=6), _lattice(3, frac=True, seed=7), _no_ties(3, seed=8),
           _lattice(3, frac=True, seed=9), _lattice(3, seed=10), _no_ties(3, frac=True, seed=11)]
    for multi in (False, True):
        _check(ctx, hip, mgs, 3, _oracles(mgs, 3, False, multi), multi=multi)


def test_counts_do_not_outlive_their_run(dev):
    """One context: an all-ties batch, then a no-ties batch of the same shape (a count left
    behind would decide cliques that are not in the list), then a larger batch (the buffers
    regrow), through both paths each."""
    ctx, hip = dev
    k = 3
    a = [_lattice(k, seed=20 + i) for i in range(3)]
    b = [_no_ties(k, seed=30 + i) for i in range(3)]
    c = [(_lattice if i % 2 else _no_ties)(k, nx=6, ny=6, seed=40 + i) for i in range(9)]
    for mgs in (a, b, a, c, b):
        _check(ctx, hip, mgs, k, _oracles(mgs, k, False, False))


def test_ties_in_every_chunk_of_a_chunked_epilogue(dev):
    """Dense clusters (12 near-duplicates per picker and cluster, 5184 cliques of 108 boxes: far
    more than the clique queue holds, so P6 runs chunk by chunk and the segment counter carries
    over).  Integer offsets in [-3, 3] put exact ties among the cliques of every picker-0 box
    (checked here on the oracle's cliques); a chunk holds whole DFS subtrees of many such roots,
    so every chunk hands cliques off."""
    ctx, hip = dev
    k, per, ncl = 3, 12, 3
    mgs = [_dense_clusters(k, per, ncl, seed) for seed in range(2)]
    oracles = _oracles(mgs, k, False, False)
    for mg, o in zip(mgs, oracles):
        t = _oracle_ties(mg, o, k)
        assert len(t) == ncl * per ** k
        roots = {r for r, _ in t}
        assert len(roots) == ncl * per and roots == {r for r, tie in t if tie}
        assert sum(tie for _, tie in t) > len(t) // 20
    _check(ctx, hip, mgs, k, oracles)
    _check(ctx, hip, mgs, k, _oracles(mgs, k, False, True), multi=True)
