"""``--ji_threshold`` on the device: the edge decision ``JI > t`` of both routes and both LDS
layouts at thresholds other than the reference's 0.3, against the CPU oracles with their
THRESHOLD patched to t and against the reference's own runs (tests/golden/thr_*).

The pair tests are built as tests/test_gpu_threshold.py is: one micrograph per pair, k = 2, one
box per picker, the RGC_F_EDGES hook; the device's edges must be the oracle's and its f64 JIs
bit-identical.
"""
import argparse
import builtins
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import assert_matches_golden, read_outputs
from threshold_util import THR, c_of, load_thr, make_thr_inputs, patch_oracles, rho

pytestmark = pytest.mark.gpu

BT = [(13, 0.3), (26, 0.5), (180, 0.2), (180, 0.05), (64, 0.0), (2896, 0.45)]


# ----------------------------------------------------------------------------- pairs
def _device_edges(x, y, a, b, B, t, no_fused):
    """One micrograph per pair -> {pair index: device JI} of the pairs the device keeps."""
    from repic_amd import _lib
    n = len(x)
    X = np.stack([x, a], axis=1).reshape(-1)
    Y = np.stack([y, b], axis=1).reshape(-1)
    S = np.full(2 * n, 0.5)
    box_off = np.arange(2 * n + 1, dtype=np.int64)
    id_base = np.arange(0, 2 * n, 2, dtype=np.int64)
    fl = _lib.F_HOST_OUTPUTS | _lib.F_EDGES | (_lib.F_NO_FUSED if no_fused else 0)
    ctx = _lib.Context(0)
    r = ctx.run(n, 2, B, box_off, id_base, X, Y, S, fl, ji_threshold=t)
    u, v, ji = ctx.last_edges()
    st = np.array(r.status)
    ctx.close()
    assert len(u) == int(r.n_edges)
    assert (u % 2 == 0).all() and (v == u + 1).all()
    m = u // 2
    assert len(np.unique(m)) == len(m)
    want = np.full(n, _lib.NO_EDGES)
    want[m] = _lib.OK
    assert np.array_equal(st, want)
    return dict(zip(m.tolist(), ji))


def _check_pairs(x, y, a, b, B):
    """Both routes against the (patched) oracle's decision and JI -> number of edges."""
    from oracle import cpu_vec
    t = cpu_vec.THRESHOLD
    x, y, a, b = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, a, b))
    ji_ref = cpu_vec.jaccard(x, y, a, b, B)
    edge = (np.abs(x - a) <= B) & (ji_ref > t)             # get_cliques.py:64-65
    for no_fused in (False, True):
        got = _device_edges(x, y, a, b, B, t, no_fused)
        assert sorted(got) == np.nonzero(edge)[0].tolist(), ("no_fused", no_fused)
        idx = np.array(sorted(got), dtype=np.int64)
        dev = np.array([got[i] for i in idx])
        assert np.array_equal(dev.view(np.uint64), ji_ref[idx].view(np.uint64))
    return int(edge.sum())


def _int_offsets(B, t, cut):
    """(dx, dy) >= 0 of the integer layout's deciding cases: areas within 2 of the cut, the
    nearest area on either side of it for every x overlap, and |dx| or |dy| within one pixel
    of the reach rho(t) B (B <= 64: every offset up to B + 1)."""
    if B <= 64:
        d = np.arange(0, B + 2)
        dx, dy = (v.reshape(-1) for v in np.meshgrid(d, d))
        return dx, dy
    px, py = [], []
    xo = np.arange(1, B + 1, dtype=np.int64)
    for area in range(max(cut - 2, 1), cut + 3):
        m = (area % xo == 0) & (area // xo <= B)
        px.append(B - xo[m])
        py.append(B - area // xo[m])
    # every column's nearest areas on either side of the cut (the window above can be empty:
    # at B = 2896, t = 0.45 no product of two overlaps lies within 2 of the cut)
    yo = cut // xo
    for w in (yo, yo + 1):
        m = (w >= 1) & (w <= B)
        px.append(B - xo[m])
        py.append(B - w[m])
    r = rho(t) * B
    full = np.arange(0, B + 2, dtype=np.int64)
    for v in range(max(int(np.floor(r)) - 1, 0), min(int(np.ceil(r)) + 1, B + 1) + 1):
        px += [np.full_like(full, v), full]
        py += [full, np.full_like(full, v)]
    p = np.unique(np.stack([np.concatenate(px), np.concatenate(py)], axis=1), axis=0)
    return p[:, 0], p[:, 1]


@pytest.mark.parametrize("B,t", BT)
def test_integer_layout_at_the_cutoff(B, t, monkeypatch):
    """Integer coordinates (f32 layout): every offset whose area is within 2 of int_cut, the
    offsets around the reach, all four sign combinations; at t = 0 the whole grid up to
    |dx| = B + 1, where JI = 0 at |dx| = B is not an edge."""
    from repic_amd import _lib
    patch_oracles(monkeypatch, t)
    cut = _lib.ji_cutoff(B, t)[0]
    dx, dy = _int_offsets(B, t, cut)
    area = np.maximum(B - dx, 0) * np.maximum(B - dy, 0)
    assert (area <= cut).any() and (area > cut).any()
    sx = np.concatenate([dx, -dx, dx, -dx]).astype(np.float64)
    sy = np.concatenate([dy, dy, -dy, -dy]).astype(np.float64)
    p = np.unique(np.stack([sx, sy], axis=1), axis=0)
    x0, y0 = 4000.0, 5000.0
    n = _check_pairs(np.full(len(p), x0), np.full(len(p), y0), x0 + p[:, 0], y0 + p[:, 1], B)
    assert 0 < n < len(p)
    if t == 0.0:
        at_b = (np.abs(p[:, 0]) == B) | (np.abs(p[:, 1]) == B)
        assert at_b.any()


@pytest.mark.parametrize("B,t", BT)
def test_f64_layout_at_the_threshold(B, t, monkeypatch):
    """Fractional coordinates (f64 layout): the partner's x stepped by +-1..4 ulps of the
    coordinate and by 2^-m relative steps of the offset (m = 30..52) around I = c(t) B^2, at
    several fixed dy."""
    patch_oracles(monkeypatch, t)
    rng = np.random.default_rng(B)
    c = c_of(t)
    x0, y0 = 512.25, 700.5
    A, Bb = [], []
    for f in (1.0, 0.8125, 0.71, 0.55, 0.37):
        yo = f * B
        if yo <= c * B:          # the area cannot reach c B^2 at this dy
            continue
        dy = B - yo
        dxs = B - c * B * B / yo   # the offset at which I crosses c(t) B^2
        for s in (-1.0, 1.0):
            a0 = x0 + s * dxs
            xs = [a0]
            for d in (np.inf, -np.inf):
                v = a0
                for _ in range(4):
                    v = np.nextafter(v, d)
                    xs.append(v)
            xs += [x0 + s * dxs * (1 + e * 2.0 ** -m) for m in range(30, 53) for e in (-1, 1)]
            A += xs
            Bb += [y0 - s * dy] * len(xs)
    a, b = np.array(A), np.array(Bb)
    o = rng.permutation(len(a))
    a, b = a[o], b[o]
    n = _check_pairs(np.full(len(a), x0), np.full(len(a), y0), a, b, B)
    assert 0 < n < len(a)


# ----------------------------------------------------------------------------- reach
def _reach_field(t, seed, B=100, n_anchor=50, field=4000):
    """One k = 3 micrograph of 4 n_anchor boxes on a 40 B x 40 B field: picker-0 anchors; a
    picker-1 partner of each at d_in = floor(rho B - 1) pixels in x, in y or on a diagonal;
    a picker-2 partner of each picker-1 box likewise; picker-2 decoys of the anchors at
    d_out = ceil(rho B + 1)."""
    rng = np.random.default_rng(seed)
    d_in, d_out = int(np.floor(rho(t) * B - 1)), int(np.ceil(rho(t) * B + 1))
    dirs = np.array([(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)])
    ax = rng.integers(3 * B, field - 3 * B, n_anchor).astype(np.float64)
    ay = rng.integers(3 * B, field - 3 * B, n_anchor).astype(np.float64)
    d1 = dirs[np.arange(n_anchor) % 8]
    d2 = dirs[rng.integers(0, 8, n_anchor)]
    d3 = dirs[(np.arange(n_anchor) + 3) % 8]
    p1x, p1y = ax + d1[:, 0] * d_in, ay + d1[:, 1] * d_in
    p2x, p2y = p1x + d2[:, 0] * d_in, p1y + d2[:, 1] * d_in
    qx, qy = ax + d3[:, 0] * d_out, ay + d3[:, 1] * d_out
    sc = lambda n: rng.uniform(0.3, 1.0, n)  # noqa: E731
    return [(ax, ay, sc(n_anchor)), (p1x, p1y, sc(n_anchor)),
            (np.concatenate([p2x, qx]), np.concatenate([p2y, qy]), sc(2 * n_anchor))]


@pytest.mark.parametrize("t", [0.0, 0.05, 0.15])
def test_reach_across_cell_borders(t, monkeypatch):
    """Lower thresholds reach further than today's cells: the grid planned from rho(t) must
    still hold every partner in the 2x3 stencil.  Edge list == cpu_vec.edges on both routes,
    on the integer layout and on the same coordinates + 0.125 (f64 layout)."""
    from oracle import cpu_vec
    from repic_amd import _lib
    patch_oracles(monkeypatch, t)
    B = 100
    mg = _reach_field(t, seed=int(t * 100) + 1, B=B)
    for shift in (0.0, 0.125):
        x = np.concatenate([p[0] for p in mg]) + shift
        y = np.concatenate([p[1] for p in mg]) + shift
        s = np.concatenate([p[2] for p in mg])
        counts = [len(p[0]) for p in mg]
        pick = np.repeat(np.arange(3), counts)
        ou, ov, oji = cpu_vec.edges(x, y, pick, B)
        assert len(ou) >= 30                                # (the partners at d_in in x or y)
        box_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        for no_fused in (False, True):
            fl = _lib.F_HOST_OUTPUTS | _lib.F_EDGES | (_lib.F_NO_FUSED if no_fused else 0)
            ctx = _lib.Context(0)
            r = ctx.run(1, 3, B, box_off, np.zeros(1, np.int64), x, y, s, fl, ji_threshold=t)
            u, v, ji = ctx.last_edges()
            ne = int(r.n_edges)
            ctx.close()
            o = np.lexsort((v, u))
            assert ne == len(ou), (shift, no_fused, ne, len(ou))
            assert np.array_equal(u[o], ou) and np.array_equal(v[o], ov), (shift, no_fused)
            assert np.array_equal(ji[o].view(np.uint64), oji.view(np.uint64))


# ----------------------------------------------------------------------------- goldens
def _args(in_dir, out_dir, meta, **kw):
    a = argparse.Namespace(in_dir=in_dir, out_dir=out_dir, box_size=meta["box"],
                           multi_out="--multi_out" in meta["flags"],
                           get_cc="--get_cc" in meta["flags"], batch_boxes=1 << 25,
                           threads=None, device=None, listing=meta["listing"],
                           ji_threshold=meta["ji_threshold"])
    for k_, v in kw.items():
        setattr(a, k_, v)
    return a


@pytest.mark.parametrize("no_fused", [False, True])
@pytest.mark.parametrize("name", THR)
def test_gpu_matches_reference_at_threshold(name, no_fused, tmp_path):
    """The reference's own run with its threshold argument set to t, bit-exact, both routes."""
    from repic_amd.commands import get_cliques
    meta, data = load_thr(name)
    in_dir = make_thr_inputs(meta, str(tmp_path))
    out_dir = os.path.join(str(tmp_path), "out")
    exc = None
    try:
        get_cliques.main(_args(in_dir, out_dir, meta, no_fused=no_fused))
    except Exception as e:  # noqa: BLE001 - the exception class is part of the contract
        exc = e
    if meta["exception"]:
        assert isinstance(exc, getattr(builtins, meta["exception"])), exc
    else:
        assert exc is None, repr(exc)
    mgs, arrays = read_outputs(out_dir, meta)
    assert_matches_golden(meta, data, mgs, arrays)


def test_gpu_cli_threshold_subprocess(tmp_path):
    """`python -m repic_amd.main get_cliques <in> <out> 180 --ji_threshold 0.2` as a separate
    process, replaying the recorded listing."""
    meta, data = load_thr("thr_syn_k3_0.2")
    in_dir = make_thr_inputs(meta, str(tmp_path))
    out_dir = os.path.join(str(tmp_path), "out")
    lst = os.path.join(str(tmp_path), "listing.json")
    with open(lst, "w") as f:
        json.dump(meta["listing"], f)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "repic-copy_amd"),
                                                       os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "repic_amd.main", "get_cliques", in_dir, out_dir,
                        str(meta["box"]), "--ji_threshold", "0.2", "--listing", lst], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    mgs, arrays = read_outputs(out_dir, meta)
    assert_matches_golden(meta, data, mgs, arrays)


# ----------------------------------------------------------------------------- vs oracles
def _check_vs_vec(mgs, k, box, t, get_cc=False, no_fused=False):
    """Every output of a batch against the vectorised oracle (patched to t), bit-exact."""
    from oracle import cpu_vec
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    assert cpu_vec.THRESHOLD == t
    batch = Batch.pack(k, box, mgs)
    ctx = _lib.Context(0)
    res = run_batch(ctx, batch, get_cc=get_cc, no_fused=no_fused, members=True, ji_threshold=t)
    ctx.close()
    n_cl, edges = 0, []
    for m, mg in enumerate(mgs):
        b0 = int(batch.box_off[m * k])
        x, y, s = (np.concatenate([p[i] for p in mg]) for i in range(3))
        o = cpu_vec.micrograph(x, y, s, [len(p[0]) for p in mg], box, get_cc=get_cc,
                               id_base=int(batch.id_base[m]))
        r = res[m]
        assert o["status"] == "ok" and r.status == _lib.OK
        assert (r.cc_max, r.cc_cnt) == (o["cc_max"], o["cc_cnt"])
        assert r.n_edges == o["n_edges"] and r.n_vert == o["V"]
        mem = r.members.astype(np.int64) - b0
        assert mem.shape == o["members"].shape, (mem.shape, o["members"].shape)
        p = np.lexsort(mem.T[::-1])      # oracle members are already lexicographic
        assert np.array_equal(mem[p], o["members"])
        assert np.array_equal(r.rows[p], o["rows"])
        assert np.array_equal(r.w[p].view(np.uint32), o["w"].view(np.uint32))
        assert np.array_equal(r.conf[p].view(np.uint32), o["conf"].view(np.uint32))
        assert np.array_equal(r.consensus[p].astype(np.int64) - b0, o["consensus"])
        n_cl += len(p)
        edges.append(o["n_edges"])
    return n_cl, edges


@pytest.mark.parametrize("get_cc", [False, True])
def test_dense_low_threshold(get_cc, monkeypatch):
    """4 micrographs of the C2 kind (k = 3, about 900 boxes) at t = 0.02, with the field halved
    to 2048 x 2048: on C2's own 4096 x 4096 field the oracle counts about 2600 edges per
    micrograph, within the 960-box class's edge capacity (about 4270), so nothing would defer;
    on the halved field it counts about 8200 (forward lists of up to 43 targets, past the 32
    candidates of the edge bitmask), so the f32 pass overflows its edge capacity and the
    micrographs go through deferral."""
    from repic_amd import synth
    from repic_amd.ingest import sigmoid
    t = 0.02
    patch_oracles(monkeypatch, t)
    cfg = synth.SynthConfig(**{**synth.CONFIGS["C2"], "width": 2048, "height": 2048}, seed=5,
                            logit=(1,))
    mgs = [[(x, y, sigmoid(s) if s.min() < 0 else s) for (x, y, s) in mg]
           for mg in synth.batch(cfg, 4)]
    n_cl, edges = _check_vs_vec(mgs, cfg.k, cfg.box, t, get_cc=get_cc)
    assert n_cl > 0 and max(edges) > 4300


def _clusters(k, per, n_clusters, seed, spread, box=100):
    """tests/test_gpu_parity._dense_clusters with the +-3 pixel jitter scaled by ``spread``."""
    rng = np.random.default_rng(seed)
    cx = rng.uniform(0, 3000, n_clusters).round()
    cy = rng.uniform(0, 3000, n_clusters).round()
    mg = []
    for _ in range(k):
        x = np.concatenate([c + spread * rng.integers(-3, 4, per) for c in cx]).astype(np.float64)
        y = np.concatenate([c + spread * rng.integers(-3, 4, per) for c in cy]).astype(np.float64)
        mg.append((x, y, rng.uniform(0.3, 1.0, len(x))))
    return mg


@pytest.mark.parametrize("k,per,n_clusters", [(4, 3, 30), (5, 4, 6)])
def test_p4_adjacency_agrees_with_p2(k, per, n_clusters, monkeypatch):
    """Near-duplicate clusters whose member distances (up to 36 pixels per axis) straddle the
    reach rho(0.5) B = 33.3: some members of a cluster are adjacent and some are not, so a
    BFS adjacency test (EdgeP) that disagreed with P2's edge lists would change the cliques.
    Cliques, weights and consensus against the scalar oracle on both routes."""
    from oracle import cpu_ref, cpu_vec
    from repic_amd import _lib
    from repic_amd.pipeline import Batch, run_batch
    t, box = 0.5, 100
    patch_oracles(monkeypatch, t)
    mgs = [_clusters(k, per, n_clusters, seed, spread=6, box=box) for seed in range(2)]
    # the clusters do straddle: within a cluster some cross-picker pairs are edges, some not
    x, y = (np.concatenate([p[i] for p in mgs[0]]) for i in range(2))
    pick = np.repeat(np.arange(k), [len(p[0]) for p in mgs[0]])
    ne = len(cpu_vec.edges(x, y, pick, box)[0])
    n_pairs = n_clusters * per * per * k * (k - 1) // 2
    assert 0.1 * n_pairs < ne < 0.9 * n_pairs
    batch = Batch.pack(k, box, mgs)
    methods = [f"picker{p}" for p in range(k)]
    for no_fused in (False, True):
        ctx = _lib.Context(0)
        res = run_batch(ctx, batch, no_fused=no_fused, ji_threshold=t)
        ctx.close()
        for m, mg in enumerate(mgs):
            coords, nid = [], int(batch.id_base[m])
            for (px, py, ps) in mg:
                coords.append([(float(a), float(b), float(c), nid + i)
                               for i, (a, b, c) in enumerate(zip(px, py, ps))])
                nid += len(px)
            o = cpu_ref.micrograph(coords, box, methods)
            r = res[m]
            A = o["A"].tocoo()
            C = A.shape[1]
            assert C > 0 and r.status == _lib.OK and len(r.w) == C and r.n_vert == A.shape[0]
            orows = np.sort(A.row[np.argsort(A.col, kind="stable")].reshape(C, k), axis=1)
            po, pg = np.lexsort(orows.T[::-1]), np.lexsort(r.rows.T[::-1])
            assert np.array_equal(orows[po], r.rows[pg])
            assert np.array_equal(o["w"][po].view(np.uint32), r.w[pg].view(np.uint32))
            assert np.array_equal(o["conf"][po].view(np.uint32), r.conf[pg].view(np.uint32))
            idb = int(batch.id_base[m]) - int(batch.box_off[m * k])
            got = [(float(batch.x[g]), float(batch.y[g]), idb + int(g)) for g in r.consensus[pg]]
            assert got == [o["consensus"][i] for i in po]
            assert (r.cc_max, r.cc_cnt) == (o["cc_max"], o["cc_cnt"])


# ----------------------------------------------------------------------------- default path
def _syn_k3_batch(root):
    from golden_util import load_case, make_inputs
    from repic_amd.ingest import DirIndex, list_methods, micrograph_names, plan_chunk
    meta, _ = load_case("syn_k3")
    in_dir = make_inputs("syn_k3", root)
    methods = list_methods(in_dir)
    index = DirIndex(in_dir, methods, meta["listing"])
    names = micrograph_names(index, methods)
    ch = plan_chunk(in_dir, methods, index, names, len(methods), meta["box"], 0, None)
    assert ch.crash is None and ch.batch is not None
    return ch.batch


_PER_MG = ("status", "cc_max", "cc_cnt", "n_nodes", "n_vert", "n_edges_mg", "clique_cnt")


def _snap_host(r):
    d = {f: np.array(getattr(r, f)).tobytes() for f in _PER_MG}
    d["tot"] = (int(r.n_boxes), int(r.n_edges), int(r.n_cliques))
    for f in ("rows", "w", "conf", "consensus", "members"):
        v = np.asarray(getattr(r, f))
        d[f] = [v[int(b0):int(b0) + int(n)].tobytes() for b0, n in zip(r.clique_base, r.clique_cnt)]
    return d


def test_default_threshold_flag_changes_nothing_run(tmp_path):
    """rgc_run with RGC_F_JI_THRESHOLD and 0.3 == rgc_run without the flag, byte for byte, on
    both routes; and 0.2 does change the result (the flag is honoured)."""
    from repic_amd import _lib
    b = _syn_k3_batch(str(tmp_path))
    for route in (0, _lib.F_NO_FUSED):
        fl = _lib.F_HOST_OUTPUTS | _lib.F_MEMBERS | _lib.F_GET_CC | route
        ctx = _lib.Context(0)
        snaps = [_snap_host(ctx.run(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y,
                                    b.score, fl, ji_threshold=t)) for t in (None, 0.3, 0.2)]
        ctx.close()
        assert snaps[0] == snaps[1]
        assert snaps[2]["tot"][1] > snaps[0]["tot"][1]       # more edges at 0.2
    for bad in (-0.1, 1.0, float("nan"), float("inf")):
        ctx = _lib.Context(0)
        with pytest.raises(_lib.RGCError, match="ji_threshold"):
            ctx.run(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                    _lib.F_HOST_OUTPUTS, ji_threshold=bad)
        with pytest.raises(_lib.RGCError, match="ji_threshold"):
            ctx.submit(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                       _lib.F_HOST_OUTPUTS, ji_threshold=bad)
        with pytest.raises(_lib.RGCError, match="ji_threshold"):
            ctx.consensus(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                          ji_threshold=bad)
        ctx.close()


class _Hip:
    """Device buffers through the HIP runtime the library itself uses."""

    def __init__(self):
        import ctypes
        self.C = ctypes
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.ptrs = []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.C.c_void_p()
        assert self.hip.hipMalloc(self.C.byref(p), self.C.c_size_t(max(arr.nbytes, 8))) == 0
        assert self.hip.hipMemcpy(p, self.C.c_void_p(arr.ctypes.data),
                                  self.C.c_size_t(arr.nbytes), self.C.c_int(1)) == 0
        self.ptrs.append(p)
        return p.value

    def down(self, ptr, n, dtype):
        out = np.empty(n, dtype=dtype)
        if n:
            assert self.hip.hipMemcpy(self.C.c_void_p(out.ctypes.data), self.C.c_void_p(int(ptr)),
                                      self.C.c_size_t(out.nbytes), self.C.c_int(2)) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


def test_default_threshold_flag_changes_nothing_submit(tmp_path):
    """rgc_submit / rgc_wait on HBM-resident inputs (the single fused launch the bench's steps
    take): the flag with 0.3 gives the unflagged run's outputs, byte for byte per micrograph."""
    from repic_amd import _lib
    b = _syn_k3_batch(str(tmp_path))
    k = b.k
    hip = _Hip()
    ctx = _lib.Context(0)
    try:
        dx, dy, ds = hip.up(b.x), hip.up(b.y), hip.up(b.score)
        meta = (hip.up(b.box_off.astype(np.int32)), hip.up(b.id_base.astype(np.int64)))
        fl = _lib.F_DEVICE_INPUTS | _lib.F_MEMBERS | _lib.F_GET_CC

        def go(t):
            ctx.submit(b.n_mg, k, b.box_size, b.box_off, b.id_base, dx, dy, ds, fl,
                       dev_meta=meta, ji_threshold=t)
            r = ctx.wait()
            d = {f: np.array(getattr(r, f)).tobytes() for f in _PER_MG}
            d["tot"] = (int(r.n_boxes), int(r.n_edges), int(r.n_cliques))
            C = int(r.n_cliques)
            for f, dt, w in (("rows", np.int32, k), ("w", np.float32, 1), ("conf", np.float32, 1),
                             ("consensus", np.int32, 1), ("members", np.int32, k)):
                v = hip.down(getattr(r, f), C * w, dt).reshape(C, w)
                d[f] = [v[int(b0):int(b0) + int(n)].tobytes()
                        for b0, n in zip(r.clique_base, r.clique_cnt)]
            return d
        plain, flagged, lower = go(None), go(0.3), go(0.2)
        assert plain["tot"][2] > 0 and plain == flagged
        assert lower["tot"][1] > plain["tot"][1]
    finally:
        ctx.close()
        hip.free()


# ----------------------------------------------------------------------------- consensus
def test_consensus_at_threshold_matches_two_step(tmp_path):
    """`repic consensus --ji_threshold 0.5` writes the .box files of `get_cliques
    --ji_threshold 0.5` followed by `run_ilp`, byte for byte (and the get_cliques half is the
    reference's run at 0.5)."""
    from repic_amd.commands import consensus, get_cliques, run_ilp
    meta, data = load_thr("thr_syn_k3_0.5")
    in_dir = make_thr_inputs(meta, str(tmp_path))
    two, one = str(tmp_path / "two"), str(tmp_path / "one")
    get_cliques.main(_args(in_dir, two, meta, ji_threshold=0.5))
    mgs, arrays = read_outputs(two, meta)
    assert_matches_golden(meta, data, mgs, arrays)
    run_ilp.main(argparse.Namespace(in_dir=two, box_size=meta["box"], num_particles=None,
                                    node_limit=0, device=None))
    consensus.main(_args(in_dir, one, meta, ji_threshold=0.5, num_particles=None, node_limit=0))

    def boxes(d):
        out = {}
        for f in sorted(os.listdir(d)):
            if f.endswith(".box"):
                with open(os.path.join(d, f), "rb") as fh:
                    out[f] = fh.read()
        return out
    want, got = boxes(two), boxes(one)
    assert want and sorted(want) == sorted(got)
    assert all(len(v) > 0 for v in want.values())
    for f in want:
        assert got[f] == want[f], f
    # the default threshold gives other picks: the option reaches the device
    dflt = str(tmp_path / "dflt")
    consensus.main(_args(in_dir, dflt, meta, ji_threshold=None, num_particles=None,
                         node_limit=0))
    assert boxes(dflt) != got
