"""``repic consensus`` on the GPU (ABI 10): BOX directories to final picks in one device pass.

* the emit kernels (rgc_pick_select) against sorted(..., reverse=True) + np.rint in numpy, for
  segment sizes across the wavefront / workgroup / LDS-tile boundaries, with tied confidences
  (+0.0 and -0.0 among them) and every num_particles case
* the command's .box files are byte for byte those of get_cliques + run_ilp, on the goldens,
  with --num_particles, --get_cc and the multi-kernel route; the summary's ILP status is the
  two-step path's
* the picked columns are an optimal packing by an independent solver (HiGHS fixture / live)
* failure semantics: same exception class as get_cliques, same .box files as the two-step path
* the dispatcher entry point, the RGC_F_TIMING section names, the busy-context and --multi_out
  rejections
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import load_case, make_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- emit kernels
SIZES = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 5000]
CONF_VALUES = np.array([0.0, -0.0, 0.25, 0.5, 0.75, 1.0], np.float32)


@pytest.fixture(scope="module")
def pick_case():
    """One batch of segments (inputs and, per segment, the reference order), built once."""
    rng = np.random.default_rng(2024)
    col_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    nc = int(col_off[-1])
    x = (rng.random(nc) < 0.5).astype(np.uint8)
    x[col_off[4]:col_off[5]] = 0          # the 64-column segment: nothing chosen
    x[col_off[8]:col_off[9]] = 1          # the 1025-column segment: everything chosen
    x[col_off[1]] = 1                     # the 1-column segment has its pick
    conf = CONF_VALUES[rng.integers(0, len(CONF_VALUES), nc)]
    # .5 cases (half to even both ways), negatives, -0.x (rounds to -0.0)
    cx = rng.integers(-50, 4096, nc) + rng.choice([0.0, 0.5, 0.25, -0.25], nc)
    cy = rng.integers(-50, 4096, nc) + rng.choice([0.0, 0.5, 0.75], nc)
    order = []
    for m in range(len(SIZES)):
        a, b = int(col_off[m]), int(col_off[m + 1])
        sel = [j for j in range(b - a) if x[a + j] == 1]
        # run_ilp.py:120-128: a stable reverse sort of (clique, confidence) by confidence
        ranked = sorted(zip(sel, [conf[a + j] for j in sel]), key=lambda t: t[1], reverse=True)
        order.append(np.array([j for j, _ in ranked], np.int64))
    for a in (col_off, x, conf, cx, cy):
        a.setflags(write=False)
    return col_off, x, conf, cx, cy, order


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("num_particles", [None, 0, 1, 64, 100000])
def test_pick_select_matches_python_sort(pick_case, ctx, num_particles):
    col_off, x, conf, cx, cy, order = pick_case
    pick_off, px, py, pconf, pcol = ctx.pick_select(col_off, x, conf, cx, cy, num_particles)
    want_off, w_col, w_x, w_y, w_c = [0], [], [], [], []
    for m, o in enumerate(order):
        keep = o if num_particles is None else o[:num_particles]
        g = int(col_off[m]) + keep
        want_off.append(want_off[-1] + len(keep))
        w_col.append(keep)
        w_x.append(np.rint(cx[g]))
        w_y.append(np.rint(cy[g]))
        w_c.append(conf[g])
    assert np.array_equal(pick_off, np.array(want_off, np.int64))
    assert np.array_equal(pcol, np.concatenate(w_col).astype(np.int32))
    for got, want in ((px, np.concatenate(w_x)), (py, np.concatenate(w_y))):
        assert got.dtype == np.float64 and np.array_equal(got, want)
        assert np.array_equal(np.signbit(got), np.signbit(want))
    assert np.array_equal(pconf.view(np.uint32),
                          np.concatenate(w_c).astype(np.float32).view(np.uint32))


def test_pick_select_empty_batches(ctx):
    z = np.zeros(0)
    off, px, py, pconf, pcol = ctx.pick_select([0], z, z, z, z)
    assert off.tolist() == [0] and len(px) == len(pcol) == 0
    off, px, py, pconf, pcol = ctx.pick_select([0, 0, 0], z, z, z, z)
    assert off.tolist() == [0, 0, 0] and len(px) == 0


# ----------------------------------------------------------------------------- command parity
def _gc_args(in_dir, out_dir, meta, **kw):
    a = argparse.Namespace(in_dir=in_dir, out_dir=out_dir, box_size=meta["box"], multi_out=False,
                           get_cc=False, batch_boxes=1 << 25, threads=None, device=None,
                           listing=meta["listing"])
    for k_, v in kw.items():
        setattr(a, k_, v)
    return a


def _boxes(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".box"):
            with open(os.path.join(d, f), "rb") as fh:
                out[f] = fh.read()
    return out


def _two_step(in_dir, out_dir, meta, num_particles=None, **kw):
    """get_cliques then run_ilp into out_dir -> the exception get_cliques raised, or None."""
    from repic_amd.commands import get_cliques, run_ilp
    exc = None
    try:
        get_cliques.main(_gc_args(in_dir, out_dir, meta, **kw))
    except Exception as e:  # noqa: BLE001 - the class is compared with consensus'
        exc = e
    run_ilp.main(argparse.Namespace(in_dir=out_dir, box_size=meta["box"],
                                    num_particles=num_particles, node_limit=0, device=None))
    return exc


def _consensus(in_dir, out_dir, meta, num_particles=None, **kw):
    from repic_amd.commands import consensus
    exc = None
    try:
        consensus.main(_gc_args(in_dir, out_dir, meta, num_particles=num_particles,
                                node_limit=0, **kw))
    except Exception as e:  # noqa: BLE001
        exc = e
    return exc


def _summary(out_dir):
    from repic_amd.commands import consensus
    with open(os.path.join(out_dir, consensus.SUMMARY)) as f:
        lines = f.read().splitlines()
    assert lines[0] + "\n" == consensus.SUMMARY_HEADER
    return [ln.split("\t") for ln in lines[1:]]


def _assert_parity(name, tmp_path, num_particles=None, **kw):
    meta, _ = load_case(name)
    in_dir = make_inputs(name, str(tmp_path))
    two, one = str(tmp_path / "two"), str(tmp_path / "one")
    assert _two_step(in_dir, two, meta, num_particles, **kw) is None
    assert _consensus(in_dir, one, meta, num_particles, **kw) is None
    want, got = _boxes(two), _boxes(one)
    assert sorted(got) == sorted(want) and want
    for f in want:
        assert got[f] == want[f], f
    # nothing but the .box files and the summary
    assert sorted(os.listdir(one)) == sorted(list(got) + ["consensus_summary.tsv"])
    rows = _summary(one)
    assert len(rows) == len(want)
    assert sorted(r[0] + ".box" for r in rows) == sorted(want)
    n_ok = 0
    for r in rows:
        side = os.path.join(two, r[0] + "_ilp_status.tsv")
        if r[1] == "skip":
            assert want[r[0] + ".box"] == b"" and not os.path.exists(side)
            continue
        with open(side) as f:
            assert r[6] == f.read().split("\t")[0]
        assert int(r[3]) == want[r[0] + ".box"].count(b"\n")
        float(r[7])
        n_ok += 1
    assert n_ok > 0
    return rows


@pytest.mark.parametrize("name", ["c1_10017", "ties", "skips", "syn_k3_frac", "syn_k4", "syn_k5",
                                  "syn_k8"])
def test_consensus_matches_two_step(name, tmp_path):
    _assert_parity(name, tmp_path)


def test_consensus_num_particles(tmp_path):
    rows = _assert_parity("c1_10017", tmp_path, num_particles=7)
    assert max(int(r[3]) for r in rows) == 7


def test_consensus_get_cc(tmp_path):
    _assert_parity("c1_10017", tmp_path, get_cc=True)


def test_consensus_multikernel_route(tmp_path):
    _assert_parity("c1_10017", tmp_path, no_fused=True)


def test_consensus_split_batches(tmp_path):
    """Several device batches per chunk change nothing."""
    _assert_parity("c1_10017", tmp_path, batch_boxes=2000)


# ----------------------------------------------------------------------------- independent optimum
def _golden_batch(name, root):
    from repic_amd.ingest import DirIndex, list_methods, micrograph_names, plan_chunk
    meta, _ = load_case(name)
    in_dir = make_inputs(name, root)
    methods = list_methods(in_dir)
    index = DirIndex(in_dir, methods, meta["listing"])
    names = micrograph_names(index, methods)
    ch = plan_chunk(in_dir, methods, index, names, len(methods), meta["box"], 0, None)
    assert ch.crash is None and ch.batch is not None
    return ch.batch


def test_consensus_picks_are_an_optimal_packing(tmp_path, ctx):
    from scipy.sparse import coo_matrix

    from repic_amd import _lib
    from test_ilp import _check
    b = _golden_batch("c1_10017", str(tmp_path))
    r = ctx.consensus(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score,
                      flags=_lib.F_HOST_OUTPUTS)
    run = r.run
    probs, xs = [], []
    for m in range(b.n_mg):
        assert run.status[m] == _lib.OK
        c0, C = int(run.clique_base[m]), int(run.clique_cnt[m])
        rows = np.asarray(run.rows[c0:c0 + C])
        A = coo_matrix((np.ones(C * b.k, np.int64),
                        (rows.reshape(-1), np.repeat(np.arange(C), b.k))),
                       shape=(int(run.n_vert[m]), C))
        x = np.zeros(C, np.uint8)
        cols = r.pcol[r.pick_off[m]:r.pick_off[m + 1]]
        assert len(set(cols.tolist())) == len(cols) == r.sel_cnt[m]
        x[cols] = 1
        probs.append((A, np.asarray(run.w[c0:c0 + C]).copy()))
        xs.append(x)
        # the pick arrays are the chosen columns' own data, by decreasing confidence
        conf = np.asarray(run.conf[c0:c0 + C])
        g = np.asarray(run.consensus[c0:c0 + C])[cols]
        assert np.array_equal(r.pconf[r.pick_off[m]:r.pick_off[m + 1]], conf[cols])
        assert np.all(np.diff(conf[cols]) <= 0)
        assert np.array_equal(r.px[r.pick_off[m]:r.pick_off[m + 1]], np.rint(b.x[g]))
        assert np.array_equal(r.py[r.pick_off[m]:r.pick_off[m + 1]], np.rint(b.y[g]))
    assert probs
    _check(probs, xs, r.ilp_status.tolist())
    assert r.h2d_bytes > 0 and r.d2h_bytes > 0


# ----------------------------------------------------------------------------- failures
@pytest.mark.parametrize("name", ["crash_noedges", "crash_nocliques", "crash_4cols"])
def test_consensus_failure_semantics(name, tmp_path):
    meta, _ = load_case(name)
    in_dir = make_inputs(name, str(tmp_path))
    two, one = str(tmp_path / "two"), str(tmp_path / "one")
    e2 = _two_step(in_dir, two, meta)
    e1 = _consensus(in_dir, one, meta)
    assert e2 is not None and type(e1) is type(e2), (e1, e2)
    assert _boxes(one) == _boxes(two)


# ----------------------------------------------------------------------------- entry points
def test_consensus_cli_subprocess(tmp_path):
    in_dir = make_inputs("c1_10017", str(tmp_path))
    out = str(tmp_path / "out")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "repic-copy_amd"))
    r = subprocess.run([sys.executable, "-m", "repic_amd.main", "consensus", in_dir, out, "180"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "BOX files as starting point" in r.stdout
    boxes = _boxes(out)
    assert boxes and all(v for v in boxes.values())
    assert len(_summary(out)) == len(boxes)


def _small_batch():
    from repic_amd import synth
    from repic_amd.ingest import sigmoid
    from repic_amd.pipeline import Batch
    cfg = synth.SynthConfig(k=3, n_true=60, box=180, width=2048, height=2048, dup=0.1,
                            logit=(2,), seed=3)
    mgs = [[(x, y, sigmoid(s) if s.min() < 0 else s) for (x, y, s) in mg]
           for mg in synth.batch(cfg, 8)]
    return Batch.pack(cfg.k, cfg.box, mgs)


def test_consensus_timing_names_and_rejections(ctx):
    from repic_amd import _lib
    b = _small_batch()
    a = (b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score)
    r = ctx.consensus(*a, timing=True)
    names = [n for n, _ in ctx.kernel_times()]
    assert "k_pick_cols" in names and "k_pick_emit" in names
    assert names.index("k_pick_cols") < names.index("k_pick_emit")
    assert r.n_picked == r.pick_off[-1] > 0 and (r.ilp_status == 1).all()
    # the same batch without timing, and with the per-clique arrays kept in HBM: same picks
    r2 = ctx.consensus(*a)
    for f in ("pick_off", "px", "py", "pconf", "pcol", "sel_cnt"):
        assert np.array_equal(getattr(r, f), getattr(r2, f)), f
    with pytest.raises(_lib.RGCError, match="MULTI_OUT"):
        ctx.consensus(*a, flags=_lib.F_MULTI_OUT)
    ctx.submit(*a)
    try:
        with pytest.raises(_lib.RGCError, match="rgc_wait"):
            ctx.consensus(*a)
    finally:
        ctx.wait()
