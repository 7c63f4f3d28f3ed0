"""Particle-level matching at every confidence threshold on the GPU (k_score_match_sweep through
rgc_score_match_sweep): a step that has to move an earlier match, a warm-start augmenting path
through 299 earlier matches, equality with match_pairs and with the scipy oracle at every
threshold (mixed boxes, NaN confidences, unordered and duplicate thresholds, chunk loops past
256 and 1024 boxes, a batch whose pairs coincide), the edges of T, the refusals, the timing
names, the command line, and match_pairs unchanged after a sweep on the same context.
Everything is a count or a formatted count: nothing has a tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from score_match_sweep_util import ap_formula, check_monotone, check_sweep, mixed, sq, sweep_oracle
from score_match_util import case, oracle, prf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def _sweep(pairs, t, threshs, **kw):
    """match_sweep checked against the oracle at every pair and threshold."""
    from repic_amd import score_detections as sd
    got = sd.match_sweep(pairs, t, threshs, **kw)
    check_sweep(got, pairs, t, threshs)
    check_monotone(got, threshs)
    return got


# ---------------------------------------------------------------- the warm start
def test_second_step_moves_an_earlier_match():
    gt = np.array([[0., 0., 100., 100., 1.], [40., 0., 100., 100., 1.]])
    pk = np.array([[20., 0., 100., 100., .9], [0., 0., 100., 100., .5]])    # A: both boxes, B: the first
    assert sweep_oracle(gt, pk, 0.5, [0.7, 0.3]).tolist() == [[2, 1, 1], [2, 2, 2]]
    got = _sweep([(gt, pk)], 0.5, [0.7, 0.3])
    assert got[0, :, 2].tolist() == [1, 2]


def test_warm_start_path_through_299_earlier_matches():
    i = np.arange(300.0)
    gt = sq(np.stack([100 * i, 0 * i], axis=1), 100)
    pk = np.concatenate([sq(np.stack([100 * i[:299] + 50, 0 * i[:299]], axis=1), 100,
                            np.full(299, 0.9)),
                         sq([[0, 0]], 100, [0.2])])
    got = _sweep([(gt, pk)], 0.3, [0.5, 0.1])
    assert got[0].tolist() == [[300, 299, 299], [300, 300, 300]]


# ---------------------------------------------------------------- equality at every threshold
def test_mixed_boxes_equal_match_pairs_and_oracle_at_every_threshold():
    from repic_amd import score_detections as sd
    rng = np.random.default_rng(31)
    pairs = []
    for i in range(6):
        g = mixed(rng, 90, 400, 8, 60, neg=50)
        p = g[rng.integers(0, 90, 140)].copy()
        p[:, :2] += rng.integers(-16, 17, (140, 2)) / 2
        p[:, 2:4] += rng.integers(-10, 11, (140, 2)) / 2
        g[::7, 2] = rng.choice([0.0, 0.5, -3.0, 0.4], len(g[::7]))     # round(w) < 1
        p[::9, 3] = rng.choice([0.0, 0.5, -3.0, 0.4], len(p[::9]))     # round(h) < 1
        p[:, 4] = rng.uniform(0, 1, 140).round(1)
        p[rng.choice(140, 2, replace=False), 4] = np.nan
        pairs.append((g, p))
    ts = [0.5, -INF, 0.9, 0.5, 0.05, INF, 2.0]
    for t in (0.0, 0.3, 0.5):
        got = _sweep(pairs, t, ts)
        for j, ct in enumerate(ts):
            assert np.array_equal(got[:, j], sd.match_pairs(pairs, t, conf_thresh=ct)), (t, ct)
        assert (got[:, 5, 1] == 2).all() and (got[:, 6, 1] == 2).all()   # only the NaN picks
        assert (got[:, 1, 1] == 140).all() and np.array_equal(got[:, 0], got[:, 3])
        assert (got[:, 1, 2] > got[:, 2, 2]).all()
    curve = sd.match_curve(pairs[:2], 0.3, ts)
    got = sd.match_sweep(pairs[:2], 0.3, ts)
    for i in range(2):
        for j in range(len(ts)):
            g, k, tp = (int(v) for v in got[i, j])
            assert curve[i][j] == prf(g, k, tp) + (tp, g, k)
        assert [type(v) for v in curve[i][0]] == [float] * 3 + [int] * 3
        assert sd.average_precision(got[i]) == ap_formula(sweep_oracle(*pairs[i], 0.3, ts))


def test_one_pair_whose_chunk_loops_wrap_past_256_and_1024():
    rng = np.random.default_rng(32)
    g = sq(rng.integers(0, 3000, (700, 2)), 90)
    p = sq(g[rng.integers(0, 700, 1300), :2] + rng.integers(-35, 36, (1300, 2)), 90,
           rng.uniform(0, 1, 1300))
    ts = np.linspace(0.02, 0.98, 17).tolist()
    got = _sweep([(g, p)], 0.3, ts)
    assert len(set(got[0, :, 1].tolist())) == 17 and 500 < got[0, 0, 2] <= 700
    assert got[0, -1, 2] < got[0, 8, 2] < got[0, 0, 2]


def test_batch_of_64_pairs_whose_boxes_coincide_across_pairs():
    rng = np.random.default_rng(33)
    g = sq(rng.integers(0, 600, (40, 2)), 50)
    p = sq(g[rng.integers(0, 40, 55), :2] + rng.integers(-15, 16, (55, 2)), 50,
           rng.uniform(0, 1, 55).round(1))
    none = np.zeros((0, 5))
    pairs = []
    for i in range(64):
        # the same field in every pair, cut differently: state or a keep row that crossed
        # pairs would change the counts of the pairs that hold only a part of it
        gi = none if i % 9 == 4 else g[: 1 + (i * 7) % 40]
        pi = none if i % 11 == 6 else p[(i * 5) % 30:]
        pairs.append((gi, pi))
    got = _sweep(pairs, 0.3, [0.9, 0.1, 0.5, 0.3, 0.7])
    assert (got[[4, 13, 6, 17], :, 2] == 0).all()                  # early return: all T written
    assert got[:, 1, 2].max() > 20 and len(set(got[:, 1, 2].tolist())) > 10


def test_one_threshold_and_the_most_thresholds():
    from repic_amd import score_detections as sd
    rng = np.random.default_rng(34)
    g = sq(rng.integers(0, 600, (40, 2)), 50)
    p = sq(g[rng.integers(0, 40, 55), :2] + rng.integers(-15, 16, (55, 2)), 50,
           rng.uniform(0, 1, 55))
    for ct in (0.4, -INF):
        one = _sweep([(g, p)], 0.3, [ct])
        assert one.shape == (1, 1, 3)
        assert np.array_equal(one[:, 0], sd.match_pairs([(g, p)], 0.3, conf_thresh=ct))
    ts = np.linspace(0.0, 1.0, 1024)
    got = sd.match_sweep([(g, p)], 0.3, ts)
    assert got.shape == (1, 1024, 3)
    check_monotone(got, ts)
    for j in (0, 1, 100, 333, 512, 700, 1000, 1023):
        assert tuple(got[0, j].tolist()) == oracle(g, p, 0.3, ts[j])[0], j
    assert got[0, 0, 1] == 55 and got[0, 1023, 1] == 0 and got[0, 0, 2] > 20


# ---------------------------------------------------------------- refusals, timing
def _raw(ctx, n_pairs, gt_off, pk_off, boxes, t, n_thr, keep, counts=True, flags=0):
    from repic_amd import _lib
    from repic_amd import score_detections as sd
    go = np.ascontiguousarray(gt_off, dtype=np.int64)
    po = np.ascontiguousarray(pk_off, dtype=np.int64)
    bx = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.int64)
    out = np.full((min(max(n_pairs, 1), 8), max(min(n_thr, 1024), 1), 3), -7, np.int64)
    mi = sd.ScoreMatchIn(n_pairs, go.ctypes.data, po.ctypes.data, bx.ctypes.data, t, flags)
    sw = sd.ScoreMatchSweepIn(mi, n_thr, None if kp is None else kp.ctypes.data)
    _lib._check(_lib.lib.rgc_score_match_sweep(ctx._p, C.byref(sw),
                                               out.ctypes.data if counts else None))
    return out


def test_refusals_leave_the_context_usable():
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch
    c = _lib.Context(0)
    try:
        boxes = [[0, 10, 0, 10], [100, 110, 0, 10], [2, 12, 0, 10], [100, 110, 3, 13], [50, 60, 0, 10]]
        keep = [3, 2, 1]
        good = (1, [0, 2], [2, 5], boxes, 0.3, 3, keep)

        def valid():
            assert _raw(c, *good).tolist() == [[[2, 3, 2], [2, 2, 2], [2, 1, 1]]]

        def refused(match, *args, **kw):
            with pytest.raises(_lib.RGCError, match=match):
                _raw(c, *args, **kw)
            valid()
        valid()
        # what rgc_score_match refuses
        for t in (float("nan"), 1.0, -0.1, INF):
            refused("ji_threshold", 1, [0, 2], [2, 5], boxes, t, 3, keep)
        refused("null argument", *good, counts=False)
        refused("n_pairs out of range", -1, [0, 2], [2, 5], boxes, 0.3, 3, keep)
        refused("n_pairs out of range", 2 ** 31, [0, 2], [2, 5], boxes, 0.3, 3, keep)
        refused("negative box offset", 1, [-1, 2], [2, 5], boxes, 0.3, 3, keep)
        refused("non-decreasing", 2, [0, 2, 1], [2, 5, 5], boxes, 0.3, 3, keep * 2)
        refused("non-decreasing", 2, [0, 1, 2], [2, 5, 4], boxes, 0.3, 3, keep * 2)
        refused("2\\^31 - 1 boxes", 2, [0, 2 ** 30, 2 ** 31], [0, 0, 5], boxes, 0.3, 3, keep * 2)
        for bad in ([2 ** 30 + 1, 2 ** 30 + 2, 0, 1], [0, 1, -2 ** 30 - 1, 0],
                    [0, 2 ** 25 + 1, 0, 1], [0, 1, -5, 2 ** 25]):
            refused("box 3 is out of range", 1, [0, 2], [2, 5], boxes[:3] + [bad] + boxes[4:], 0.3,
                    3, keep)
        # the sweep's own
        for T in (0, -1, 1025, 2 ** 31 - 1):
            refused("n_thr -?[0-9]+ is outside 1..1024", 1, [0, 2], [2, 5], boxes, 0.3, T, keep)
        refused("null argument", 1, [0, 2], [2, 5], boxes, 0.3, 3, None)
        refused(r"keep\[0\]\[2\] = -1 is outside the pair's 3 picks", 1, [0, 2], [2, 5], boxes,
                0.3, 3, [3, 2, -1])
        refused(r"keep\[0\]\[0\] = 4 is outside the pair's 3 picks", 1, [0, 2], [2, 5], boxes,
                0.3, 3, [4, 2, 1])
        refused(r"keep\[0\] increases at threshold 2", 1, [0, 2], [2, 5], boxes, 0.3, 3, [2, 1, 2])
        refused(r"keep\[1\]\[0\] = 1 is outside the pair's 0 picks", 2, [0, 2, 2], [2, 5, 5],
                boxes, 0.3, 3, [3, 2, 1, 1, 0, 0])
        # no pairs: 0, nothing written, keep not read
        assert _raw(c, 0, [0], [0], boxes, 0.3, 3, None).tolist() == [[[-7] * 3] * 3]
        # the limit itself is accepted
        out = _raw(c, 1, [0, 2], [2, 5], boxes, 0.3, 1024, [3] * 24 + [2] * 500 + [0] * 500)
        assert out[0, :, 2].tolist() == [2] * 524 + [0] * 500
        # a submitted run that awaits rgc_wait
        cfg = synth.SynthConfig(k=3, n_true=20, box=180, width=1024, height=1024, seed=5)
        b = Batch.pack(cfg.k, cfg.box, synth.batch(cfg, 2))
        c.submit(b.n_mg, cfg.k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score)
        with pytest.raises(_lib.RGCError, match="rgc_score_match_sweep: a submitted run awaits "
                                                "rgc_wait"):
            _raw(c, *good)
        c.wait()
        valid()
    finally:
        c.close()


def test_timing_names_the_kernels():
    from repic_amd import score_detections as sd
    _, g, p, per_t = case("jitter")
    p = p.copy()
    p[:, 4] = np.random.default_rng(35).uniform(0, 1, len(p))
    counts, ms = sd.match_sweep([(g, p)], 0.3, [0.5, -INF], timing=True)
    assert counts[0, 1].tolist() == [300, 330, per_t[0][2]]
    assert list(ms) == ["k_score_match_count", "k_score_match_sweep"]
    assert all(v > 0 for v in ms.values())


def test_no_pairs():
    from repic_amd import score_detections as sd
    c = sd.match_sweep([], 0.3, [0.5, 0.1])
    assert c.shape == (0, 2, 3) and c.dtype == np.int64
    assert sd.match_curve([], 0.3, [0.5]) == []


# ---------------------------------------------------------------- match_pairs after a sweep
@pytest.mark.parametrize("name", ["chain300", "jitter"])
def test_match_pairs_returns_its_assignment_after_a_sweep_on_the_context(name):
    from repic_amd import _lib
    from repic_amd import score_detections as sd
    _, g, p, per_t = case(name)
    t = per_t[0][0]
    rng = np.random.default_rng(36)
    big_g = sq(rng.integers(0, 2000, (500, 2)), 90)
    big_p = sq(big_g[rng.integers(0, 500, 800), :2] + rng.integers(-35, 36, (800, 2)), 90,
               rng.uniform(0, 1, 800))
    q = p.copy()
    q[:, 4] = rng.uniform(0, 1, len(q))
    c = _lib.Context(0)
    try:
        before = sd.match_pairs([(g, p)] * 2, t, ctx=c, assignment=True)
        sd.match_sweep([(big_g, big_p), (g, q)], t, [0.2, 0.8, 0.5], ctx=c)
        after = sd.match_pairs([(g, p)] * 2, t, ctx=c, assignment=True)
    finally:
        c.close()
    assert np.array_equal(before[0], after[0]) and after[0][0, 2] == per_t[0][2]
    for x, y in zip(before[1], after[1]):
        assert np.array_equal(x, y) and np.array_equal(y, after[1][0])
    if name == "chain300":     # the one maximum matching of the chain
        assert after[1][0].tolist() == list(range(1, 300)) + [0]


# ---------------------------------------------------------------- command line
def test_command_line_match_sweep(tmp_path):
    rng = np.random.default_rng(37)
    gdir, pdir = tmp_path / "gt", tmp_path / "pk"
    gdir.mkdir()
    pdir.mkdir()
    data = {}
    for i in range(4):
        n = 30 + 10 * i
        g = sq(rng.integers(0, 900, (n, 2)), 64)
        p = sq(g[rng.integers(0, n, n + 8), :2] + rng.integers(-25, 26, (n + 8, 2)), 64,
               rng.uniform(0, 1, n + 8).round(1))
        for d, a, nm in ((gdir, g, f"mg{i}.box"), (pdir, p, f"mg{i}_picked.box")):
            with open(d / nm, "w") as f:
                for r in a:
                    f.write(f"{int(r[0])}\t{int(r[1])}\t64\t64\t{float(r[4])!r}\n")
        data[f"mg{i}"] = (g, p)
    names = ["mg0", "mg1", "mg2", "mg3"]
    files = (["-g"] + [str(f) for f in sorted(gdir.iterdir())] +
             ["-p"] + [str(f) for f in sorted(pdir.iterdir())])
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(
        [os.path.join(ROOT, "repic-copy_amd")] + [v for v in [env.get("PYTHONPATH")] if v])
    plain, swept, never = tmp_path / "plain", tmp_path / "swept", tmp_path / "never"
    t, ts = 0.4, [0.8, 0.2, 0.5]
    base = [sys.executable, "-m", "repic_amd.score_detections"] + files + ["-c", "0.3"]
    flag = ["--match_sweep"] + [repr(v) for v in ts]
    bad = subprocess.run(base + ["--out_dir", str(never)] + flag, env=env, timeout=300,
                         capture_output=True, text=True)
    assert bad.returncode == 2 and "--match_sweep needs --match_ji" in bad.stderr
    assert not never.exists()
    base += ["--match_ji", repr(t)]
    subprocess.run(base + ["--out_dir", str(plain)], check=True, env=env, timeout=300)
    subprocess.run(base + ["--out_dir", str(swept)] + flag, check=True, env=env, timeout=300)
    old = ["particle_set_comp.tsv", "particle_set_match.tsv", "particle_set_match_pooled.tsv"]
    assert sorted(f.name for f in plain.iterdir()) == old
    assert sorted(f.name for f in swept.iterdir()) == sorted(
        old + ["particle_set_match_sweep.tsv", "particle_set_match_sweep_pooled.tsv"])
    for f in old:
        assert (swept / f).read_bytes() == (plain / f).read_bytes(), f
    want = np.stack([sweep_oracle(*data[m], t, ts) for m in names])
    lines = (swept / "particle_set_match_sweep.tsv").read_text().splitlines()
    assert lines[0] == ("filename\tji_thresh\tconf_thresh\tn_gt\tn_picked\ttp\tprecision\trecall"
                        "\tf1")
    assert [ln.split("\t") for ln in lines[1:]] == [
        [m, repr(t), repr(ct)] + [str(v) for v in tuple(c) + prf(*c)]
        for m, cs in zip(names, want.tolist()) for ct, c in zip(ts, cs)]
    tot = want.sum(axis=0)
    assert (0 < tot[:, 2]).all() and tot[0, 2] < tot[2, 2] < tot[1, 2] < tot[1, 1]
    lines = (swept / "particle_set_match_sweep_pooled.tsv").read_text().splitlines()
    assert lines[0] == "ji_thresh\tconf_thresh\tn_gt\tn_picked\ttp\tprecision\trecall\tf1"
    assert [ln.split("\t") for ln in lines[1:4]] == [
        [repr(t), repr(ct)] + [str(v) for v in tuple(c) + prf(*c)]
        for ct, c in zip(ts, tot.tolist())]
    mean = sum(ap_formula(w) for w in want) / 4
    assert lines[4:] == [f"# average_precision\t{mean}\t{ap_formula(tot)}"]
    assert 0 < mean < 1 and 0 < ap_formula(tot) < 1
