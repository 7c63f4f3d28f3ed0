"""Particle-level matching of score_detections on the GPU (k_score_match through
rgc_score_match): the sizes and the edges the real reference recorded, a numpy / scipy
restatement on the kernel's own edges (mixed sizes, rounding, boxes without a pixel, chunk loops
past 256 and 1024 boxes, a batch whose pairs coincide, contested boxes), the confidence filter,
determinism, the refusals, the timing names and the command line.  Everything is a count or an
index: nothing has a tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from score_match_util import case, cases, check_assignment, kept, oracle, prf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sq(xy, B, conf=None):
    """(n, 5) boxes x, y, B, B, conf of (n, 2) corners."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    c = np.ones(len(xy)) if conf is None else np.asarray(conf, dtype=np.float64)
    return np.concatenate([xy, np.full((len(xy), 2), float(B)), c[:, None]], axis=1)


def _check_pairs(pairs, t, conf_thresh=None):
    """match_pairs on `pairs` against the restatement: counts, and every assignment a matching
    of its own pair's edges."""
    from repic_amd import score_detections as sd
    counts, assign = sd.match_pairs(pairs, t, conf_thresh, assignment=True)
    assert counts.shape == (len(pairs), 3) and counts.dtype == np.int64
    assert len(assign) == len(pairs)
    for i, (g, p) in enumerate(pairs):
        want, E = oracle(g, p, t, conf_thresh)
        assert tuple(counts[i].tolist()) == want, (i, counts[i], want)
        assert len(assign[i]) == want[1]
        check_assignment(assign[i], E, want[2], want[0])
    return counts, assign


# ---------------------------------------------------------------- goldens
def test_goldens_sizes_and_assignments_on_the_reference_edges():
    from repic_amd import score_detections as sd
    n = 0
    for name, g, p, per_t in cases():
        for t, edges, size in per_t:
            counts, assign = sd.match_pairs([(g, p)], t, assignment=True)
            assert counts.tolist() == [[len(g), len(p), size]], (name, t, counts)
            check_assignment(assign[0], edges, size, len(g))
            n += 1
    assert n == 4 + 4 + 3


def test_goldens_in_one_batch_and_scores():
    from repic_amd import score_detections as sd
    cs = [c for c in cases() if len(c[3]) == 1 and c[3][0][0] == 0.3]
    assert len(cs) == 5
    got = sd.match_scores([(g, p) for _, g, p, _ in cs], 0.3)
    for (name, g, p, per_t), s in zip(cs, got):
        size = per_t[0][2]
        assert s == prf(len(g), len(p), size) + (size, len(g), len(p)), name
        assert [type(v) for v in s] == [float] * 3 + [int] * 3


# ---------------------------------------------------------------- the restatement oracle
def _mixed(rng, n, field, lo, hi, neg=0):
    x = rng.integers(-2 * neg, 2 * field, n) / 2          # .5 values: round() goes to even
    y = rng.integers(-2 * neg, 2 * field, n) / 2
    w = rng.integers(2 * lo, 2 * hi, n) / 2
    h = rng.integers(2 * lo, 2 * hi, n) / 2
    return np.stack([x, y, w, h, rng.uniform(0, 1, n)], axis=1)


def test_mixed_sizes_fractional_negative_and_degenerate_boxes():
    rng = np.random.default_rng(21)
    pairs = []
    for i in range(6):
        g = _mixed(rng, 90, 400, 8, 60, neg=50)
        p = g[rng.integers(0, 90, 140)].copy()
        p[:, :2] += rng.integers(-16, 17, (140, 2)) / 2
        p[:, 2:4] += rng.integers(-10, 11, (140, 2)) / 2
        g[::7, 2] = rng.choice([0.0, 0.5, -3.0, 0.4], len(g[::7]))     # round(w) < 1
        p[::9, 3] = rng.choice([0.0, 0.5, -3.0, 0.4], len(p[::9]))     # round(h) < 1
        pairs.append((g, p))
    for t in (0.0, 0.3, 0.5):
        counts, _ = _check_pairs(pairs, t)
        assert (counts[:, 2] > 0).all()


def test_one_pair_whose_chunk_loops_wrap_past_256_and_1024():
    rng = np.random.default_rng(22)
    g = _sq(rng.integers(0, 3000, (700, 2)), 90)
    p = _sq(g[rng.integers(0, 700, 1300), :2] + rng.integers(-35, 36, (1300, 2)), 90)
    counts, _ = _check_pairs([(g, p)], 0.3)
    assert 500 < counts[0, 2] <= 700


def test_batch_of_64_pairs_whose_boxes_coincide_across_pairs():
    rng = np.random.default_rng(23)
    g = _sq(rng.integers(0, 600, (40, 2)), 50)
    p = _sq(g[rng.integers(0, 40, 55), :2] + rng.integers(-15, 16, (55, 2)), 50)
    none = np.zeros((0, 5))
    pairs = []
    for i in range(64):
        # the same field in every pair, cut differently: an edge that crossed pairs would add
        # matches to the pairs that hold only a part of it
        gi = none if i % 9 == 4 else g[: 1 + (i * 7) % 40]
        pi = none if i % 11 == 6 else p[(i * 5) % 30:]
        pairs.append((gi, pi))
    counts, _ = _check_pairs(pairs, 0.3)
    assert (counts[[4, 13, 6, 17], 2] == 0).all()
    assert counts[:, 2].max() > 20 and len(set(counts[:, 2].tolist())) > 10


def test_contested_boxes():
    from repic_amd import score_detections as sd
    spot = [[100.0, 100.0]]
    five_on_three = (_sq(spot * 3, 32), _sq(spot * 5, 32))
    star = (_sq(spot, 32), _sq([[100 + dx, 100 + dy] for dx, dy in
                                [(0, 0), (3, 0), (-3, 0), (0, 3), (0, -3), (2, 2), (-2, 2), (2, -2)]], 32))
    heap = (_sq(spot * 20, 32), _sq(spot * 30, 32))
    assert _check_pairs([five_on_three, star], 0.3)[0][:, 2].tolist() == [3, 1]
    counts, assign = _check_pairs([heap], 0.0)
    assert counts.tolist() == [[20, 30, 20]]
    assert sorted(a for a in assign[0].tolist() if a >= 0) == list(range(20))
    assert sd.match_scores([star], 0.3) == [(1 / 8, 1.0, 2 * (1 / 8) / (1 + 1 / 8), 1, 1, 8)]


# ---------------------------------------------------------------- confidence filter
def test_conf_thresh_equals_prefiltered_lists_and_keeps_nan():
    from repic_amd import score_detections as sd
    rng = np.random.default_rng(24)
    g = _sq(rng.integers(0, 800, (80, 2)), 60)
    conf = rng.uniform(0, 1, 120).round(1)
    conf[[3, 50]] = np.nan
    p = _sq(g[rng.integers(0, 80, 120), :2] + rng.integers(-20, 21, (120, 2)), 60, conf)
    for ct in (0.5, 0.0, 2.0):
        counts, assign = _check_pairs([(g, p)], 0.3, ct)
        pre = sd.match_pairs([(g, kept(p, ct))], 0.3, assignment=True)
        assert np.array_equal(counts, pre[0]) and np.array_equal(assign[0], pre[1][0])
    assert sd.match_pairs([(g, p)], 0.3, 2.0)[0, 1] == 2          # only the NaN picks are left
    recs = [tuple(r) for r in p.tolist()]                         # box records, as the CLI's
    assert np.array_equal(sd.match_pairs([(g.tolist(), recs)], 0.3, 0.5),
                          sd.match_pairs([(g, p)], 0.3, 0.5))


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["chain300", "jitter"])
def test_two_runs_return_identical_assignments(name):
    from repic_amd import score_detections as sd
    _, g, p, per_t = case(name)
    a = sd.match_pairs([(g, p)] * 3, per_t[0][0], assignment=True)
    b = sd.match_pairs([(g, p)] * 3, per_t[0][0], assignment=True)
    assert np.array_equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y) and np.array_equal(x, a[1][0])
    if name == "chain300":     # the one maximum matching of the chain
        assert a[1][0].tolist() == list(range(1, 300)) + [0]


# ---------------------------------------------------------------- refusals, timing
def _raw(ctx, n_pairs, gt_off, pk_off, boxes, t, counts=True, flags=0):
    from repic_amd import _lib
    from repic_amd import score_detections as sd
    go = np.ascontiguousarray(gt_off, dtype=np.int64)
    po = np.ascontiguousarray(pk_off, dtype=np.int64)
    bx = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    out = np.full((min(max(n_pairs, 1), 8), 3), -7, np.int64)
    match = np.full(max(int(po[-1] - po[0]), 1), -7, np.int32)
    mi = sd.ScoreMatchIn(n_pairs, go.ctypes.data, po.ctypes.data, bx.ctypes.data, t, flags)
    _lib._check(_lib.lib.rgc_score_match(ctx._p, C.byref(mi), out.ctypes.data if counts else None,
                                         match.ctypes.data))
    return out, match


def test_refusals_leave_the_context_usable():
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch
    c = _lib.Context(0)
    try:
        boxes = [[0, 10, 0, 10], [100, 110, 0, 10], [2, 12, 0, 10], [100, 110, 3, 13], [50, 60, 0, 10]]
        good = (1, [0, 2], [2, 5], boxes, 0.3)

        def valid():
            out, match = _raw(c, *good)
            assert out.tolist() == [[2, 3, 2]] and match.tolist() == [0, 1, -1]
        valid()
        for t in (float("nan"), 1.0, -0.1, float("inf")):
            with pytest.raises(_lib.RGCError, match="ji_threshold"):
                _raw(c, 1, [0, 2], [2, 5], boxes, t)
        with pytest.raises(_lib.RGCError, match="null argument"):
            _raw(c, *good, counts=False)
        with pytest.raises(_lib.RGCError, match="n_pairs out of range"):
            _raw(c, -1, [0, 2], [2, 5], boxes, 0.3)
        with pytest.raises(_lib.RGCError, match="n_pairs out of range"):
            _raw(c, 2 ** 31, [0, 2], [2, 5], boxes, 0.3)
        with pytest.raises(_lib.RGCError, match="negative box offset"):
            _raw(c, 1, [-1, 2], [2, 5], boxes, 0.3)
        with pytest.raises(_lib.RGCError, match="non-decreasing"):
            _raw(c, 2, [0, 2, 1], [2, 5, 5], boxes, 0.3)
        with pytest.raises(_lib.RGCError, match="non-decreasing"):
            _raw(c, 2, [0, 1, 2], [2, 5, 4], boxes, 0.3)
        with pytest.raises(_lib.RGCError, match="2\\^31 - 1 boxes"):
            _raw(c, 2, [0, 2 ** 30, 2 ** 31], [0, 0, 5], boxes, 0.3)
        for bad in ([2 ** 30 + 1, 2 ** 30 + 2, 0, 1], [0, 1, -2 ** 30 - 1, 0],
                    [0, 2 ** 25 + 1, 0, 1], [0, 1, -5, 2 ** 25]):
            with pytest.raises(_lib.RGCError, match="box 3 is out of range"):
                _raw(c, 1, [0, 2], [2, 5], boxes[:3] + [bad] + boxes[4:], 0.3)
        valid()
        assert _raw(c, 0, [0], [0], boxes, 0.3)[0].tolist() == [[-7, -7, -7]]    # no pairs: 0
        # a submitted run that awaits rgc_wait
        cfg = synth.SynthConfig(k=3, n_true=20, box=180, width=1024, height=1024, seed=5)
        b = Batch.pack(cfg.k, cfg.box, synth.batch(cfg, 2))
        c.submit(b.n_mg, cfg.k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score)
        with pytest.raises(_lib.RGCError, match="awaits rgc_wait"):
            _raw(c, *good)
        c.wait()
        valid()
    finally:
        c.close()


def test_timing_names_the_kernels():
    from repic_amd import score_detections as sd
    _, g, p, per_t = case("jitter")
    counts, ms = sd.match_pairs([(g, p)], 0.3, timing=True)
    assert counts.tolist() == [[300, 330, per_t[0][2]]]
    assert list(ms) == ["k_score_match_count", "k_score_match"]
    assert all(v > 0 for v in ms.values())
    counts, assign, ms = sd.match_pairs([(g, p)], 0.3, timing=True, assignment=True)
    assert "k_score_match" in ms and len(assign[0]) == 330


def test_no_pairs():
    from repic_amd import score_detections as sd
    c = sd.match_pairs([], 0.3)
    assert c.shape == (0, 3) and c.dtype == np.int64
    assert sd.match_pairs([], 0.3, assignment=True)[1] == [] and sd.match_scores([], 0.3) == []


# ---------------------------------------------------------------- command line
def test_command_line_match_ji(tmp_path):
    rng = np.random.default_rng(25)
    gdir, pdir = tmp_path / "gt", tmp_path / "pk"
    gdir.mkdir()
    pdir.mkdir()
    data = {}
    for i in range(4):
        n = 30 + 10 * i
        g = _sq(rng.integers(0, 900, (n, 2)), 64)
        p = _sq(g[rng.integers(0, n, n + 8), :2] + rng.integers(-25, 26, (n + 8, 2)), 64,
                rng.uniform(0, 1, n + 8).round(1))
        for d, a, nm in ((gdir, g, f"mg{i}.box"), (pdir, p, f"mg{i}_picked.box")):
            with open(d / nm, "w") as f:
                for r in a:
                    f.write(f"{int(r[0])}\t{int(r[1])}\t64\t64\t{float(r[4])!r}\n")
        data[f"mg{i}"] = (g, p)
    files = (["-g"] + [str(f) for f in sorted(gdir.iterdir())] +
             ["-p"] + [str(f) for f in sorted(pdir.iterdir())])
    env = dict(os.environ)
    env["PYTHONPATH"] = os.pathsep.join(
        [os.path.join(ROOT, "repic-copy_amd")] + [v for v in [env.get("PYTHONPATH")] if v])
    plain, matched = tmp_path / "plain", tmp_path / "matched"
    t = 0.4
    base = [sys.executable, "-m", "repic_amd.score_detections"] + files + ["-c", "0.3"]
    subprocess.run(base + ["--out_dir", str(plain)], check=True, env=env, timeout=300)
    subprocess.run(base + ["--out_dir", str(matched), "--match_ji", repr(t)], check=True, env=env,
                   timeout=300)
    assert sorted(f.name for f in plain.iterdir()) == ["particle_set_comp.tsv"]
    assert sorted(f.name for f in matched.iterdir()) == [
        "particle_set_comp.tsv", "particle_set_match.tsv", "particle_set_match_pooled.tsv"]
    assert ((matched / "particle_set_comp.tsv").read_bytes() ==
            (plain / "particle_set_comp.tsv").read_bytes())
    lines = (matched / "particle_set_match.tsv").read_text().splitlines()
    assert lines[0] == "filename\tji_thresh\tn_gt\tn_picked\ttp\tprecision\trecall\tf1"
    tot = np.zeros(3, np.int64)
    want = []
    for m in ("mg0", "mg1", "mg2", "mg3"):
        c, _ = oracle(*data[m], t, 0.3)
        tot += c
        want.append([m, repr(t)] + [str(v) for v in c + prf(*c)])
    assert [ln.split("\t") for ln in lines[1:]] == want
    assert 0 < tot[2] < tot[1] < sum(len(p) for _, p in data.values())
    lines = (matched / "particle_set_match_pooled.tsv").read_text().splitlines()
    assert lines[0] == "ji_thresh\tn_gt\tn_picked\ttp\tprecision\trecall\tf1"
    c = tuple(int(v) for v in tot)
    assert [ln.split("\t") for ln in lines[1:]] == [[repr(t)] + [str(v) for v in c + prf(*c)]]
