"""score_detections threshold sweep on the GPU (k_score_sweep through rgc_score_sweep): the
reference goldens bit for bit, parity with the looped single-threshold path and the oracle, and
the kernel's own edges (the 256-box scan chunk, the tiles, the 64-pixel words, the batch, the
threshold limit, the refusals), against numpy masks painted here.  Small shapes throughout: the
scores are ratios of exact pixel counts, so nothing has a tolerance."""
import ctypes as C
import warnings

import numpy as np
import pytest

from score_sweep_util import cases, oracle_scores, recs, same_as_golden, same_scores

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the C ABI, called directly
def _raw(fn_name, ctx, H, W, gts, pks, keep=None):
    """rgc_score_sweep (keep: (n_pairs, T)) or rgc_score_pairs (keep None) on per-pair slice
    arrays (r0, r1, c0, c1) -> the int64 counts."""
    from repic_amd import _lib
    from repic_amd import score_detections as sd
    # (hold: the arrays si points into)
    si, *hold = sd._score_in([np.asarray(g, np.int32).reshape(-1, 4) for g in gts],
                                  [np.asarray(p, np.int32).reshape(-1, 4) for p in pks],
                                  list(H), list(W), False)
    n = len(H)
    if keep is None:
        counts = np.zeros((n, 3), np.int64)
        _lib._check(_lib.lib.rgc_score_pairs(ctx._p, C.byref(si), counts.ctypes.data))
        return counts
    keep = np.ascontiguousarray(keep, dtype=np.int64).reshape(n, -1)
    T = keep.shape[1]
    counts = np.full((n, T, 3), -7, np.int64)
    sw = sd.ScoreSweepIn(si, T, keep.ctypes.data)
    _lib._check(getattr(_lib.lib, fn_name)(ctx._p, C.byref(sw), counts.ctypes.data))
    del hold
    return counts


def _sweep_raw(ctx, H, W, gts, pks, keep):
    return _raw("rgc_score_sweep", ctx, H, W, gts, pks, keep)


def _mask_counts(H, W, gt, pk, keep):
    """numpy masks: counts[j] of the picks pk[:keep[j]] (keep non-increasing)."""
    g = np.zeros((H, W), bool)
    for r0, r1, c0, c1 in np.asarray(gt).reshape(-1, 4):
        g[r0:r1, c0:c1] = True
    m = np.zeros((H, W), bool)
    out = np.zeros((len(keep), 3), np.int64)
    done = 0
    for j in range(len(keep) - 1, -1, -1):
        for r0, r1, c0, c1 in np.asarray(pk).reshape(-1, 4)[done:keep[j]]:
            m[r0:r1, c0:c1] = True
        done = max(done, keep[j])
        out[j] = g.sum(), m.sum(), (g & m).sum()
    return out


def _rand_slices(rng, n, H, W, smax):
    r0 = rng.integers(0, H, n)
    c0 = rng.integers(0, W, n)
    r1 = np.minimum(H, r0 + rng.integers(1, smax + 1, n))
    c1 = np.minimum(W, c0 + rng.integers(1, smax + 1, n))
    return np.stack([r0, r1, c0, c1], axis=1).astype(np.int32)


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import score_detections as sd
    return sd._ctx()


# ---------------------------------------------------------------- goldens and parity
def test_goldens_bit_for_bit():
    from repic_amd import score_detections as sd
    n = 0
    for case, g, p, ts in cases():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = sd.score_sweep([(recs(g), recs(p))], ts, **case["kwargs"])
        assert len(got) == 1 and len(got[0]) == len(ts)
        for j in range(len(ts)):
            same_as_golden(got[0][j], case, j)
            n += 1
    assert n == 63


def _mixed_pairs():
    rng = np.random.default_rng(3)
    pairs = []
    for i in range(24):
        W, H = int(rng.integers(64, 1500)), int(rng.integers(64, 1500))
        sz = int(rng.integers(4, 200))

        def mk(n):
            x = rng.uniform(-sz, W, n).round(1)
            y = rng.uniform(-sz, H, n).round(1)
            return np.stack([x, y, np.full(n, float(sz)), np.full(n, float(sz)),
                             rng.uniform(0, 1, n).round(1)], axis=1)
        pairs.append((mk(int(rng.integers(0, 60))), mk(int(rng.integers(1, 80)))))
    return pairs


def test_sweep_equals_looped_score_pairs_and_oracle():
    from repic_amd import score_detections as sd
    pairs = _mixed_pairs()
    ts = [0.4, 0.0, 0.9, 0.4, 1.5]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = sd.score_sweep(pairs, ts)
        loop = [sd.score_pairs(pairs, conf_thresh=t) for t in ts]
    assert len(got) == len(pairs)
    for i, (g, p) in enumerate(pairs):
        assert len(got[i]) == len(ts)
        for j, t in enumerate(ts):
            same_scores(got[i][j], loop[j][i], (i, t, "score_pairs"))
            same_scores(got[i][j], oracle_scores(g, p, t), (i, t, "oracle"))


def test_one_threshold_equals_score_pairs_counts(ctx):
    rng = np.random.default_rng(4)
    H, W = [300, 700, 64], [500, 129, 64]
    gts = [_rand_slices(rng, 30, h, w, 90) for h, w in zip(H, W)]
    pks = [_rand_slices(rng, n, h, w, 90) for n, h, w in zip((40, 300, 1), H, W)]
    keep = [[25], [300], [0]]
    got = _sweep_raw(ctx, H, W, gts, pks, keep)
    want = _raw(None, ctx, H, W, gts, [p[:k[0]] for p, k in zip(pks, keep)])
    assert np.array_equal(got[:, 0, :], want)
    for i in range(3):
        assert np.array_equal(got[i], _mask_counts(H[i], W[i], gts[i], pks[i], keep[i]))


# ---------------------------------------------------------------- segments and the scan chunk
def test_segment_edges_at_the_256_box_chunk(ctx):
    rng = np.random.default_rng(5)
    H, W = 400, 900
    gt = _rand_slices(rng, 50, H, W, 120)
    pk = _rand_slices(rng, 600, H, W, 40)
    keeps = [[600, 257, 256, 255, 1, 0],
             [600, 600, 300, 300, 300, 0],      # equal neighbours: empty segments
             [512, 512, 256, 256, 0, 0],
             [0, 0, 0, 0, 0, 0],
             [600, 600, 600, 600, 600, 600]]
    got = _sweep_raw(ctx, [H] * 5, [W] * 5, [gt] * 5, [pk] * 5, keeps)
    for i, k in enumerate(keeps):
        assert np.array_equal(got[i], _mask_counts(H, W, gt, pk, k)), k


# ---------------------------------------------------------------- tiles and words
def _edge_boxes(H, W):
    """Picks in level order (keep below gives each its own or a shared threshold)."""
    b = [[0, H, 0, W],                                  # the whole mask, highest level
         [H // 4, H // 2, W // 4, W // 2],              # inside it, lower level
         [3, 9, 60, 70],                                # straddles a 64-pixel word
         [5, 7, 62, 66],                                # inside the straddler, lower level
         [10, 20, 10, 64],                              # ends on a word boundary
         [10, 20, 64, min(128, W)],                     # starts on one
         [0, H, W - 1, W],                              # one pixel wide, last column
         [H - 1, H, 0, W],                              # one pixel high, every word
         [30, 40, 63, 64],                              # one pixel wide, last bit of a word
         [30, 40, 64, 65]]                              # ... first bit of the next
    return np.asarray(b, np.int32)


@pytest.mark.parametrize("which", ["wide", "tall", "both"])
def test_tile_and_word_edges(ctx, which):
    rng = np.random.default_rng(6)
    dims = {"wide": [(200, 2100)], "tall": [(3000, 100)], "both": [(200, 2100), (3000, 100)]}
    H = [d[0] for d in dims[which]]
    W = [d[1] for d in dims[which]]
    gts, pks, keeps = [], [], []
    for h, w in zip(H, W):
        e = _edge_boxes(h, w)
        r = _rand_slices(rng, 40, h, w, 300)
        # the whole-mask box first would hide everything after it: two orders, as two pairs
        pks += [np.concatenate([e[1:], r, e[:1]]), np.concatenate([e, r])]
        n = len(e) + len(r)
        keeps += [[n, n - 1, 30, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0],
                  [n, 40, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]]
        g = np.concatenate([_rand_slices(rng, 30, h, w, 200), [[0, h, 63, 65]]]).astype(np.int32)
        gts += [g, g]
    H2, W2 = np.repeat(H, 2).tolist(), np.repeat(W, 2).tolist()
    got = _sweep_raw(ctx, H2, W2, gts, pks, keeps)
    for i in range(len(H2)):
        assert np.array_equal(got[i], _mask_counts(H2[i], W2[i], gts[i], pks[i], keeps[i])), i


# ---------------------------------------------------------------- batches
def test_pairs_without_picks_or_ground_truth_in_one_launch():
    from repic_amd import score_detections as sd
    rng = np.random.default_rng(7)

    def mk(n, W=300, H=200, sz=30):
        return np.stack([rng.integers(-10, W, n), rng.integers(-10, H, n), np.full(n, sz),
                         np.full(n, sz), rng.uniform(0, 1, n).round(1)], axis=1).astype(float)
    none = np.zeros((0, 5))
    pairs = [(mk(20), mk(25)), (mk(20), none), (none, mk(25)), (mk(5), mk(300)), (mk(20), none)]
    ts = [0.5, 0.0, 1.0, 0.2]
    kw = {"mrc_w": 300, "mrc_h": 200}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = sd.score_sweep(pairs, ts, **kw)
        counts = sd.sweep_counts(pairs, ts, **kw)
    assert counts.shape == (5, 4, 3) and counts.dtype == np.int64
    assert (counts[1, :, 1:] == 0).all() and (counts[2, :, 0] == 0).all()
    assert (counts[:, :, 0] == counts[:, :1, 0]).all()
    for i, (g, p) in enumerate(pairs):
        for j, t in enumerate(ts):
            same_scores(got[i][j], oracle_scores(g, p, t, **kw), (i, t))


def test_no_pairs():
    from repic_amd import score_detections as sd
    c = sd.sweep_counts([], [0.1, 0.2, 0.3])
    assert c.shape == (0, 3, 3) and c.dtype == np.int64
    assert sd.score_sweep([], [0.5]) == []


# ---------------------------------------------------------------- limits and refusals
def test_1024_thresholds(ctx):
    from repic_amd import score_detections as sd
    rng = np.random.default_rng(8)
    H, W = 300, 330
    n = 1500
    gt = np.stack([rng.integers(0, W, 40), rng.integers(0, H, 40), np.full(40, 25),
                   np.full(40, 25), np.ones(40)], axis=1).astype(float)
    pk = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), np.full(n, 12),
                   np.full(n, 12), rng.uniform(0, 1, n)], axis=1).astype(float)
    ts = np.linspace(0.0, 1.0, 1024)
    got = sd.sweep_counts([(gt, pk)], ts, mrc_w=W, mrc_h=H)
    assert got.shape == (1, 1024, 3)
    order = np.argsort(-pk[:, 4], kind="stable")
    keep = [(~(pk[:, 4] < t)).sum() for t in ts]

    def sl(a):
        x, y, w, h = (a[:, k].astype(int) for k in range(4))
        return np.stack([y, np.minimum(y + h, H), x, np.minimum(x + w, W)], axis=1)
    assert np.array_equal(got[0], _mask_counts(H, W, sl(gt), sl(pk[order]), keep))


def test_refusals_leave_the_context_usable():
    from repic_amd import _lib
    rng = np.random.default_rng(9)
    c = _lib.Context(0)
    try:
        H, W = [100], [200]
        gt = [_rand_slices(rng, 10, 100, 200, 40)]
        pk = [_rand_slices(rng, 20, 100, 200, 40)]
        with pytest.raises(_lib.RGCError, match=r"n_thr 1025 is outside 1\.\.1024"):
            _sweep_raw(c, H, W, gt, pk, [[20] * 1025])
        with pytest.raises(_lib.RGCError, match=r"increases at threshold 2"):
            _sweep_raw(c, H, W, gt, pk, [[10, 5, 6, 0]])
        with pytest.raises(_lib.RGCError, match=r"keep\[0\]\[0\] = 21 is outside the pair's 20"):
            _sweep_raw(c, H, W, gt, pk, [[21, 5]])
        with pytest.raises(_lib.RGCError, match=r"keep\[0\]\[1\] = -1 is outside"):
            _sweep_raw(c, H, W, gt, pk, [[5, -1]])
        keep = [20, 7, 7, 0]
        got = _sweep_raw(c, H, W, gt, pk, [keep])
        assert np.array_equal(got[0], _mask_counts(100, 200, gt[0], pk[0], keep))
    finally:
        c.close()


# ---------------------------------------------------------------- command line
def _paint_counts(g, p, t):
    """(counts, area) of one pair as the oracle paints it (inferred dimensions)."""
    W = round(max(b[0] + b[2] for b in recs(g) + recs(p)))
    H = round(max(b[1] + b[3] for b in recs(g) + recs(p)))
    ga, pa = np.zeros((H, W), np.int16), np.zeros((H, W), np.int16)
    for b in recs(g):
        x, y, w, h = (round(v) for v in b[:4])
        ga[y:y + h, x:x + w] = 1
    for b in recs(p):
        if b[4] < t:
            continue
        x, y, w, h = (round(v) for v in b[:4])
        pa[y:y + h, x:x + w] = 1
    return np.array([ga.sum(), pa.sum(), (ga * pa).sum()], np.int64), H * W


def test_command_line_sweep(tmp_path):
    from repic_amd import score_detections as sd
    rng = np.random.default_rng(10)
    gdir, pdir = tmp_path / "gt", tmp_path / "pk"
    gdir.mkdir()
    pdir.mkdir()
    data = {}
    for i in range(3):
        g = np.stack([rng.integers(0, 900, 50), rng.integers(0, 900, 50), np.full(50, 64),
                      np.full(50, 64), rng.uniform(0, 1, 50)], axis=1)
        p = g.copy()
        p[:, :2] += rng.integers(-20, 20, (50, 2))
        p[:, 4] = rng.uniform(0, 1, 50).round(1)
        for d, a, nm in ((gdir, g, f"mg{i}.box"), (pdir, p, f"mg{i}_picked.box")):
            with open(d / nm, "w") as f:
                for r in a:
                    f.write(f"{int(r[0])}\t{int(r[1])}\t64\t64\t{float(r[4])!r}\n")
        data[f"mg{i}"] = (g.astype(float), p.astype(float))
    files = (["-g"] + [str(f) for f in sorted(gdir.iterdir())] +
             ["-p"] + [str(f) for f in sorted(pdir.iterdir())])
    ts = [0.5, 0.0, 0.9, 0.5, 2.0]
    plain, swept = tmp_path / "plain", tmp_path / "swept"
    sd.main(files + ["-c", "0.2", "--out_dir", str(plain)])
    sd.main(files + ["-c", "0.2", "--out_dir", str(swept), "--sweep"] + [repr(t) for t in ts])
    assert sorted(f.name for f in plain.iterdir()) == ["particle_set_comp.tsv"]
    assert sorted(f.name for f in swept.iterdir()) == [
        "particle_set_comp.tsv", "particle_set_sweep.tsv", "particle_set_sweep_pooled.tsv"]
    assert ((swept / "particle_set_comp.tsv").read_bytes() ==
            (plain / "particle_set_comp.tsv").read_bytes())
    lines = (swept / "particle_set_sweep.tsv").read_text().splitlines()
    assert lines[0] == "filename\tconf_thresh\tprecision\trecall\tf1\tpos_frac"
    want = [[m, repr(float(t))] + [str(v) for v in oracle_scores(*data[m], t)]
            for m in ("mg0", "mg1", "mg2") for t in ts]
    assert [ln.split("\t") for ln in lines[1:]] == want
    lines = (swept / "particle_set_sweep_pooled.tsv").read_text().splitlines()
    assert lines[0] == ("conf_thresh\tprecision\trecall\tf1\tpos_frac\tgt_pixels\t"
                        "picked_pixels\ttp_pixels")
    assert len(lines) == 1 + len(ts)
    for t, ln in zip(ts, lines[1:]):
        tot, area = np.zeros(3, np.int64), 0
        for m in data:
            c, a = _paint_counts(*data[m], t)
            tot += c
            area += a
        g, k, tp = (np.int64(v) for v in tot)
        prec = 0.0 if (tp == k == 0.0) else tp / k
        rec = tp / g
        f1 = 0.0 if (prec == rec == 0.0) else (2 * prec * rec) / (prec + rec)
        assert ln.split("\t") == [repr(float(t)), str(prec), str(rec), str(f1), str(k / area),
                                  str(g), str(k), str(tp)]
