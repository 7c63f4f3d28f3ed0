"""Shared by the tests of the particle-level matching at every confidence threshold
(match_sweep): box builders, the per-threshold oracle (score_match_util.oracle once per
threshold) and a restatement of the average-precision formula."""
import numpy as np

from score_match_util import oracle, prf


def sq(xy, B, conf=None):
    """(n, 5) boxes x, y, B, B, conf of (n, 2) corners."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    c = np.ones(len(xy)) if conf is None else np.asarray(conf, dtype=np.float64)
    return np.concatenate([xy, np.full((len(xy), 2), float(B)), c[:, None]], axis=1)


def mixed(rng, n, field, lo, hi, neg=0):
    """Boxes of mixed sizes at .5 coordinates (round() goes to even), some at negative ones."""
    x = rng.integers(-2 * neg, 2 * field, n) / 2
    y = rng.integers(-2 * neg, 2 * field, n) / 2
    w = rng.integers(2 * lo, 2 * hi, n) / 2
    h = rng.integers(2 * lo, 2 * hi, n) / 2
    return np.stack([x, y, w, h, rng.uniform(0, 1, n)], axis=1)


def sweep_oracle(gt, pk, t, threshs):
    """(T, 3) int64 n_gt, n_picked, tp of one pair at every threshold, each from scratch."""
    return np.array([oracle(gt, pk, t, ct)[0] for ct in threshs], dtype=np.int64).reshape(-1, 3)


def check_sweep(got, pairs, t, threshs):
    """`got` (n_pairs, T, 3) equals the oracle at every pair and threshold; -> the oracle's."""
    want = np.stack([sweep_oracle(g, p, t, threshs) for g, p in pairs])
    assert got.dtype == np.int64 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    return want


def check_monotone(counts, threshs):
    """Per pair: tp and n_picked do not fall as the threshold falls, tp <= min(n_gt, n_picked)."""
    order = np.argsort(-np.asarray(threshs, dtype=np.float64), kind="stable")
    c = np.asarray(counts)[:, order, :]
    assert (np.diff(c[:, :, 2], axis=1) >= 0).all() and (np.diff(c[:, :, 1], axis=1) >= 0).all()
    assert (c[:, :, 2] <= np.minimum(c[:, :, 0], c[:, :, 1])).all()


def ap_formula(counts):
    """sum_i (R_i - R_(i-1)) P_i over the distinct rows by increasing n_picked, R_-1 = 0."""
    rows = sorted({(k, tp, g) for g, k, tp in np.asarray(counts).reshape(-1, 3).tolist()})
    ap, last = 0.0, 0.0
    for k, tp, g in rows:
        p, r, _ = prf(g, k, tp)
        ap += (r - last) * p
        last = r
    return ap
