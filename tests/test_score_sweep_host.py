"""Host side of the score_detections threshold sweep (no GPU): the ordering of the picks and
the keep table against brute force, the parser, the two TSV writers from synthetic counts, the
ValueErrors, and the oracle looped over the thresholds against the goldens the real reference
produced (tests/golden/make_score_sweep_golden.py), which pins them here."""
import numpy as np
import pytest

from score_sweep_util import cases, oracle_scores, same_as_golden

INF = float("inf")
NAN = float("nan")


def test_oracle_looped_over_thresholds_matches_reference_golden():
    n = 0
    for case, g, p, ts in cases():
        for j, t in enumerate(ts):
            same_as_golden(oracle_scores(g, p, t, **case["kwargs"]), case, j)
            n += 1
    assert n == 6 + 11 + 5 + 6 + 3 + 32


def _brute_kept(conf, t):
    return [not (c < t) for c in conf]          # score_detections.py:34-36


@pytest.mark.parametrize("conf, ts", [
    ([0.1, 0.5, 0.5, 0.9, 0.3], [0.0, 0.5, 1.0]),
    ([0.5, 0.5, 0.5], [0.5]),                                   # every pick on the threshold
    ([0.2, NAN, 0.7, NAN], [0.1, 0.5, INF]),                    # NaN is kept even at +inf
    ([-INF, INF, 0.0, -0.0, 1.0], [-INF, 0.0, 1.0, INF]),
    ([0.3, 0.1, 0.2], [0.3, 0.1, 0.2, 0.1, 0.3]),               # unsorted, duplicated
    ([], [0.5, 0.7]),
    ([0.4], [2.0]),                                             # nothing kept
    (np.round(np.random.default_rng(0).uniform(0, 1, 300) * 10) / 10, (np.arange(11) / 10)),
    (np.random.default_rng(1).uniform(0, 1, 257), np.random.default_rng(2).uniform(0, 1, 40)),
])
def test_sweep_plan_against_brute_force(conf, ts):
    from repic_amd.score_detections import _check_threshs, _sweep_plan
    conf = np.asarray(conf, dtype=np.float64)
    ts = _check_threshs(ts)
    uniq, inv = np.unique(ts, return_inverse=True)
    assert np.all(np.diff(uniq) > 0)
    order, keep = _sweep_plan(conf, uniq)
    assert sorted(order.tolist()) == list(range(len(conf)))
    assert keep.dtype == np.int64 and keep.shape == (len(uniq),)
    assert np.all(np.diff(keep) <= 0) and (len(conf) >= keep).all() and (keep >= 0).all()
    level = np.array([sum(_brute_kept([c], t)[0] for t in uniq) for c in conf], dtype=np.int64)
    ol = level[order]
    assert np.all(np.diff(ol) <= 0)                              # level descending ...
    for a, b in zip(order[:-1], order[1:]):                      # ... and stable
        assert level[a] > level[b] or a < b
    for j, t in enumerate(uniq):                                 # the kept picks are the prefix
        kept = _brute_kept(conf, t)
        assert keep[j] == sum(kept)
        assert sorted(order[:keep[j]].tolist()) == [i for i, k in enumerate(kept) if k]
    for j, t in enumerate(ts):                                   # the caller's order comes back
        assert uniq[inv.reshape(-1)[j]] == t


def test_threshold_errors_before_any_device_call(monkeypatch):
    from repic_amd import _lib
    from repic_amd import score_detections as sd

    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(sd, "_ctx", no_ctx)
    monkeypatch.setattr(_lib, "Context", no_ctx)
    pair = [(np.array([[0., 0., 4., 4., 1.]]), np.array([[1., 1., 4., 4., .5]]))]
    for fn in (sd.sweep_counts, sd.score_sweep):
        with pytest.raises(ValueError, match="empty"):
            fn(pair, [])
        with pytest.raises(ValueError, match="NaN"):
            fn(pair, [0.5, NAN])
    with pytest.raises(ValueError, match="NaN"):
        sd.main(["-g", "a.box", "-p", "a_p.box", "--sweep", "0.1", "nan"])
    assert sd._check_threshs([INF, -INF, 0.25, 0.25]).tolist() == [INF, -INF, 0.25, 0.25]


def test_parser():
    from repic_amd.score_detections import _parser
    a = _parser().parse_args(["-g", "g.box", "-p", "p.box"])
    assert a.sweep is None and a.c is None
    a = _parser().parse_args(["-g", "g.box", "-p", "p.box", "-c", "0.3", "--sweep", "0.5", "0",
                              "1e-3", "inf", "0.5"])
    assert a.c == 0.3 and a.sweep == [0.5, 0.0, 1e-3, INF, 0.5]
    a = _parser().parse_args(["--sweep", "-1", "--out_dir", "o", "-g", "g.box", "-p", "p.box"])
    assert a.sweep == [-1.0] and a.out_dir == "o"
    with pytest.raises(SystemExit):
        _parser().parse_args(["-g", "g.box", "-p", "p.box", "--sweep"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["-g", "g.box", "-p", "p.box", "--sweep", "x"])


# synthetic counts: 2 pairs x 3 thresholds x (gt, picked, tp)
_COUNTS = np.array([[[100, 80, 40], [100, 10, 10], [100, 0, 0]],
                    [[0, 50, 0], [0, 50, 0], [0, 0, 0]]], dtype=np.int64)
_H, _W = np.array([20, 10]), np.array([30, 40])
_TS = [0.0, 0.5, INF]


def test_sweep_tsv_writer(tmp_path):
    from repic_amd import score_detections as sd
    path = tmp_path / "particle_set_sweep.tsv"
    with np.errstate(all="ignore"):
        sd.write_sweep_tsv(path, ["mga", "mgb"], _TS, _COUNTS, _H, _W)
        want = [[m, repr(float(t))] + [str(v) for v in sd._scores(_COUNTS[i][j], int(_H[i]),
                                                                 int(_W[i]))]
                for i, m in enumerate(["mga", "mgb"]) for j, t in enumerate(_TS)]
    lines = path.read_text().splitlines()
    assert lines[0] == "filename\tconf_thresh\tprecision\trecall\tf1\tpos_frac"
    assert [ln.split("\t") for ln in lines[1:]] == want
    # grouped by file, thresholds in the order given; spot values
    assert [ln.split("\t")[:2] for ln in lines[1:]] == [
        ["mga", "0.0"], ["mga", "0.5"], ["mga", "inf"], ["mgb", "0.0"], ["mgb", "0.5"],
        ["mgb", "inf"]]
    assert lines[1].split("\t")[2:] == ["0.5", "0.4", str(2 * .5 * .4 / (.5 + .4)),
                                        str(80 / 600)]
    assert lines[3].split("\t")[2:] == ["0.0", "0.0", "0.0", "0.0"]       # the 0.0 branches
    assert lines[4].split("\t")[2:] == ["0.0", "nan", "nan", "0.125"]     # no ground truth


def test_sweep_pooled_tsv_writer(tmp_path):
    from repic_amd import score_detections as sd
    path = tmp_path / "particle_set_sweep_pooled.tsv"
    sd.write_sweep_pooled_tsv(path, _TS, _COUNTS, _H, _W)
    lines = path.read_text().splitlines()
    assert lines[0] == ("conf_thresh\tprecision\trecall\tf1\tpos_frac\tgt_pixels\t"
                        "picked_pixels\ttp_pixels")
    assert len(lines) == 4
    area = 20 * 30 + 10 * 40
    for j, ln in enumerate(lines[1:]):
        g, k, tp = (np.int64(v) for v in _COUNTS[:, j, :].sum(axis=0))
        prec = 0.0 if (tp == k == 0.0) else tp / k
        rec = tp / g
        f1 = 0.0 if (prec == rec == 0.0) else (2 * prec * rec) / (prec + rec)
        assert ln.split("\t") == [repr(float(_TS[j])), str(prec), str(rec), str(f1),
                                  str(k / area), str(g), str(k), str(tp)]
    assert lines[1].split("\t")[4:] == ["0.13", "100", "130", "40"]
    assert lines[3].split("\t")[1:5] == ["0.0", "0.0", "0.0", "0.0"]
