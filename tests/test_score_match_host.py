"""Host side of the particle-level matching of score_detections (no GPU): the edge test the
kernel uses (rgc_test_iou_edge) against the edges the real reference recorded
(tests/golden/make_score_match_golden.py) and against a numpy restatement, the two symbols, the
parser, the ValueErrors raised before a device context exists, the score formulas and the two
TSV writers."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from score_match_util import cases, edge_matrix, prf, rects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_edge_test_equals_every_reference_edge_and_non_edge():
    from repic_amd.score_detections import iou_edge
    seen = 0
    for name, g, p, per_t in cases():
        gr, pr = rects(g).tolist(), rects(p).tolist()
        for t, edges, _ in per_t:
            got = {(i, j) for i, a in enumerate(gr) for j, b in enumerate(pr) if iou_edge(a, b, t)}
            assert got == edges, (name, t, sorted(got ^ edges)[:5])
            seen += len(edges)
    assert seen == 599 + 506 + 859 + 122 + (1 + 3 + 3 + 5)


def test_ties_values_are_decided_by_one_f64_division():
    from repic_amd.score_detections import iou_edge
    a = [0, 10, 0, 10]
    five, six = [5, 15, 0, 10], [0, 10, -6, 4]
    third = 1.0 / 3.0
    assert 50 / 150 == third and 40 / 160 == 0.25
    assert not iou_edge(a, five, third) and iou_edge(a, five, math.nextafter(third, 0.0))
    assert not iou_edge(a, six, 0.25) and iou_edge(a, six, math.nextafter(0.25, 0.0))
    assert iou_edge(a, a, math.nextafter(1.0, 0.0)) and iou_edge(a, [9, 19, 9, 19], 0.0)
    assert not iou_edge(a, [10, 20, 0, 10], 0.0)          # touching: I = 0
    for none in ([3, 3, 0, 10], [3, 2, 0, 10], [0, 10, 4, 4], [0, 10, 5, 1]):
        assert not iou_edge(a, none, 0.0) and not iou_edge(none, a, 0.0)
        assert not iou_edge(none, none, 0.0)


def test_edge_test_equals_numpy_restatement_on_random_rectangles():
    from repic_amd.score_detections import _match_rects, iou_edge
    rng = np.random.default_rng(11)
    n = 0
    for lim, smax, ts in ((60, 40, [0.0, 0.1, 0.3, 1 / 3, 0.5, 0.9]),
                          (2 ** 30 - 2 ** 25, 2 ** 25, [0.0, 0.3, 0.75])):
        def mk(k):
            x = rng.integers(-2 * lim, 2 * lim + 1, k) / 2        # .5 values go through round()
            y = rng.integers(-2 * lim, 2 * lim + 1, k) / 2
            w = rng.integers(-2, 2 * smax + 1, k) / 2             # mixed sizes, some without a pixel
            h = rng.integers(-2, 2 * smax + 1, k) / 2
            return np.stack([x, y, w, h], axis=1)
        g, p = mk(70), mk(70)
        if lim > 60:      # far apart boxes never meet: put the picks near the ground truth
            p[:, :2] = g[:, :2] + rng.integers(-smax, smax, (70, 2))
            p[:, :2] = np.clip(p[:, :2], -lim, lim)
        gr, pr = rects(g), rects(p)
        lib = _match_rects(*g.T)
        assert lib.dtype == np.int32
        keep = (gr[:, 1] > gr[:, 0]) & (gr[:, 3] > gr[:, 2])
        assert np.array_equal(lib[keep], gr[keep])               # the library's rounding
        assert (lib[~keep, 0] == lib[~keep, 1]).all() and (lib[~keep, 2] == lib[~keep, 3]).all()
        for t in ts:
            E = edge_matrix(gr, pr, t)
            got = np.array([[iou_edge(a, b, t) for b in pr.tolist()] for a in gr.tolist()])
            assert np.array_equal(got, E), (lim, t)
            n += int(E.sum())
    assert n > 100


def test_header_exports_and_library_agree_on_the_symbols():
    from repic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "repic_gc.h")).read()
    decl = set(re.findall(r"\b(rgc_[a-z_]+)\s*\(", hdr))
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rgc_score_match", "rgc_test_iou_edge"):
        assert name in decl and name in _lib.EXPORTS and hasattr(so, name), name
    assert re.search(r"typedef struct rgc_score_match_in \{[^}]*double ji_threshold;[^}]*\}", hdr)
    assert re.search(r"^#define\s+RGC_ABI_VERSION\s+11\s*$", hdr, re.M) and _lib.abi_version() == 11


def test_parser_takes_match_ji():
    from repic_amd.score_detections import _parser
    a = _parser().parse_args(["-g", "g.box", "-p", "p.box"])
    assert a.match_ji is None
    a = _parser().parse_args(["-g", "g.box", "-p", "p.box", "-c", "0.2", "--match_ji", "0.5"])
    assert a.match_ji == 0.5 and a.c == 0.2 and a.sweep is None
    with pytest.raises(SystemExit):
        _parser().parse_args(["-g", "g.box", "-p", "p.box", "--match_ji"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["-g", "g.box", "-p", "p.box", "--match_ji", "x"])
    assert "--sweep" in _parser().format_help() and "--match_ji" in _parser().format_help()


def test_value_errors_before_any_device_call(monkeypatch):
    from repic_amd import _lib
    from repic_amd import score_detections as sd

    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(sd, "_ctx", no_ctx)
    monkeypatch.setattr(_lib, "Context", no_ctx)
    ok = np.array([[0., 0., 4., 4., 1.]])
    pair = [(ok, np.array([[1., 1., 4., 4., .5]]))]
    for fn in (sd.match_pairs, sd.match_scores):
        for t in (-0.1, 1.0, NAN, INF):
            with pytest.raises(ValueError, match="ji_threshold"):
                fn(pair, t)
        for col, v in ((0, 2.0 ** 30 + 1), (1, -(2.0 ** 30) - 1), (2, 2.0 ** 25 + 1),
                       (3, 2.0 ** 25 + 1), (0, 1e300), (3, 1e300)):
            bad = ok.copy()
            bad[0, col] = v
            with pytest.raises(ValueError, match=r"beyond"):
                fn([(bad, ok)], 0.3)
            with pytest.raises(ValueError, match=r"beyond"):
                fn([(ok, bad)], 0.3)
        for v in (NAN, INF, -INF):
            bad = ok.copy()
            bad[0, 1] = v
            with pytest.raises(ValueError, match="cannot convert float NaN or infinity"):
                fn([(ok, bad)], 0.3)
    with pytest.raises(ValueError, match="ji_threshold"):
        sd.main(["-g", "a.box", "-p", "a_p.box", "--match_ji", "1.0"])
    # the limits themselves pass the checks (a huge negative size is a box without a pixel)
    edge = np.array([[2.0 ** 30, -(2.0 ** 30), 2.0 ** 25, 2.0 ** 25, 1.], [0., 0., -1e300, 5., 1.]])
    assert sd._match_rects(*edge[:, :4].T).tolist() == [
        [2 ** 30, 2 ** 30 + 2 ** 25, -2 ** 30, -2 ** 30 + 2 ** 25], [0, 0, 0, 0]]


def test_score_formulas_at_zero_denominators():
    from repic_amd.score_detections import _prf
    assert _prf(0, 0, 0) == (0.0, 0.0, 0.0)
    assert _prf(5, 0, 0) == (0.0, 0.0, 0.0)
    assert _prf(0, 7, 0) == (0.0, 0.0, 0.0)
    assert _prf(5, 7, 0) == (0.0, 0.0, 0.0)
    assert _prf(4, 8, 2) == (0.25, 0.5, 2 * 0.25 * 0.5 / 0.75)
    assert _prf(3, 3, 3) == (1.0, 1.0, 1.0)
    for v in _prf(np.int64(4), np.int64(8), np.int64(2)):
        assert type(v) is float
    for args in ((0, 0, 0), (5, 0, 0), (4, 8, 2), (10, 3, 3)):
        assert _prf(*args) == prf(*args)


_COUNTS = np.array([[4, 8, 2], [0, 5, 0], [6, 0, 0]], dtype=np.int64)


def test_match_tsv_writers(tmp_path):
    from repic_amd import score_detections as sd
    t = math.nextafter(1 / 3, 0.0)
    sd.write_match_tsv(tmp_path / "m.tsv", ["mga", "mgb", "mgc"], t, _COUNTS)
    lines = (tmp_path / "m.tsv").read_text().splitlines()
    assert lines[0] == "filename\tji_thresh\tn_gt\tn_picked\ttp\tprecision\trecall\tf1"
    assert [ln.split("\t") for ln in lines[1:]] == [
        ["mga", repr(t), "4", "8", "2", "0.25", "0.5", str(2 * 0.25 * 0.5 / 0.75)],
        ["mgb", repr(t), "0", "5", "0", "0.0", "0.0", "0.0"],
        ["mgc", repr(t), "6", "0", "0", "0.0", "0.0", "0.0"]]
    sd.write_match_pooled_tsv(tmp_path / "p.tsv", 0.5, _COUNTS)
    lines = (tmp_path / "p.tsv").read_text().splitlines()
    assert lines[0] == "ji_thresh\tn_gt\tn_picked\ttp\tprecision\trecall\tf1"
    p, r, f = prf(10, 13, 2)
    assert [ln.split("\t") for ln in lines[1:]] == [["0.5", "10", "13", "2", str(p), str(r), str(f)]]
