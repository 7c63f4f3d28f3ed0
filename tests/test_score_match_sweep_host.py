"""Host side of the particle-level matching at every confidence threshold (no GPU): the new
symbol and its struct, average_precision on hand-made curves, the two TSV writers, the parser
and the errors raised before a device context exists."""
import ctypes
import os
import re

import numpy as np
import pytest

from score_match_util import prf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")


def test_header_declares_the_struct_and_the_symbol():
    from repic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "repic_gc.h")).read()
    assert "rgc_score_match_sweep" in set(re.findall(r"\b(rgc_[a-z_]+)\s*\(", hdr))
    assert re.search(r"typedef struct rgc_score_match_sweep_in \{\s*rgc_score_match_in pairs;[^}]*"
                     r"int32_t n_thr;[^}]*const int64_t\* keep;[^}]*\} rgc_score_match_sweep_in;", hdr)
    assert re.search(r"^#define\s+RGC_MATCH_MAX_THR\s+1024\s*$", hdr, re.M)
    assert re.search(r"^#define\s+RGC_ABI_VERSION\s+11\s*$", hdr, re.M) and _lib.abi_version() == 11


def test_symbol_is_exported_and_resolves():
    from repic_amd import _lib
    from repic_amd import score_detections as sd
    assert "rgc_score_match_sweep" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "rgc_score_match_sweep")
    # the binding's struct: rgc_score_match_in, then n_thr and keep
    assert [f[0] for f in sd.ScoreMatchSweepIn._fields_] == ["pairs", "n_thr", "keep"]
    assert sd.ScoreMatchSweepIn.pairs.size == ctypes.sizeof(sd.ScoreMatchIn)
    assert sd.ScoreMatchSweepIn.n_thr.offset == ctypes.sizeof(sd.ScoreMatchIn)
    assert sd.ScoreMatchSweepIn.keep.offset == ctypes.sizeof(sd.ScoreMatchIn) + 8


def test_average_precision_on_hand_made_curves():
    from repic_amd.score_detections import average_precision
    perfect = [[4, 1, 1], [4, 2, 2], [4, 4, 4]]
    assert average_precision(perfect) == 1.0 and type(average_precision(perfect)) is float
    assert average_precision(np.array(perfect, dtype=np.int64)) == 1.0
    assert average_precision([[4, 0, 0], [4, 3, 0], [4, 9, 0]]) == 0.0
    assert average_precision([[0, 0, 0]]) == 0.0 and average_precision([[0, 5, 0]]) == 0.0
    # three points, n_gt = 4: (P, R) = (1, 1/4), (1/2, 1/2), (3/10, 3/4)
    #   AP = 1/4 * 1 + (1/2 - 1/4) * 1/2 + (3/4 - 1/2) * 3/10 = 0.25 + 0.125 + 0.075 = 0.45
    three = [[4, 1, 1], [4, 4, 2], [4, 10, 3]]
    want = (0.25 - 0.0) * 1.0 + (0.5 - 0.25) * 0.5 + (0.75 - 0.5) * (3 / 10)
    assert average_precision(three) == want and abs(want - 0.45) < 1e-15
    # the rows in any order, duplicate thresholds collapsed, a threshold that adds no pick
    assert average_precision([three[2], three[0], three[1], three[0], three[2]]) == want
    # a single threshold: R * P
    assert average_precision([[4, 10, 3]]) == 0.75 * 0.3
    # a curve that starts with no pick kept
    assert average_precision([[4, 0, 0]] + three) == want


_COUNTS = np.array([[[4, 8, 2], [4, 2, 1], [4, 8, 2]],
                    [[0, 5, 0], [0, 0, 0], [0, 5, 0]],
                    [[6, 3, 3], [6, 1, 1], [6, 3, 3]]], dtype=np.int64)
_TS = [0.25, INF, 0.25]


def test_match_sweep_tsv_writers(tmp_path):
    from repic_amd import score_detections as sd
    sd.write_match_sweep_tsv(tmp_path / "m.tsv", ["mga", "mgb", "mgc"], 0.5, _TS, _COUNTS)
    lines = (tmp_path / "m.tsv").read_text().splitlines()
    assert lines[0] == ("filename\tji_thresh\tconf_thresh\tn_gt\tn_picked\ttp\tprecision\trecall"
                        "\tf1")
    want = [[m, "0.5", repr(float(t))] + [str(v) for v in tuple(c) + prf(*c)]
            for m, cs in zip(["mga", "mgb", "mgc"], _COUNTS.tolist()) for t, c in zip(_TS, cs)]
    assert [ln.split("\t") for ln in lines[1:]] == want
    assert lines[1].split("\t") == ["mga", "0.5", "0.25", "4", "8", "2", "0.25", "0.5",
                                    str(2 * 0.25 * 0.5 / 0.75)]
    assert lines[5].split("\t") == ["mgb", "0.5", "inf", "0", "0", "0", "0.0", "0.0", "0.0"]
    sd.write_match_sweep_pooled_tsv(tmp_path / "p.tsv", 0.5, _TS, _COUNTS)
    lines = (tmp_path / "p.tsv").read_text().splitlines()
    assert lines[0] == "ji_thresh\tconf_thresh\tn_gt\tn_picked\ttp\tprecision\trecall\tf1"
    tot = [(10, 16, 5), (10, 3, 2), (10, 16, 5)]
    assert [ln.split("\t") for ln in lines[1:4]] == [
        ["0.5", repr(float(t))] + [str(v) for v in c + prf(*c)] for t, c in zip(_TS, tot)]
    # per file: mga 1/4 * 1/2 + 1/4 * 1/4, mgb 0, mgc 1/6 * 1 + 2/6 * 1; pooled 2/10 * 2/3 + 3/10 * 5/16
    aps = [0.25 * 0.5 + (0.5 - 0.25) * 0.25, 0.0, (1 / 6) * 1.0 + (3 / 6 - 1 / 6) * 1.0]
    pooled = (2 / 10) * (2 / 3) + (5 / 10 - 2 / 10) * (5 / 16)
    assert lines[4] == f"# average_precision\t{sum(aps) / 3}\t{pooled}" and len(lines) == 5


def test_parser_takes_match_sweep_and_needs_match_ji(tmp_path, capsys):
    from repic_amd import score_detections as sd
    base = ["-g", str(tmp_path / "g.box"), "-p", str(tmp_path / "g_p.box")]
    a = sd._parser().parse_args(base)
    assert a.match_sweep is None
    a = sd._parser().parse_args(base + ["--match_ji", "0.4", "--match_sweep", "0.8", "0.2", "0.5"])
    assert a.match_sweep == [0.8, 0.2, 0.5] and a.match_ji == 0.4 and a.sweep is None and a.c is None
    with pytest.raises(SystemExit):
        sd._parser().parse_args(base + ["--match_ji", "0.4", "--match_sweep"])
    out = tmp_path / "never"
    with pytest.raises(SystemExit) as e:      # before --out_dir is made or a file is read
        sd.main(base + ["--match_sweep", "0.5", "--out_dir", str(out)])
    assert e.value.code == 2 and not out.exists()
    assert "--match_sweep needs --match_ji" in capsys.readouterr().err
    text = " ".join(sd._parser().format_help().split())
    assert "--match_sweep T [T ...]" in text and "particle_set_match_sweep_pooled.tsv" in text
    assert "not at the --sweep thresholds" not in text and "threshold only" not in text


def test_value_errors_before_any_device_call(monkeypatch, tmp_path):
    from repic_amd import _lib
    from repic_amd import score_detections as sd

    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(sd, "_ctx", no_ctx)
    monkeypatch.setattr(_lib, "Context", no_ctx)
    ok = np.array([[0., 0., 4., 4., 1.]])
    pair = [(ok, np.array([[1., 1., 4., 4., .5]]))]
    for fn in (sd.match_sweep, sd.match_curve):
        for ts in ([], [0.5, NAN], [NAN]):
            with pytest.raises(ValueError, match="conf_threshs"):
                fn(pair, 0.3, ts)
        for t in (-0.1, 1.0, NAN, INF):
            with pytest.raises(ValueError, match="ji_threshold"):
                fn(pair, t, [0.5])
        bad = ok.copy()
        bad[0, 2] = 2.0 ** 25 + 1
        with pytest.raises(ValueError, match="beyond"):
            fn([(ok, bad)], 0.3, [0.5])
        bad[0, 2] = NAN
        with pytest.raises(ValueError, match="cannot convert float NaN or infinity"):
            fn([(bad, ok)], 0.3, [0.5])
    files = ["-g", "a.box", "-p", "a_p.box", "--out_dir", str(tmp_path / "never")]
    with pytest.raises(ValueError, match="conf_threshs"):
        sd.main(files + ["--match_ji", "0.3", "--match_sweep", "nan"])
    with pytest.raises(ValueError, match="ji_threshold"):
        sd.main(files + ["--match_ji", "1.0", "--match_sweep", "0.5"])
    assert not (tmp_path / "never").exists()
