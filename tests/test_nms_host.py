"""Host side of the greedy NMS feature, without a device: ``nms_order``, the ``repic nms``
command's file handling (with ``nms.nms_keep`` replaced by the CPU oracle), the refusals of
``consensus --dedup_ji`` before any side effect, and the dispatcher."""
import argparse
import os

import numpy as np
import pytest

import nms_util
from repic_amd import _lib, main as repic_main, nms
from repic_amd.commands import consensus, nms as nms_cmd


# ----------------------------------------------------------------------------- nms_order
def test_nms_order_nan_last_and_descending():
    s = np.array([0.5, np.nan, 2.0, -1.0, np.nan, 3.0, -np.inf, np.inf])
    assert nms.nms_order(s).tolist() == [7, 5, 2, 0, 3, 6, 1, 4]


def test_nms_order_signed_zero_tie_and_stability():
    s = np.array([0.0, -0.0, 1.0, -0.0, 0.0, 1.0, 1.0])
    assert nms.nms_order(s).tolist() == [2, 5, 6, 0, 1, 3, 4]
    assert nms.nms_order(np.zeros(0)).tolist() == []
    assert nms.nms_order([7]).tolist() == [0]


def test_oracle_threshold_boundary():
    """The hand values of the contract, box 10: area 50 is JI = 50/150 == 1/3 in f64 (kept at
    T = 1/3, suppressed at 0.3); area 45 is kept at 0.3; area 48 is suppressed at 0.3."""
    assert nms_util.jaccard(0.0, 0.0, 5.0, 0.0, 10.0) == 1 / 3
    assert nms_util.nms_oracle([0, 5], [0, 0], 10, 1 / 3).tolist() == [True, True]
    assert nms_util.nms_oracle([0, 5], [0, 0], 10, 0.3).tolist() == [True, False]
    assert nms_util.nms_oracle([0, 5], [0, 1], 10, 0.3).tolist() == [True, True]
    assert nms_util.nms_oracle([0, 4], [0, 2], 10, 0.3).tolist() == [True, False]
    ic = _lib.ji_cutoff(10, 0.3)[0]
    assert 45 <= ic < 48
    assert nms_util.characterised([0, 5, 4], [0, 1, 2], [1, 1, 0], 10, 0.3) is None
    assert nms_util.characterised([0, 5, 4], [0, 1, 2], [1, 1, 1], 10, 0.3) == 2


# ----------------------------------------------------------------------------- repic nms
HEAD = b"x y w h conf\n"


def _line(x, y, s, end=b"\n"):
    return f"{x}\t{y}\t10\t10\t{s}".encode() + end


def _make_inputs(root):
    a, b = root / "in" / "pickA", root / "in" / "pickB"
    a.mkdir(parents=True)
    b.mkdir()
    (root / "in" / ".hidden").mkdir()
    files = {}
    # header; the second line (highest score) suppresses the first and the fourth
    files["pickA", "m1.box"] = HEAD + _line(0, 0, 0.5) + _line(1, 1, 0.9) + \
        _line(40, 40, 0.1) + _line(2, 0, 0.7) + _line(100, 0, 0.2)
    # CRLF endings, no header, no final newline; the last line is kept
    files["pickA", "m2.box"] = _line(0, 0, 0.9, b"\r\n") + _line(1, 0, 0.8, b"\r\n") + \
        _line(50, 50, 0.7, b"")
    # no final newline and the last line suppressed
    files["pickA", "m3.box"] = _line(0, 0, 0.9) + _line(30, 0, 0.5) + _line(1, 0, 0.8, b"")
    # negative scores stay raw (no sigmoid): -1 outranks -2
    files["pickB", "m1.box"] = _line(0, 0, -2.0) + _line(1, 0, -1.0)
    # copied verbatim: a non-float x token, an empty file, a 4-column file
    files["pickB", "m2.box"] = _line(0, 0, 0.9) + _line("abc", 0, 0.8) + _line(1, 0, 0.7)
    files["pickB", "m3.box"] = b""
    files["pickB", "m4.box"] = b"0 0 10 10\n1 0 10 10\n"
    for (m, f), raw in files.items():
        (root / "in" / m / f).write_bytes(raw)
    (a / ".hidden.box").write_bytes(_line(0, 0, 1))
    (a / "notes.txt").write_text("not a box file\n")
    return files


def _nms_args(root, **kw):
    a = argparse.Namespace(in_dir=str(root / "in"), out_dir=str(root / "out"), box_size=10,
                           ji_threshold=0.3, threads=None, device=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_repic_nms_files(tmp_path, monkeypatch):
    files = _make_inputs(tmp_path)
    monkeypatch.setattr(nms, "nms_keep", nms_util.oracle_keep_list)
    nms_cmd.main(_nms_args(tmp_path))
    out = tmp_path / "out"
    got = {(m, f): (out / m / f).read_bytes() for (m, f) in files}
    assert sorted(os.listdir(out)) == ["nms_summary.tsv", "pickA", "pickB"]
    assert sorted(os.listdir(out / "pickA")) == ["m1.box", "m2.box", "m3.box"]
    assert got["pickA", "m1.box"] == HEAD + _line(1, 1, 0.9) + _line(40, 40, 0.1) + \
        _line(100, 0, 0.2)
    assert got["pickA", "m2.box"] == _line(0, 0, 0.9, b"\r\n") + _line(50, 50, 0.7, b"")
    assert got["pickA", "m3.box"] == _line(0, 0, 0.9) + _line(30, 0, 0.5)
    assert got["pickB", "m1.box"] == _line(1, 0, -1.0)
    for f in ("m2.box", "m3.box", "m4.box"):
        assert got["pickB", f] == files["pickB", f]
    rows = (out / "nms_summary.tsv").read_text().splitlines()
    assert rows[0] + "\n" == nms_cmd.SUMMARY_HEADER == "picker\tfile\tstatus\tboxes\tkept\n"
    assert [r.split("\t") for r in rows[1:]] == [
        ["pickA", "m1.box", "filtered", "5", "3"],
        ["pickA", "m2.box", "filtered", "3", "2"],
        ["pickA", "m3.box", "filtered", "3", "2"],
        ["pickB", "m1.box", "filtered", "2", "1"],
        ["pickB", "m2.box", "copied", "0", "0"],
        ["pickB", "m3.box", "copied", "0", "0"],
        ["pickB", "m4.box", "copied", "0", "0"]]
    # every kept line is a line of the input, in the input's order
    for key, raw in files.items():
        src = raw.splitlines(keepends=True)
        it = iter(src)
        assert all(any(ln == s for s in it) for ln in got[key].splitlines(keepends=True)), key


def test_repic_nms_refuses_non_empty_out_dir(tmp_path, monkeypatch):
    _make_inputs(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    (out / "keep.txt").write_text("x")

    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", no_ctx)
    monkeypatch.setattr(nms, "nms_keep", no_ctx)
    with pytest.raises(_lib.RGCError, match="not an empty directory"):
        nms_cmd.main(_nms_args(tmp_path))
    assert os.listdir(out) == ["keep.txt"] and (out / "keep.txt").read_text() == "x"


def test_repic_nms_accepts_empty_out_dir_and_bad_threshold(tmp_path, monkeypatch):
    _make_inputs(tmp_path)
    monkeypatch.setattr(nms, "nms_keep", nms_util.oracle_keep_list)
    with pytest.raises(ValueError):
        nms_cmd.main(_nms_args(tmp_path, ji_threshold=1.0))
    assert not (tmp_path / "out").exists()
    (tmp_path / "out").mkdir()
    nms_cmd.main(_nms_args(tmp_path))
    assert (tmp_path / "out" / "nms_summary.tsv").exists()


def test_repic_nms_world_size_refused(tmp_path, monkeypatch):
    _make_inputs(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(_lib.RGCError, match="WORLD_SIZE"):
        nms_cmd.main(_nms_args(tmp_path))
    assert not (tmp_path / "out").exists()


# ----------------------------------------------------------------------------- consensus --dedup_ji
def _consensus_args(in_dir, out_dir, **kw):
    a = argparse.Namespace(in_dir=str(in_dir), out_dir=str(out_dir), box_size=180,
                           num_particles=None, get_cc=False, node_limit=0,
                           batch_boxes=1 << 25, threads=None, device=None, listing=None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw, exc, match", [
    (dict(dedup_ji=0.3, members=True), _lib.RGCError, "--members"),
    (dict(dedup_ji=1.0), ValueError, "ji_threshold"),
    (dict(dedup_ji=float("nan")), ValueError, "ji_threshold"),
])
def test_dedup_refusals_before_any_side_effect(tmp_path, monkeypatch, kw, exc, match):
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    (in_dir / "a").mkdir(parents=True)
    out_dir.mkdir()
    sentinel = out_dir / "keep.txt"
    sentinel.write_text("x")

    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", no_ctx)
    with pytest.raises(exc, match=match):
        consensus.main(_consensus_args(in_dir, out_dir, **kw))
    assert sentinel.read_text() == "x"


def test_dedup_option_parses():
    import argparse as ap
    p = ap.ArgumentParser()
    consensus.add_arguments(p)
    assert p.parse_args(["i", "o", "10"]).dedup_ji is None
    assert p.parse_args(["i", "o", "10", "--dedup_ji", "0.25"]).dedup_ji == 0.25
    with pytest.raises(SystemExit):
        p.parse_args(["i", "o", "10", "--dedup_ji", "1.5"])
    assert consensus.dedup_ji_of(argparse.Namespace()) is None


# ----------------------------------------------------------------------------- dispatcher
def test_dispatcher_nms_help(capsys):
    with pytest.raises(SystemExit) as e:
        repic_main.main(["nms", "-h"])
    assert e.value.code == 0
    assert "--ji_threshold" in capsys.readouterr().out
