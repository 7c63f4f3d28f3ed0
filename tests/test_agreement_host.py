"""Host side of the picker-agreement feature, without a device: the oracle of the contract
(agree_util) against the reference's edges and the issue's totals on the committed fixture, the
hand cases of the rule, the ``repic agreement`` command with the device call replaced by the
oracle, its refusals before any side effect, the dispatcher and the library's symbols."""
import argparse
import os

import numpy as np
import pytest

import agree_util as au
import vote_util as vu
from oracle import cpu_ref
from repic_amd import _lib, agreement as ag, main as repic_main
from repic_amd.commands import agreement as ag_cmd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ----------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def c1():
    methods, bases, mgs = vu.load_dir(os.path.join(GOLDEN, "inputs_10017"))
    n_mg, off, x, y = au.pack(3, [[(a, b) for a, b, _ in mg] for mg in mgs])
    r = au.oracle(n_mg, 3, 180, off, x, y, 0.3)
    return methods, mgs, n_mg, off, x, y, r


def test_oracle_edges_are_the_references(c1):
    """Per micrograph and ordered picker pair, the oracle's joined pairs and their JI are
    ``cpu_ref.edges_vectorised``'s, bit for bit."""
    methods, mgs, n_mg, off, x, y, r = c1
    assert cpu_ref.THRESHOLD == 0.3
    for m, mg in enumerate(mgs):
        lists = [[(float(a), float(b), 0.0, i) for i, (a, b) in enumerate(zip(px, py))]
                 for px, py, _ in mg]
        for p in range(3):
            for q in range(3):
                if p == q:
                    continue
                want = sorted(cpu_ref.edges_vectorised(lists[p], lists[q], 180))
                i, j, ji = au.pair_edges_window(mg[p][0], mg[p][1], mg[q][0], mg[q][1], 180, 0.3)
                assert list(zip(i.tolist(), j.tolist(), ji.tolist())) == want, (m, p, q)
                assert r.pair_edges[m, p, q] == len(want)


def test_oracle_totals_on_the_fixture(c1):
    methods, mgs, n_mg, off, x, y, r = c1
    assert methods == ["crYOLO", "deepPicker", "topaz"]
    pick = ag.box_pickers(off, 3)
    assert np.bincount(pick).tolist() == [8908, 3964, 9518]
    assert r.pair_supported.sum(0).tolist() == [[0, 3160, 8777], [2693, 0, 2902], [7951, 3109, 0]]
    assert r.pair_edges.sum(0).tolist() == [[0, 3477, 10006], [3477, 0, 3398], [10006, 3398, 0]]
    assert r.pair_mutual.sum(0).tolist() == [[0, 2588, 7885], [2588, 0, 2779], [7885, 2779, 0]]
    assert ag.venn_counts(r.support, pick, 3).tolist() == [
        [95, 0, 36, 0, 5653, 0, 3124, 0],
        [944, 118, 0, 0, 327, 2575, 0, 0],
        [1249, 5160, 318, 2791, 0, 0, 0, 0]]
    # the masks and the matrices say the same thing
    for p in range(3):
        for q in range(3):
            if p != q:
                assert int(((r.support[pick == p] >> q) & 1).sum()) == r.pair_supported.sum(0)[p, q]
    assert np.array_equal(r.pair_edges, r.pair_edges.transpose(0, 2, 1))
    assert np.array_equal(r.pair_mutual, r.pair_mutual.transpose(0, 2, 1))
    uns, full = ag.support_counts(r.support, pick, 3)
    assert (uns, full) == (95 + 944 + 1249, 3124 + 2575 + 2791)


def test_window_oracle_equals_brute_force(c1):
    """The x-window loses nothing: the first micrograph through the full matrix."""
    methods, mgs, n_mg, off, x, y, r = c1
    o3 = off[:4]
    a = au.oracle(1, 3, 180, o3, x, y, 0.3)
    b = au.oracle(1, 3, 180, o3, x, y, 0.3, edges=au.pair_edges_brute)
    au.assert_same(a, b)
    assert a.pair_edges.sum() > 0


# ----------------------------------------------------------------------------- hand cases
def _two(xa, ya, xb, yb, box, t, edges=au.pair_edges_window):
    n_mg, off, x, y = au.pack(2, [[(xa, ya), (xb, yb)]])
    return au.oracle(n_mg, 2, box, off, x, y, t, edges=edges)


@pytest.mark.parametrize("edges", [au.pair_edges_window, au.pair_edges_brute])
def test_hand_threshold_boundary(edges):
    """Box 10, overlap area 50: JI == 50 / 150 == 1/3 in f64: not joined at T = 1/3 (strict),
    joined at 0.3."""
    for xa, xb in ((0, 5), (5, 0)):
        r = _two([xa], [0], [xb], [0], 10, 1 / 3, edges)
        assert r.support.tolist() == [0, 0] and r.partner.tolist() == [[-1, -1], [-1, -1]]
        assert r.pair_edges.sum() == 0 and not r.partner_ji.any()
        r = _two([xa], [0], [xb], [0], 10, 0.3, edges)
        assert r.support.tolist() == [2, 1] and r.partner.tolist() == [[-1, 1], [0, -1]]
        assert r.partner_ji[0, 1] == r.partner_ji[1, 0] == 1 / 3 == 50.0 / (200.0 - 50.0)
        assert r.pair_edges[0].tolist() == r.pair_supported[0].tolist() == [[0, 1], [1, 0]]
        assert r.pair_mutual[0].tolist() == [[0, 1], [1, 0]]


@pytest.mark.parametrize("edges", [au.pair_edges_window, au.pair_edges_brute])
def test_hand_dx_equal_box_and_identical(edges):
    # |dx| == B passes the prefilter but has no overlap: never joined, even at t = 0
    for t in (0.0, 0.3):
        assert _two([0], [0], [10], [0], 10, t, edges).pair_edges.sum() == 0
        assert _two([10], [0], [0], [0], 10, t, edges).pair_edges.sum() == 0
    # identical boxes: I = B^2, JI = 1
    r = _two([3.5], [7.25], [3.5], [7.25], 10, 0.3, edges)
    assert r.partner_ji[0, 1] == 1.0 and r.pair_mutual[0].tolist() == [[0, 1], [1, 0]]
    assert _two([3.5], [7.25], [3.5], [7.25], 10, 0.999999, edges).pair_edges.sum() == 2


@pytest.mark.parametrize("edges", [au.pair_edges_window, au.pair_edges_brute])
def test_hand_partner_ties_and_mutual(edges):
    """Picker 0 has one box; picker 1 has three at the same JI from it (mirror images and a
    copy): the partner is the lowest batch index.  All three name box 0 as their partner, and
    only the pair (0, 1) is reciprocal."""
    r = _two([0], [0], [2, -2, 2], [0, 0, 0], 10, 0.3, edges)
    assert r.partner_ji[1, 0] == r.partner_ji[2, 0] == r.partner_ji[3, 0] == r.partner_ji[0, 1]
    assert r.partner[:, 1].tolist() == [1, -1, -1, -1]
    assert r.partner[:, 0].tolist() == [-1, 0, 0, 0]
    assert r.pair_edges[0].tolist() == [[0, 3], [3, 0]]
    assert r.pair_supported[0].tolist() == [[0, 1], [3, 0]]
    assert r.pair_mutual[0].tolist() == [[0, 1], [1, 0]]
    # a larger JI beats a lower index
    r = _two([0], [0], [2, 1], [0, 0], 10, 0.3, edges)
    assert r.partner[0, 1] == 2
    # two identical boxes per picker, every JI equal: all name the lowest index of the other
    # picker, so only 0 <-> 2 is reciprocal (reciprocal best is not a maximum matching)
    r = _two([0, 0], [0, 0], [1, 1], [0, 0], 10, 0.3, edges)
    assert r.partner[:, 1].tolist()[:2] == [2, 2] and r.partner[:, 0].tolist()[2:] == [0, 0]
    assert r.pair_mutual[0].tolist() == [[0, 1], [1, 0]] and r.pair_edges[0, 0, 1] == 4


@pytest.mark.parametrize("edges", [au.pair_edges_window, au.pair_edges_brute])
def test_hand_non_finite_boxes_join_nothing(edges):
    nan, inf = float("nan"), float("inf")
    xa = [0, nan, inf, -inf, 0, 0, 0, 1]
    ya = [0, 0, 0, 0, nan, inf, -inf, 0]
    r = _two(xa, ya, xa, ya, 10, 0.0, edges)
    # only the finite boxes 0 and 7 of either picker meet
    assert r.support.tolist() == [2, 0, 0, 0, 0, 0, 0, 2] + [1, 0, 0, 0, 0, 0, 0, 1]
    assert r.pair_edges[0].tolist() == [[0, 4], [4, 0]]
    assert r.partner[0].tolist() == [-1, 8] and r.partner[7].tolist() == [-1, 15]


def test_k1_and_empty():
    n_mg, off, x, y = au.pack(1, [[([0, 1], [0, 0])], [([], [])]])
    r = au.oracle(n_mg, 1, 10, off, x, y, 0.3)
    assert r.support.tolist() == [0, 0] and r.partner.tolist() == [[-1], [-1]]
    assert not r.pair_edges.any() and r.pair_edges.shape == (2, 1, 1)
    r = au.oracle(0, 3, 10, np.zeros(1, np.int64), [], [], 0.3)
    assert r.support.shape == (0,) and r.pair_mutual.shape == (0, 3, 3)


# ----------------------------------------------------------------------------- host formatting
def test_venn_rows_and_pair_rows():
    methods = ["a", "b", "c"]
    counts = np.arange(24).reshape(3, 8)
    rows = ag.venn_rows(methods, counts)
    assert rows == ["a\t-\t0\n", "a\tb\t2\n", "a\tc\t4\n", "a\tb,c\t6\n",
                    "b\t-\t8\n", "b\ta\t9\n", "b\tc\t12\n", "b\ta,c\t13\n",
                    "c\t-\t16\n", "c\ta\t17\n", "c\tb\t18\n", "c\ta,b\t19\n"]
    assert ag.venn_rows(["only"], np.array([[5, 0]])) == ["only\t-\t5\n"]
    m = np.arange(9).reshape(3, 3)
    assert ag.pair_rows(methods, [7, 8, 9], m, m * 10, m * 100, base="mg")[:2] == [
        "mg\ta\tb\t7\t1\t10\t100\n", "mg\ta\tc\t7\t2\t20\t200\n"]
    assert len(ag.pair_rows(methods, [7, 8, 9], m, m, m)) == 6
    assert ag.box_pickers([0, 2, 2, 3, 4, 6, 6], 3).tolist() == [0, 0, 2, 0, 1, 1]


# ----------------------------------------------------------------------------- repic agreement
HEAD = b"x y w h conf\n"


def _line(x, y, s, end=b"\n"):
    return f"{x}\t{y}\t10\t10\t{s}".encode() + end


def _make_inputs(root, crash=False):
    ins = root / "in"
    for p in ("pickA", "pickB", "pickC"):
        (ins / p).mkdir(parents=True)
    f = {}
    # m1: a header line, CRLF endings, negative scores
    f["pickA", "m1.box"] = HEAD + _line(0, 0, 0.5) + _line(100, 100, 0.9) + _line(50, 50, 0.1)
    f["pickB", "m1.box"] = _line(1, 0, 0.9, b"\r\n") + _line(100, 101, 0.8, b"\r\n") + \
        _line(300, 300, 0.7, b"\r\n")
    f["pickC", "m1.box"] = _line(0, 1, -2.0) + _line(200, 200, -1.0)
    # m2: pickB has no file -> skipped
    f["pickA", "m2.box"] = _line(0, 0, 0.5)
    f["pickC", "m2.box"] = _line(0, 0, 0.5)
    # m3: no two boxes meet
    f["pickA", "m3.box"] = _line(500, 500, 0.5)
    f["pickB", "m3.box"] = _line(600, 600, 0.5) if not crash else b"0 0 10 10\n1 0 10 10\n"
    f["pickC", "m3.box"] = _line(700, 700, 0.5) + _line(720, 720, 0.4)
    for (p, name), raw in f.items():
        (ins / p / name).write_bytes(raw)
    order = ["m1.box", "m2.box", "m3.box"]
    return {"pickA": order, "pickB": ["m1.box", "m3.box"], "pickC": order}


def _args(root, listing=None, **kw):
    a = argparse.Namespace(in_dir=str(root / "in"), out_dir=str(root / "out"), box_size=10,
                           ji_threshold=0.3, per_box=False, batch_boxes=1 << 25, threads=None,
                           device=None, listing=listing)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _no_device(monkeypatch, call=au.oracle_device_call):
    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", no_ctx)
    monkeypatch.setattr(ag, "device_call", call)


J90 = repr(90.0 / (200.0 - 90.0))    # overlap 9 x 10 at box 10
J81 = repr(81.0 / (200.0 - 81.0))    # overlap 9 x 9

SUMMARY = ("base\tstatus\tboxes\tunsupported\tfully_supported\n"
           "m1\tok\t8\t3\t3\n"
           "m2\tskip\t0\t0\t0\n"
           "m3\tok\t4\t4\t0\n")
PAIRS = ("base\tpicker\tother\tboxes\tsupported\tedges\tmutual\n"
         "m1\tpickA\tpickB\t3\t2\t2\t2\n"
         "m1\tpickA\tpickC\t3\t1\t1\t1\n"
         "m1\tpickB\tpickA\t3\t2\t2\t2\n"
         "m1\tpickB\tpickC\t3\t1\t1\t1\n"
         "m1\tpickC\tpickA\t2\t1\t1\t1\n"
         "m1\tpickC\tpickB\t2\t1\t1\t1\n"
         "m3\tpickA\tpickB\t1\t0\t0\t0\n"
         "m3\tpickA\tpickC\t1\t0\t0\t0\n"
         "m3\tpickB\tpickA\t1\t0\t0\t0\n"
         "m3\tpickB\tpickC\t1\t0\t0\t0\n"
         "m3\tpickC\tpickA\t2\t0\t0\t0\n"
         "m3\tpickC\tpickB\t2\t0\t0\t0\n")
MATRIX = ("picker\tother\tboxes\tsupported\tedges\tmutual\n"
          "pickA\tpickB\t4\t2\t2\t2\n"
          "pickA\tpickC\t4\t1\t1\t1\n"
          "pickB\tpickA\t4\t2\t2\t2\n"
          "pickB\tpickC\t4\t1\t1\t1\n"
          "pickC\tpickA\t4\t1\t1\t1\n"
          "pickC\tpickB\t4\t1\t1\t1\n")
VENN = ("picker\tsupported_by\tboxes\n"
        "pickA\t-\t2\n" "pickA\tpickB\t1\n" "pickA\tpickC\t0\n" "pickA\tpickB,pickC\t1\n"
        "pickB\t-\t2\n" "pickB\tpickA\t1\n" "pickB\tpickC\t0\n" "pickB\tpickA,pickC\t1\n"
        "pickC\t-\t3\n" "pickC\tpickA\t0\n" "pickC\tpickB\t0\n" "pickC\tpickA,pickB\t1\n")
PER_BOX_M1 = (
    "picker\tline\tx\ty\tpickA_line\tpickA_ji\tpickB_line\tpickB_ji\tpickC_line\tpickC_ji\n"
    f"pickA\t0\t0.0\t0.0\t-\t-\t0\t{J90}\t0\t{J90}\n"
    f"pickA\t1\t100.0\t100.0\t-\t-\t1\t{J90}\t-\t-\n"
    "pickA\t2\t50.0\t50.0\t-\t-\t-\t-\t-\t-\n"
    f"pickB\t0\t1.0\t0.0\t0\t{J90}\t-\t-\t0\t{J81}\n"
    f"pickB\t1\t100.0\t101.0\t1\t{J90}\t-\t-\t-\t-\n"
    "pickB\t2\t300.0\t300.0\t-\t-\t-\t-\t-\t-\n"
    f"pickC\t0\t0.0\t1.0\t0\t{J90}\t0\t{J81}\t-\t-\n"
    "pickC\t1\t200.0\t200.0\t-\t-\t-\t-\t-\t-\n")
PER_BOX_M3 = (
    "picker\tline\tx\ty\tpickA_line\tpickA_ji\tpickB_line\tpickB_ji\tpickC_line\tpickC_ji\n"
    "pickA\t0\t500.0\t500.0\t-\t-\t-\t-\t-\t-\n"
    "pickB\t0\t600.0\t600.0\t-\t-\t-\t-\t-\t-\n"
    "pickC\t0\t700.0\t700.0\t-\t-\t-\t-\t-\t-\n"
    "pickC\t1\t720.0\t720.0\t-\t-\t-\t-\t-\t-\n")


def _read(out):
    return {f: (out / f).read_bytes().decode() for f in sorted(os.listdir(out))}


@pytest.mark.parametrize("batch_boxes", [1 << 25, 1])
def test_repic_agreement_files(tmp_path, monkeypatch, batch_boxes):
    listing = _make_inputs(tmp_path)
    calls = []

    def call(ctx, batch, t, partners=False, timing=False):
        calls.append(partners)
        return au.oracle_device_call(ctx, batch, t, partners, timing)
    _no_device(monkeypatch, call)
    ag_cmd.main(_args(tmp_path, listing, batch_boxes=batch_boxes))
    assert _read(tmp_path / "out") == {
        "agreement_matrix.tsv": MATRIX, "agreement_pairs.tsv": PAIRS,
        "agreement_summary.tsv": SUMMARY, "agreement_venn.tsv": VENN}
    assert calls and not any(calls)          # partners are asked for only with --per_box
    assert ag_cmd.LAST_RUN["micrographs"] == 2 and ag_cmd.LAST_RUN["boxes"] == 12
    assert ag_cmd.LAST_RUN["edges"] == 4 and ag_cmd.LAST_RUN["skipped"] == 1


@pytest.mark.parametrize("batch_boxes", [1 << 25, 1])
def test_repic_agreement_per_box(tmp_path, monkeypatch, batch_boxes):
    listing = _make_inputs(tmp_path)
    _no_device(monkeypatch)
    (tmp_path / "out").mkdir()               # an empty out_dir is accepted
    ag_cmd.main(_args(tmp_path, listing, per_box=True, batch_boxes=batch_boxes))
    assert _read(tmp_path / "out") == {
        "agreement_matrix.tsv": MATRIX, "agreement_pairs.tsv": PAIRS,
        "agreement_summary.tsv": SUMMARY, "agreement_venn.tsv": VENN,
        "m1_agreement.tsv": PER_BOX_M1, "m3_agreement.tsv": PER_BOX_M3}


def test_repic_agreement_parser_exception(tmp_path, monkeypatch):
    """pickB/m3.box has four columns: the reference's parser raises ValueError there; the rows
    of the micrographs before it are written first."""
    listing = _make_inputs(tmp_path, crash=True)
    _no_device(monkeypatch)
    with pytest.raises(ValueError):
        ag_cmd.main(_args(tmp_path, listing))
    got = _read(tmp_path / "out")
    assert got["agreement_summary.tsv"] == "".join(SUMMARY.splitlines(keepends=True)[:3])
    assert got["agreement_pairs.tsv"] == "".join(PAIRS.splitlines(keepends=True)[:7])
    assert sorted(got) == ["agreement_matrix.tsv", "agreement_pairs.tsv",
                           "agreement_summary.tsv", "agreement_venn.tsv"]


def _refused(call):
    def boom(*a, **k):
        raise AssertionError("the device call was reached")
    return boom


@pytest.mark.parametrize("kw, exc, match", [
    (dict(ji_threshold=1.0), ValueError, "ji_threshold"),
    (dict(ji_threshold=float("nan")), ValueError, "ji_threshold"),
    (dict(box_size=0), ValueError, "box_size"),
    (dict(box_size=(1 << 26) + 1), ValueError, "box_size"),
])
def test_refusals_before_any_side_effect(tmp_path, monkeypatch, kw, exc, match):
    listing = _make_inputs(tmp_path)
    _no_device(monkeypatch, _refused(None))
    with pytest.raises(exc, match=match):
        ag_cmd.main(_args(tmp_path, listing, **kw))
    assert not (tmp_path / "out").exists()


def test_world_size_refused(tmp_path, monkeypatch):
    listing = _make_inputs(tmp_path)
    _no_device(monkeypatch, _refused(None))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(_lib.RGCError, match="WORLD_SIZE"):
        ag_cmd.main(_args(tmp_path, listing))
    assert not (tmp_path / "out").exists()


def test_non_empty_out_dir_refused(tmp_path, monkeypatch):
    listing = _make_inputs(tmp_path)
    _no_device(monkeypatch, _refused(None))
    out = tmp_path / "out"
    out.mkdir()
    (out / "keep.txt").write_text("x")
    with pytest.raises(_lib.RGCError, match="not an empty directory"):
        ag_cmd.main(_args(tmp_path, listing))
    assert os.listdir(out) == ["keep.txt"] and (out / "keep.txt").read_text() == "x"
    # a file in out_dir's place is refused too
    (tmp_path / "file").write_text("y")
    with pytest.raises(_lib.RGCError, match="not an empty directory"):
        ag_cmd.main(_args(tmp_path, listing, out_dir=str(tmp_path / "file")))
    assert (tmp_path / "file").read_text() == "y"


def test_nine_pickers_refused(tmp_path, monkeypatch):
    _no_device(monkeypatch, _refused(None))
    for i in range(9):
        d = tmp_path / "in" / f"p{i}"
        d.mkdir(parents=True)
        (d / "m1.box").write_bytes(_line(0, 0, 0.5))
    with pytest.raises(_lib.RGCError, match="at most 8"):
        ag_cmd.main(_args(tmp_path))
    assert not (tmp_path / "out").exists()


# ----------------------------------------------------------------------------- dispatcher, library
def test_dispatcher_lists_agreement(capsys):
    with pytest.raises(SystemExit) as e:
        repic_main.main(["-h"])
    assert e.value.code == 0
    assert "agreement" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        repic_main.main(["agreement", "-h"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--per_box" in out and "--ji_threshold" in out
    p = argparse.ArgumentParser()
    ag_cmd.add_arguments(p)
    d = p.parse_args(["i", "o", "10"])
    assert d.per_box is False and d.ji_threshold == 0.3 and d.listing is None
    with pytest.raises(SystemExit):
        p.parse_args(["i", "o", "10", "--ji_threshold", "1.5"])


def test_library_has_the_symbols():
    import ctypes
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("rgc_agreement", "rgc_agreement_last_bytes"):
        assert hasattr(so, name) and name in _lib.EXPORTS, name
    assert _lib.has_agreement() and _lib.F_PARTNERS == 2048
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "repic_gc.h")).read()
    assert "#define RGC_F_PARTNERS 2048u" in hdr and "#define RGC_ABI_VERSION 11" in hdr


def test_missing_symbol_is_a_clear_error(monkeypatch):
    monkeypatch.setattr(_lib, "has_agreement", lambda: False)
    ctx = object.__new__(_lib.Context)
    with pytest.raises(_lib.RGCError, match="rgc_agreement"):
        _lib.Context.agreement(ctx, 0, 2, 10, [0], [], [])
    ctx._p = None   # (nothing to destroy)
