"""``repic consensus --min_pickers`` without a device: the plain-Python model (tests/vote_util.py)
on hand cases, the flag's parsing, the refusals (before a context exists or anything is deleted)
and the header / EXPORTS agreement for the new symbols."""
import argparse
import os
import re

import numpy as np
import pytest

import vote_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


hand_batch = vu.hand_batch


def test_model_subsets_are_in_tuple_order():
    assert vu.subsets(3, 2) == [(0, 1), (0, 2), (1, 2)]
    assert vu.subsets(4, 3) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)]
    assert [vu.mask_of(S) for S in vu.subsets(3, 2)] == [3, 5, 6]


def test_model_explained_is_strict_and_ignores_non_finite():
    # overlap 6 x 10 of two 10-boxes: JI = 60 / 140 = 3 / 7, the same two roundings on both sides
    t = 60.0 / 140.0
    assert not vu.explains(0.0, 0.0, 4.0, 0.0, 10, t)
    assert vu.explains(0.0, 0.0, 4.0, 0.0, 10, np.nextafter(t, 0.0))
    assert not vu.explains(float("nan"), 0.0, 0.0, 0.0, 10, 0.0)
    assert not vu.explains(0.0, float("inf"), 0.0, 0.0, 10, 0.0)
    assert not vu.explains(0.0, 0.0, float("nan"), 0.0, 10, 0.0)


def test_model_hand_case_tiers():
    b = hand_batch()
    tier = np.zeros(9, np.int32)
    # tier 3 on everything: the cliques {A0, A1, A2} and {A0, A1, duplicate} share boxes; the
    # packing takes the heavier one
    cols3 = vu.tier_columns(b, 0, tier, 3, 0.3)
    assert [S for S, _ in cols3] == [(0, 1, 2)]
    d3 = cols3[0][1]
    assert set(d3) == {(0, 3, 6), (0, 3, 7)}
    assert d3[(0, 3, 6)][0] > d3[(0, 3, 7)][0]
    assert abs(vu.tier_optimum(cols3) - float(d3[(0, 3, 6)][0])) <= 1e-12
    cons = d3[(0, 3, 6)][2]
    assert cons in (0, 3, 6)
    vu.mark_explained(tier, b, 0, [(b.x[cons], b.y[cons])], 3, 0.3)
    assert tier.tolist() == [3, 0, 0, 3, 0, 0, 3, 3, 0]     # the duplicate is explained, D is not
    # tier 2 on the rest: B from pickers (0, 1), C from pickers (1, 2), nothing from (0, 2)
    pm = vu.pseudo_micrographs(b, 0, tier, 2)
    assert [(S, segs) for S, segs in pm] == [((0, 1), [[1, 2], [4, 5]]), ((0, 2), [[1, 2], [8]]),
                                             ((1, 2), [[4, 5], [8]])]
    cols2 = vu.tier_columns(b, 0, tier, 2, 0.3)
    assert [(S, sorted(d)) for S, d in cols2] == [((0, 1), [(1, 4)]), ((0, 2), []), ((1, 2), [(5, 8)])]
    wB, confB, consB = cols2[0][1][(1, 4)]
    wC, confC, consC = cols2[2][1][(5, 8)]
    assert confB == np.float32(0.8) and confC == np.float32(0.6) and consB in (1, 4) and consC in (5, 8)
    assert abs(vu.tier_optimum(cols2) - (float(wB) + float(wC))) <= 1e-12
    vu.mark_explained(tier, b, 0, [(b.x[consB], b.y[consB]), (b.x[consC], b.y[consC])], 2, 0.3)
    assert tier.tolist() == [3, 2, 0, 3, 2, 2, 3, 3, 2]


def test_model_drops_pseudo_micrographs_with_an_empty_segment():
    b = hand_batch()
    tier = np.zeros(9, np.int32)
    tier[6:9] = 3                                   # picker 2 has nothing left
    assert [S for S, _ in vu.pseudo_micrographs(b, 0, tier, 2)] == [(0, 1)]
    tier[:] = 3
    assert vu.pseudo_micrographs(b, 0, tier, 2) == []


# ----------------------------------------------------------------------------- the flag
def _parser():
    from repic_amd.commands import consensus
    p = argparse.ArgumentParser()
    consensus.add_arguments(p)
    return p


def test_min_pickers_parsing():
    p = _parser()
    assert p.parse_args(["in", "out", "180"]).min_pickers is None
    assert p.parse_args(["in", "out", "180", "--min_pickers", "2"]).min_pickers == 2
    with pytest.raises(SystemExit) as e:
        p.parse_args(["in", "out", "180", "--min_pickers", "two"])
    assert e.value.code != 0


def _dirs(tmp_path, k=3):
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    for p in range(k):
        (in_dir / f"picker{p}").mkdir(parents=True)
        (in_dir / f"picker{p}" / "mg.box").write_text("10\t10\t10\t10\t0.5\n")
    out_dir.mkdir()
    (out_dir / "keep.txt").write_text("untouched")
    return str(in_dir), str(out_dir)


@pytest.mark.parametrize("extra", [["--min_pickers", "2", "--get_cc"],
                                   ["--min_pickers", "2", "--members"],
                                   ["--min_pickers", "1"], ["--min_pickers", "4"],
                                   ["--min_pickers", "0"], ["--min_pickers", "-2"]])
def test_refusals_leave_out_dir_untouched_and_create_no_context(tmp_path, monkeypatch, extra):
    from repic_amd import _lib
    from repic_amd.commands import consensus
    in_dir, out_dir = _dirs(tmp_path)

    def no_context(*a, **kw):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", no_context)
    args = _parser().parse_args([in_dir, out_dir, "10"] + extra)
    with pytest.raises(_lib.RGCError, match="nothing was deleted or written"):
        consensus.main(args)
    assert sorted(os.listdir(out_dir)) == ["keep.txt"]
    assert open(os.path.join(out_dir, "keep.txt")).read() == "untouched"


def test_min_pickers_of_accepts_the_range(tmp_path):
    from repic_amd.commands import consensus
    in_dir, out_dir = _dirs(tmp_path)
    ns = lambda m: argparse.Namespace(in_dir=in_dir, out_dir=out_dir, min_pickers=m)  # noqa: E731
    assert consensus.min_pickers_of(ns(None)) is None
    assert consensus.min_pickers_of(ns(2)) == 2 and consensus.min_pickers_of(ns(3)) == 3
    assert consensus.min_pickers_of(argparse.Namespace(in_dir=in_dir, out_dir=out_dir)) is None
    assert consensus.tiers_header(3, 2) == "base\tcols_3\tpicks_3\tcols_2\tpicks_2\n"


# ----------------------------------------------------------------------------- the symbols
def test_header_exports_and_library_agree_on_the_tier_symbols():
    import ctypes

    from repic_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "repic_gc.h")).read()
    decl = set(re.findall(r"\b(rgc_[a-z_]+)\s*\(", hdr))
    assert decl == set(_lib.EXPORTS), decl ^ set(_lib.EXPORTS)
    so = ctypes.CDLL(_lib.LIB_PATH)
    assert _lib.has_tiers()
    for name in ("rgc_consensus_tiers", "rgc_vote_gather"):
        assert name in decl and name in _lib.EXPORTS and hasattr(so, name), name
    assert re.search(r"^#define\s+RGC_ABI_VERSION\s+11\s*$", hdr, re.M) and _lib.abi_version() == 11
    # the bindings' structs follow the header's field order
    for struct, cls in (("rgc_tiers_out", _lib.TiersOut), ("rgc_vote_gather_in", _lib.VoteGatherIn),
                        ("rgc_vote_gather_out", _lib.VoteGatherOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.search(r"(\w+)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert names == [f[0] for f in cls._fields_], struct
