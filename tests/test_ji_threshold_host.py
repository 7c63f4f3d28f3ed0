"""``--ji_threshold`` without a GPU: the oracle at other thresholds against the reference's own
runs, the host's exact cutoffs (rgc_test_ji_cutoff) against the reference quotient by brute
force, the grid plan's stencil at the reach of every threshold, and the CLI's validation.

An edge is the reference's f64 ``I / ((2 B^2) - I) > t`` (get_cliques.py:40-46, 59-69).  The
library does not keep a band around ``c(t) B^2``: it passes the largest I whose quotient does
not exceed t (the quotient is monotone in I), so ``f64_lo == f64_hi`` and the band property
("no I outside [f64_lo, f64_hi] disagrees with the quotient") is checked with an empty band.
"""
import argparse
import builtins
import os
import sys

import numpy as np
import pytest

from golden_util import assert_matches_golden, read_outputs
from threshold_util import THR, load_thr, make_thr_inputs, patch_oracles, ref_q, rho

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "tools"))

BS = [1, 2, 7, 13, 26, 64, 180, 2896]
TS = [0.0, 0.05, 0.2, 0.3, 1.0 / 3.0, 0.5, 0.9, float(np.nextafter(0.3, np.inf)),
      float(np.nextafter(0.3, -np.inf)), float(np.nextafter(1.0, 0.0))]


# ---- 1. the oracle at other thresholds reproduces the reference's runs
@pytest.mark.parametrize("name", THR)
def test_oracle_matches_reference_at_threshold(name, tmp_path, monkeypatch):
    from oracle import cpu_ref
    meta, data = load_thr(name)
    patch_oracles(monkeypatch, meta["ji_threshold"])
    in_dir = make_thr_inputs(meta, str(tmp_path))
    out_dir = os.path.join(str(tmp_path), "out")
    exc = None
    try:
        cpu_ref.run_dir(in_dir, out_dir, meta["box"], get_cc="--get_cc" in meta["flags"],
                        multi_out="--multi_out" in meta["flags"], listing=meta["listing"])
    except Exception as e:  # noqa: BLE001 - exception class is part of the contract
        exc = e
    if meta["exception"]:
        assert isinstance(exc, getattr(builtins, meta["exception"])), (meta["exception"], exc)
    else:
        assert exc is None, exc
    mgs, arrays = read_outputs(out_dir, meta)
    assert_matches_golden(meta, data, mgs, arrays)


# ---- 2. the cutoffs the launches pass, against the quotient itself
@pytest.mark.parametrize("B", BS)
def test_integer_cutoff_is_the_quotients(B):
    """For every integer area I: ``I > int_cut`` <=> ``q(I) > t`` (all I for B <= 180; +-64
    around the cut for 2896, where monotonicity of q decides the rest)."""
    from repic_amd import _lib
    for t in TS:
        cut, _, _ = _lib.ji_cutoff(B, t)
        assert 0 <= cut < B * B
        if B <= 180:
            I = np.arange(0, B * B + 1, dtype=np.int64)
        else:
            I = np.arange(max(0, cut - 64), min(B * B, cut + 64) + 1, dtype=np.int64)
        assert np.array_equal(I > cut, ref_q(I.astype(np.float64), B) > t), (B, t)


def test_default_integer_cutoff_is_todays():
    """At 0.3 the cut is floor(6 B^2 / 13) for every B of the integer layout, so the default
    path keeps its value."""
    from repic_amd import _lib
    for B in range(1, 2897):
        assert _lib.ji_cutoff(B, 0.3)[0] == (6 * B * B) // 13, B


@pytest.mark.parametrize("B", BS)
def test_f64_cutoff_is_the_quotients(B):
    """No f64 area disagrees with the quotient: at the cut and its neighbours, at 10^5 random
    areas per (B, t) over [0, B^2], and at 10^5 within 2^-30 (relative) of the cut."""
    from repic_amd import _lib
    rng = np.random.default_rng(B)
    b2 = float(B * B)
    for t in TS:
        _, lo, hi = _lib.ji_cutoff(B, t)
        assert lo == hi and 0.0 <= hi < b2
        assert not ref_q(hi, B) > t
        assert ref_q(np.nextafter(hi, np.inf), B) > t
        steps = [hi]
        for _ in range(8):
            steps.append(np.nextafter(steps[-1], np.inf))
        down = [hi]
        for _ in range(8):
            down.append(max(0.0, np.nextafter(down[-1], -np.inf)))
        I = np.concatenate([steps, down, rng.uniform(0.0, b2, 100000),
                            np.clip(hi * (1.0 + rng.uniform(-1, 1, 100000) * 2.0 ** -30),
                                    0.0, b2)])
        assert np.array_equal(I > hi, ref_q(I, B) > t), (B, t)


def test_cutoff_hook_rejects_bad_arguments():
    from repic_amd import _lib
    for t in (-0.1, 1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.RGCError, match="ji_threshold"):
            _lib.ji_cutoff(180, t)
    with pytest.raises(_lib.RGCError):
        _lib.ji_cutoff(0, 0.3)


# ---- 3. the planned 2x3 stencil holds every partner at the reach of t
def _reach_points(B, t, rm):
    """Anchors whose column and row phases sweep a cell (17 x 17 phases at the planned minimum
    cell 2 rm x rm), each with partners at rho(t) B (1 - 2^-20) in x, in y and on the four
    diagonals; then two frame boxes that fix the field's bounding box."""
    d = rho(t) * B * (1.0 - 2.0 ** -20)
    ax, ay = np.meshgrid(np.arange(17) * (2.0 * rm) * (1.0 + 1.0 / 17.0),
                         np.arange(17) * rm * (1.0 + 1.0 / 17.0))
    ax, ay = ax.reshape(-1) + 2.0 * B, ay.reshape(-1) + 2.0 * B
    dirs = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]
    frame = np.array([0.0, ax.max() + 2.0 * B]), np.array([0.0, ay.max() + 2.0 * B])
    xs = np.concatenate([ax] + [ax + sx * d for sx, _ in dirs] + [frame[0]])
    ys = np.concatenate([ay] + [ay + sy * d for _, sy in dirs] + [frame[1]])
    return xs, ys, len(ax), len(dirs)


@pytest.mark.parametrize("large", [False, True])
@pytest.mark.parametrize("t", [0.0, 0.05, 0.15, 0.3, 0.6, 0.95])
def test_stencil_holds_partners_at_reach(t, large):
    """Cell sizes from the kernels' formula (stencil_check.row_min = JiCut.row_min).  The anchors
    are then moved onto the planned grid's own borders (exactly on, and one ulp to either
    side of, every column and row border they lie next to) and checked again."""
    import stencil_check as sc
    B = 100.0
    rm = float(sc.row_min(B, t))
    assert rm >= rho(t) * B * 1.0028 * (1 - 1e-12)
    assert rho(t) * B / (2.0 * rm) <= 0.5 / 1.0028 * (1 + 1e-12)   # the half-column margin
    cells = sc.cells_large if large else sc.cells
    plan = sc.plan_large if large else sc.plan

    def check(xs, ys, na, nd):
        cx, cy, c0 = cells(xs, ys, B, t)
        for j in range(nd):
            p = slice(na * (1 + j), na * (2 + j))
            # either end of the pair finds the other in its 2 x 3 stencil
            for a, b in ((slice(0, na), p), (p, slice(0, na))):
                ok = ((cx[b] == c0[a]) | (cx[b] == c0[a] + 1)) & (np.abs(cy[b] - cy[a]) <= 1)
                assert ok.all(), (t, large, j, int((~ok).sum()))

    xs, ys, na, nd = _reach_points(B, t, rm)
    check(xs, ys, na, nd)
    # the same field (bounding box and box count unchanged: same plan) with anchors on borders
    mnx, mny, icl, icly, gx, gy = plan(xs, ys, B, len(xs), t=t)
    d = rho(t) * B * (1.0 - 2.0 ** -20)
    bx = mnx + np.rint((xs[:na] - mnx) * icl) / icl
    by = mny + np.rint((ys[:na] - mny) * icly) / icly
    for sh in (0.0, 1.0, -1.0):
        nx = bx if sh == 0 else np.nextafter(bx, sh * np.inf)
        ny = by if sh == 0 else np.nextafter(by, sh * np.inf)
        dirs = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]
        x3 = np.concatenate([nx] + [nx + sx * d for sx, _ in dirs] + [xs[-2:]])
        y3 = np.concatenate([ny] + [ny + sy * d for _, sy in dirs] + [ys[-2:]])
        assert plan(x3, y3, B, len(x3), t=t) == plan(xs, ys, B, len(xs), t=t)
        check(x3, y3, na, nd)


def test_stencil_model_covers_edges_at_low_thresholds():
    """tools/stencil_check's random micrographs (the model test_stencil_cover.py runs at 0.3):
    no JI > t pair outside the stencil at t = 0 and 0.05, both routes."""
    import stencil_check as sc
    rng = np.random.default_rng(3)
    for t in (0.0, 0.05):
        tot = 0
        for B, n, W in ((64.0, 400, 1000.0), (37.0, 700, 1000.0), (2.5, 300, 50.0)):
            xs, ys = rng.uniform(0, W, n), rng.uniform(0, W, n)
            for fn in (sc.missed, sc.missed_large):
                m, e = fn(xs, ys, B, t)
                assert m == 0
                tot += e
        assert tot > 1000   # (a few thousand pairs per threshold: the check is not vacuous)


# ---- 4. CLI validation, before a device context exists or out_dir is touched
def _dirs(tmp_path):
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    for p in ("a", "b"):
        (in_dir / p).mkdir(parents=True)
        (in_dir / p / "m1.box").write_text("100\t100\t100\t100\t0.5\n")
    out_dir.mkdir()
    (out_dir / "keep.txt").write_text("still here")
    return str(in_dir), out_dir


@pytest.mark.parametrize("command", ["get_cliques", "consensus"])
@pytest.mark.parametrize("bad", ["-0.1", "1.0", "nan", "inf"])
def test_cli_refuses_threshold_outside_range(command, bad, tmp_path, capsys):
    from repic_amd import main as cli
    from repic_amd.commands import consensus, get_cliques
    in_dir, out_dir = _dirs(tmp_path)
    with pytest.raises(SystemExit) as e:     # the parser refuses it
        cli.main([command, in_dir, str(out_dir), "100", f"--ji_threshold={bad}"])
    assert e.value.code == 2 and "ji_threshold" in capsys.readouterr().err
    # ... and so does the command itself when called with a namespace (plugin protocol)
    mod = {"get_cliques": get_cliques, "consensus": consensus}[command]
    p = argparse.ArgumentParser()
    mod.add_arguments(p)
    args = p.parse_args([in_dir, str(out_dir), "100"])
    args.ji_threshold = float(bad)
    with pytest.raises(ValueError, match="ji_threshold"):
        mod.main(args)
    assert (out_dir / "keep.txt").read_text() == "still here"
    assert sorted(os.listdir(out_dir)) == ["keep.txt"]


@pytest.mark.parametrize("command", ["get_cliques", "consensus"])
def test_cli_default_threshold_is_the_default_path(command):
    from repic_amd import _lib
    from repic_amd.commands import consensus, get_cliques
    mod = {"get_cliques": get_cliques, "consensus": consensus}[command]
    p = argparse.ArgumentParser()
    mod.add_arguments(p)
    for argv in (["i", "o", "100"], ["i", "o", "100", "--ji_threshold", "0.3"],
                 ["i", "o", "100", "--ji_threshold", "0.30"]):
        a = p.parse_args(argv)
        assert a.ji_threshold == _lib.JI_DEFAULT == 0.3
        assert get_cliques.ji_threshold_of(a) is None      # no flag: the library's 0.3 path
    a = p.parse_args(["i", "o", "100", "--ji_threshold", "0"])
    assert get_cliques.ji_threshold_of(a) == 0.0
    a = p.parse_args(["i", "o", "100", "--ji_threshold", "0.45"])
    assert get_cliques.ji_threshold_of(a) == 0.45


def test_batch_struct_keeps_its_earlier_layout():
    """ABI 11 appends ji_threshold: every earlier field keeps its offset, and the header, the
    binding and the library agree on the version."""
    from repic_amd import _lib
    assert _lib.abi_version() == 11
    offs = {n: getattr(_lib.BatchIn, n).offset for n, _ in _lib.BatchIn._fields_}
    assert offs["dev_id_base"] == 72 and offs["ji_threshold"] == 80
    assert _lib.F_JI_THRESHOLD == 1024
