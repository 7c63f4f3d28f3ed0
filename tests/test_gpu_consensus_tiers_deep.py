"""``repic consensus --min_pickers`` (rgc_vote.hip, rgc_vote_host.cpp) where DESIGN.md 4.8 makes
promises that k = 3 and k = 4 cannot reach:

* cascades of 3 to 6 lower tiers at k = 5 and k = 8 (one context's buffers reused tier after
  tier, a tier in the middle without a column, up to 70 pseudo-micrographs per micrograph and
  tier, the mask-to-member scatter at k = 8), on both routes, against the model given the
  device's own picks (``_check_tiers`` of test_gpu_consensus_tiers.py, unchanged)
* the rule that ends the loop: a micrograph with two live pickers at k = 4 submits nothing at
  tier 3 and a pair at tier 2, alone and beside a micrograph for which tier 3 runs
* a micrograph's result does not depend on its batch, at k = 5 and k = 8
* a tier's run leaving the fused kernel (pseudo-micrographs above 4608 boxes), alone and in one
  pseudo-batch with fused ones
* device-resident inputs; the command over several device batches and at k = 5

tests/test_consensus_tiers_models.py pins every input used here with the model alone.
"""
import ctypes
import os

import numpy as np
import pytest

import vote_models as vm
import vote_util as vu
from golden_util import load_case, make_inputs
from test_gpu_consensus_tiers import _bits, _box_files, _check_tiers, _plain, _run_cli, _tiers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _route_flags(route):
    from repic_amd import _lib
    return _lib.F_NO_FUSED if route == "multi" else 0


def _assert_tiers_populated(r, name, n_mg):
    """What tests/test_consensus_tiers_models.py pins for the input, on the device's result."""
    c = vm.SYNTH[name]
    k, M = c["k"], c["M"]
    assert r.tier_cols.shape == (n_mg, k - M + 1) and r.tier_picks.shape == (n_mg, k - M + 1)
    for tier in c["populated"]:
        assert (r.tier_picks[:, k - tier] > 0).all(), tier
    for tier in c["empty"]:
        assert (r.tier_cols[:, k - tier] == 0).all() and (r.tier_picks[:, k - tier] == 0).all()


# ----------------------------------------------------------------------------- deep cascades
def test_pack_is_batch_pack():
    from repic_amd.pipeline import Batch
    for ids in (None, np.array([(1 << 31) + 5, (1 << 33) + 1], np.int64)):
        a = vm.synth_batch("k5", id_bases=ids)
        b = Batch.pack(a.k, a.box_size, vm.micrographs(a), id_bases=ids)
        assert (a.n_mg, a.k, a.box_size) == (b.n_mg, b.k, b.box_size)
        for f in ("box_off", "id_base", "x", "y", "score"):
            u, v = getattr(a, f), getattr(b, f)
            assert u.dtype == v.dtype and np.array_equal(u, v), f


@pytest.mark.parametrize("route", ["fused", "multi"])
@pytest.mark.parametrize("name", ["k5", "k8_m2", "k8_m6"])
def test_deep_cascade(ctx, name, route):
    b = vm.synth_batch(name)
    r, n_lower = _check_tiers(ctx, b, vm.SYNTH[name]["M"], None, flags=_route_flags(route))
    _assert_tiers_populated(r, name, b.n_mg)
    assert n_lower == int(r.tier_picks[:, 1:].sum()) > 0
    if name == "k8_m2":     # tier 7 ran (8 pseudo-micrographs) and gave no column
        assert (r.tier_cols[:, 1] == 0).all() and (r.tier_picks[:, 2:] > 0).all()
        assert len(set(r.pmask.tolist())) >= 20             # picks of many different subsets


@pytest.mark.parametrize("route", ["fused", "multi"])
def test_deep_cascade_fractional_coordinates(ctx, route):
    b = vm.synth_batch("k5", frac=True)
    assert (b.x != np.rint(b.x)).any()
    r, _ = _check_tiers(ctx, b, 2, 0.45, flags=_route_flags(route))
    _assert_tiers_populated(r, "k5", b.n_mg)


def test_deep_cascade_ids_above_2_to_31(ctx):
    """The consensus tie-break hashes the box ids: id bases that do not fit 32 bits."""
    ids = np.array([(1 << 31) + 5, (1 << 33) + 1], np.int64)
    b = vm.synth_batch("k5", id_bases=ids)
    assert np.array_equal(b.id_base, ids)
    r, _ = _check_tiers(ctx, b, 2, None)
    _assert_tiers_populated(r, "k5", b.n_mg)


@pytest.mark.parametrize("name", ["k5", "k8_m6"])
def test_min_pickers_k_is_the_plain_call(ctx, name):
    b = vm.synth_batch(name)
    k = b.k
    r, p = _tiers(ctx, b, k), _plain(ctx, b)
    assert r.n_picked > 0
    for f in ("pick_off", "px", "py", "pcol", "sel_cnt", "ilp_status"):
        assert np.array_equal(getattr(r, f), getattr(p, f)), f
    assert np.array_equal(_bits(r.pconf), _bits(p.pconf))
    assert (r.ptier == k).all() and (r.pmask == (1 << k) - 1).all()
    assert r.tier_cols.shape == (b.n_mg, 1) and r.tier_picks[:, 0].tolist() == np.diff(p.pick_off).tolist()
    assert set(np.unique(r.box_tier).tolist()) == {0, k}


# ----------------------------------------------------------------------------- the loop's end
def _view(r, b, m):
    """Everything the call returns about micrograph m, box indices local to the micrograph and
    floats by their bits."""
    k = b.k
    p0, p1 = int(r.pick_off[m]), int(r.pick_off[m + 1])
    b0, b1 = int(b.box_off[m * k]), int(b.box_off[(m + 1) * k])
    mem = r.pmember[p0:p1].astype(np.int64)
    assert ((mem == -1) | ((mem >= b0) & (mem < b1))).all()
    return dict(n=p1 - p0, ptier=r.ptier[p0:p1], pmask=r.pmask[p0:p1], px=r.px[p0:p1],
                py=r.py[p0:p1], pcol=r.pcol[p0:p1], pw=_bits(r.pw[p0:p1]),
                pconf=_bits(r.pconf[p0:p1]), pmember=np.where(mem >= 0, mem - b0, -1),
                box_tier=r.box_tier[b0:b1], sel_cnt=r.sel_cnt[m], status=r.run.status[m],
                ilp_status=r.ilp_status[m], tier_cols=r.tier_cols[m], tier_picks=r.tier_picks[m])


def _assert_same_view(a, b):
    assert a.keys() == b.keys()
    for f in a:
        assert np.array_equal(a[f], b[f]), (f, a[f], b[f])


def test_two_live_pickers_skip_tier_3(ctx):
    b = vm.pack(4, 10, [vm.two_live()])
    r = _tiers(ctx, b, 2)
    assert r.run.status.tolist() == [0] and r.pick_off.tolist() == [0, 2]
    assert r.ptier.tolist() == [4, 2] and r.pmask.tolist() == [15, 3]
    assert r.tier_cols.tolist() == [[1, 0, 1]] and r.tier_picks.tolist() == [[1, 0, 1]]
    assert r.pmember.tolist() == [[0, 2, 4, 5], [1, 3, -1, -1]]
    assert r.box_tier.tolist() == vm.TWO_LIVE_BOX_TIER
    assert r.sel_cnt.tolist() == [2]
    _check_tiers(ctx, b, 2, None)


@pytest.mark.parametrize("order", ["two_first", "three_first"])
def test_two_live_beside_three_live(ctx, order):
    """Tier 3 runs for the batch (three_live's triple); two_live still submits nothing there and
    its pair at tier 2: everything about it equals the run on its own."""
    alone = vm.pack(4, 10, [vm.two_live()])
    want = _view(_tiers(ctx, alone, 2), alone, 0)
    if order == "two_first":
        b, m = vm.pack(4, 10, [vm.two_live(), vm.three_live()], id_bases=[0, 6]), 0
    else:
        b, m = vm.pack(4, 10, [vm.three_live(), vm.two_live()], id_bases=[6, 0]), 1
    r = _tiers(ctx, b, 2)
    assert r.tier_cols[1 - m].tolist() == [1, 1, 1] and r.tier_cols[m].tolist() == [1, 0, 1]
    _assert_same_view(_view(r, b, m), want)
    assert want["ptier"].tolist() == [4, 2] and want["box_tier"].tolist() == vm.TWO_LIVE_BOX_TIER
    _check_tiers(ctx, b, 2, None)


def _gather_sections(ctx):
    return [n for n, _ in ctx.kernel_times()].count("k_vote_gather")


def test_loop_ends_when_no_picker_is_live(ctx):
    b = vm.pack(5, 10, [vm.all_explained()])
    r = _tiers(ctx, b, 2, timing=True)
    assert _gather_sections(ctx) == 1            # tier 4's count finds no live picker: the end
    assert r.tier_cols.tolist() == [[2, 0, 0, 0]] and r.tier_picks.tolist() == [[2, 0, 0, 0]]
    assert r.ptier.tolist() == [5, 5] and (r.box_tier == 5).all() and len(r.box_tier) == 10
    assert r.run.status.tolist() == [0]


def test_loop_runs_on_while_two_pickers_are_live(ctx):
    b = vm.pack(4, 10, [vm.two_live()])
    r = _tiers(ctx, b, 2, timing=True)
    assert _gather_sections(ctx) == 2            # tier 3 (nothing submitted) and tier 2
    assert r.ptier.tolist() == [4, 2]


# ----------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("name", ["k5", "k8_m2"])
def test_a_micrograph_does_not_see_its_batch(ctx, name):
    b = vm.synth_batch(name, n_mg=2)
    M = vm.SYNTH[name]["M"]
    r = _tiers(ctx, b, M)
    assert (r.tier_picks.sum(axis=1) > r.tier_picks[:, 0]).all()      # lower tiers have picks
    for m in range(b.n_mg):
        a = vm.one(b, m)
        _assert_same_view(_view(_tiers(ctx, a, M), a, 0), _view(r, b, m))


# ----------------------------------------------------------------------------- routes in a tier
@pytest.mark.parametrize("front", [False, True])
@pytest.mark.parametrize("name", ["deferred_tier", "fused_tier"])
def test_routes_inside_a_tier(ctx, name, front):
    """Tier 3 of either micrograph is deferred from the fused kernel; tier 2's pseudo-micrographs
    are (4700 boxes) or are not (3100).  With the hand case in front the tier-2 pseudo-batch
    holds its fused pseudo-micrographs and these."""
    mgs = ([vm.hand_mg()] if front else []) + [getattr(vm, name)()]
    b = vm.pack(3, 10, mgs)
    r, n_lower = _check_tiers(ctx, b, 2, None)
    assert r.tier_cols.tolist() == ([[2, 2]] if front else []) + [[50, 180]]
    assert r.tier_picks.tolist() == ([[1, 2]] if front else []) + [[50, 180]]
    # 50 triples and 180 pairs explain their own boxes and nothing else
    assert np.bincount(r.box_tier[9 if front else 0:]).tolist() == \
        [len(mgs[-1][0][0]) * 3 - 510, 0, 360, 150]
    assert n_lower == (182 if front else 180)


# ----------------------------------------------------------------------------- device inputs
RETURNED = ("pick_off", "px", "py", "pcol", "sel_cnt", "ilp_status", "ptier", "pmask", "pmember",
            "box_tier", "tier_cols", "tier_picks")
RETURNED_BITS = ("pconf", "pw", "ilp_gap")


def test_device_resident_inputs(ctx):
    """x, y, score already on the device (F_DEVICE_INPUTS), then the offsets and id bases too
    (dev_meta): every returned array equals the host-input call's."""
    from repic_amd import _lib
    hip = ctypes.CDLL("libamdhip64.so")
    b = vm.synth_batch("k5")
    want = _tiers(ctx, b, 2)
    assert want.tier_picks[:, 1:].all()
    held = []

    def dev(a):
        a = np.ascontiguousarray(a)
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(a.nbytes)) == 0
        held.append(p)
        assert hip.hipMemcpy(p, ctypes.c_void_p(a.ctypes.data), ctypes.c_size_t(a.nbytes),
                             ctypes.c_int(1)) == 0
        return p.value
    try:
        dx, dy, ds = dev(b.x), dev(b.y), dev(b.score)
        meta = (dev(b.box_off.astype(np.int32)), dev(b.id_base))
        assert hip.hipDeviceSynchronize() == 0
        for dev_meta in (None, meta):
            r = ctx.consensus_tiers(b.n_mg, b.k, b.box_size, b.box_off, b.id_base, dx, dy, ds, 2,
                                    flags=_lib.F_DEVICE_INPUTS, dev_meta=dev_meta)
            for f in RETURNED:
                assert np.array_equal(getattr(r, f), getattr(want, f)), (f, dev_meta)
            for f in RETURNED_BITS:
                assert np.array_equal(_bits(getattr(r, f)), _bits(getattr(want, f))), (f, dev_meta)
            assert np.array_equal(r.run.status, want.run.status)
    finally:
        for p in held:
            hip.hipFree(p)


# ----------------------------------------------------------------------------- the command
SPLIT_BOXES = 2000      # test_gpu_consensus.py::test_consensus_split_batches' --batch_boxes


def test_cli_split_batches_change_nothing(tmp_path):
    """--batch_boxes 2000 sends the 12 golden micrographs through at least 3 device batches:
    every file of the run, the run-level tables included (neither has a timing column), is byte
    for byte that of the one-batch run."""
    from repic_amd.commands import consensus
    from repic_amd.pipeline import split_batches
    meta, _ = load_case("c1_10017")
    in_dir = make_inputs("c1_10017", str(tmp_path))
    _, bases, mgs = vu.load_dir(in_dir)
    counts = [sum(len(t[0]) for t in mg) for mg in mgs]
    assert len(bases) == 12 and len(split_batches(counts, SPLIT_BOXES)) >= 3
    one = _run_cli(in_dir, str(tmp_path / "one"), meta, min_pickers=2)
    split = _run_cli(in_dir, str(tmp_path / "split"), meta, min_pickers=2, batch_boxes=SPLIT_BOXES)
    assert set(one) == set(split)
    boxes = _box_files(one)
    tiers = {f for f in one if f.endswith(consensus.TIERS_SUFFIX)} - {consensus.TIERS}
    assert len(boxes) == 12 and tiers == {f[:-4] + consensus.TIERS_SUFFIX for f in boxes}
    assert {consensus.TIERS, consensus.SUMMARY} <= set(one)
    for f in sorted(one):       # the .box and _tiers.tsv files and both tables: no file left out
        assert split[f] == one[f], f
    assert any(ln.startswith(b"2\t") for f in tiers for ln in one[f].splitlines())


def test_cli_three_of_five(tmp_path):
    """The command at k = 5, M = 3, on the BOX files of the synthetic k = 5 batch."""
    from repic_amd import synth
    from repic_amd.commands import consensus
    in_dir = str(tmp_path / "in")
    names = synth.write_box_dirs(in_dir, vm.synth_config("k5"), vm.SYNTH["k5"]["n_mg"])
    assert names == [f"picker{p}" for p in range(5)]
    meta = {"box": vm.SYNTH_BOX, "listing": None}
    plain = _run_cli(in_dir, str(tmp_path / "plain"), meta)
    m3 = _run_cli(in_dir, str(tmp_path / "m3"), meta, min_pickers=3)
    rows = m3[consensus.TIERS].decode().splitlines(keepends=True)
    assert rows[0] == consensus.tiers_header(5, 3) == \
        "base\tcols_5\tpicks_5\tcols_4\tpicks_4\tcols_3\tpicks_3\n"
    tab = {r.split("\t")[0]: [int(v) for v in r.split("\t")[1:]] for r in rows[1:]}
    assert len(_box_files(plain)) == 2 and set(tab) == {f[:-4] for f in _box_files(plain)}
    for f, v in _box_files(plain).items():
        n5 = v.count(b"\n")
        assert n5 > 0 and m3[f].startswith(v)               # lines 1..n_5: the plain file
        lines = m3[f[:-4] + consensus.TIERS_SUFFIX].decode().splitlines()
        assert len(lines) == m3[f].count(b"\n")
        tiers = [int(ln.split("\t")[0]) for ln in lines]
        assert tiers == sorted(tiers, reverse=True) and set(tiers) == {5, 4, 3}
        assert tiers.count(5) == n5
        for ln, t in zip(lines, tiers):
            pk = ln.split("\t")[1].split(",")
            assert len(pk) == t and set(pk) <= set(names) and pk == sorted(set(pk))
        c5, p5, c4, p4, c3, p3 = tab[f[:-4]]
        assert (p5, p4, p3) == tuple(tiers.count(t) for t in (5, 4, 3))
        assert c5 >= p5 and c4 >= p4 and c3 >= p3
