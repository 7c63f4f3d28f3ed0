"""The inputs of tests/test_gpu_consensus_tiers_deep.py are what that file says they are: asserted
from the model alone (tests/vote_util.py, HiGHS; tests/vote_models.py cascades tier by tier on
its own optimum), without a device.  A generator or builder that drifts - a tier that lost its
picks, a pseudo-micrograph that slipped under the fused kernel's limit - fails here, so a GPU
test cannot pass on an input that no longer reaches the code it is for."""
import functools
import os
import re

import numpy as np
import pytest

import vote_models as vm
import vote_util as vu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "repic-copy_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _synth_key(name, frac, t, n_mg):
    b = vm.synth_batch(name, frac=frac, n_mg=n_mg)
    return (b,) + vm.cascade(b, vm.SYNTH[name]["M"], t)


def _synth(name, frac=False, t=0.3, n_mg=None):
    """(batch, facts, box_tier), computed once per input."""
    return _synth_key(name, frac, t, n_mg)


@functools.lru_cache(maxsize=None)
def _hand(name):
    k, mg = {"two_live": (4, vm.two_live), "three_live": (4, vm.three_live),
             "all_explained": (5, vm.all_explained)}[name]
    b = vm.pack(k, 10, [mg()])
    return (b,) + vm.cascade(b, 2)


@functools.lru_cache(maxsize=None)
def _lattice(name):
    b = vm.pack(3, 10, [getattr(vm, name)()])
    return (b,) + vm.cascade(b, 2)


def test_limits_are_the_sources():
    src = open(os.path.join(CSRC, "rgc_ilp.hip")).read()
    assert int(re.search(r"constexpr int ILP_BIG = (\d+);", src).group(1)) == vm.ILP_BIG
    src = open(os.path.join(CSRC, "rgc_run.cpp")).read()
    assert int(re.search(r"constexpr int64_t FUSED_MAX_BOXES = (\d+);", src).group(1)) == \
        vm.FUSED_MAX_BOXES


def test_pack_lays_a_batch_out():
    b = vm.pack(4, 10, [vm.two_live(), vm.three_live()])
    assert (b.n_mg, b.k, b.box_size) == (2, 4, 10)
    assert b.box_off.tolist() == [0, 2, 4, 5, 6, 9, 12, 14, 15] and b.id_base.tolist() == [0, 6]
    assert b.x[:6].tolist() == [100, 200, 101, 201, 100, 101]
    o = vm.one(b, 1)
    assert o.id_base.tolist() == [6] and o.box_off.tolist() == [0, 3, 6, 8, 9]
    assert np.array_equal(o.x, b.x[6:]) and np.array_equal(o.score, b.score[6:])
    big = vm.pack(4, 10, [vm.two_live()], id_bases=[(1 << 33) + 7])
    assert big.id_base.dtype == np.int64 and int(big.id_base[0]) == (1 << 33) + 7


# ----------------------------------------------------------------------------- synthetic cascades
@pytest.mark.parametrize("name,frac,t", [("k5", False, 0.3), ("k5", True, 0.45),
                                         ("k8_m2", False, 0.3), ("k8_m6", False, 0.3)])
def test_synthetic_cascades(name, frac, t):
    """Every tier named as populated has a pick in every micrograph, every tier named as empty
    submits subsets and gets no column, and no conflict component is left unsearched."""
    c = vm.SYNTH[name]
    b, facts, box_tier = _synth(name, frac, t)
    k = c["k"]
    assert b.n_mg == c["n_mg"] == len(facts) and b.k == k and b.box_size == vm.SYNTH_BOX
    assert sorted(c["populated"] + c["empty"]) == list(range(c["M"], k + 1))
    for f in facts:
        for tier in c["populated"]:
            assert len(f[tier]["picks"]) >= 1 and sum(f[tier]["cols"]) >= len(f[tier]["picks"])
        for tier in c["empty"]:
            assert len(f[tier]["subsets"]) >= 1 and sum(f[tier]["cols"]) == 0
            assert f[tier]["picks"] == []
        for tier, d in f.items():
            assert d["comp"] <= vm.ILP_BIG
            assert d["live"] == k          # every picker keeps an unexplained box: all subsets go
            assert [S for S, _ in d["subsets"]] == vu.subsets(k, tier)
    assert set(np.unique(box_tier).tolist()) == {0} | set(c["populated"])
    if frac:
        assert (b.x != np.rint(b.x)).any()


def test_synthetic_k5_sizes():
    _, facts, _ = _synth("k5")
    per_tier = [sum(f[t]["cols"]) for f in facts for t in (5, 4, 3, 2)]
    assert 4 <= min(per_tier) and max(per_tier) <= 24
    assert max(d["comp"] for f in facts for d in f.values()) == 8     # a searched component


def test_synthetic_k8_two_of_eight():
    """Tier 8 has one pick; tier 7 submits its 8 subsets and has no column; the five tiers below
    all have picks; a tier submits up to 70 pseudo-micrographs."""
    _, facts, _ = _synth("k8_m2")
    f = facts[0]
    assert len(f[8]["picks"]) == 1
    assert len(f[7]["subsets"]) == 8 and f[7]["cols"] == [0] * 8
    assert [len(f[t]["picks"]) for t in (6, 5, 4, 3, 2)] == [8, 6, 9, 3, 6]
    assert [len(f[t]["subsets"]) for t in (6, 5, 4, 3, 2)] == [28, 56, 70, 56, 28]
    # the picks of the lower tiers come from many different subsets: the mask-to-member scatter
    masks = {vu.mask_of(S) for t in range(2, 7) for S, _ in f[t]["picks"]}
    assert len(masks) >= 20 and max(masks) >= 128 and min(masks) <= 12


def test_synthetic_k8_two_micrographs():
    """The batch-independence input: the second micrograph has columns at tier 7, where the
    first has none, so the tier runs for the batch with nothing to pack for the first."""
    b, facts, _ = _synth("k8_m2", n_mg=2)
    one = _synth("k8_m2")[0]
    assert b.n_mg == 2 and np.array_equal(b.x[:len(one.x)], one.x)
    assert sum(facts[0][7]["cols"]) == 0 and sum(facts[1][7]["cols"]) > 0
    assert all(len(facts[1][t]["picks"]) >= 1 for t in range(2, 9))
    assert max(d["comp"] for f in facts for d in f.values()) <= vm.ILP_BIG


def test_synthetic_k8_six_of_eight():
    _, facts, _ = _synth("k8_m6")
    f = facts[0]
    assert sum(f[8]["cols"]) == 179 and f[8]["comp"] == 96
    assert len(f[7]["picks"]) >= 1 and len(f[6]["picks"]) >= 1


# ----------------------------------------------------------------------------- the loop's end
def test_two_live():
    b, facts, box_tier = _hand("two_live")
    f = facts[0]
    assert f[4]["picks"] == [((0, 1, 2, 3), (0, 2, 4, 5))]
    assert f[3]["live"] == 2 and f[3]["subsets"] == []       # two live pickers: nothing at tier 3
    assert f[2]["live"] == 2 and f[2]["subsets"] == [((0, 1), 2)]
    assert f[2]["picks"] == [((0, 1), (1, 3))]               # B
    assert box_tier.tolist() == vm.TWO_LIVE_BOX_TIER


def test_three_live():
    b, facts, box_tier = _hand("three_live")
    f = facts[0]
    assert f[4]["picks"] == [((0, 1, 2, 3), (0, 3, 6, 8))]
    assert f[3]["live"] == 3 and f[3]["subsets"] == [((0, 1, 2), 5)]
    assert f[3]["picks"] == [((0, 1, 2), (2, 5, 7))]         # C
    assert f[2]["live"] == 2 and f[2]["picks"] == [((0, 1), (1, 4))]
    assert box_tier.tolist() == [4, 2, 3, 4, 2, 3, 4, 3, 4]
    # two_live is this micrograph without C
    two = _hand("two_live")[0]
    keep = np.array([0, 1, 3, 4, 6, 8])
    assert np.array_equal(b.x[keep], two.x) and np.array_equal(b.score[keep], two.score)


def test_all_explained():
    b, facts, box_tier = _hand("all_explained")
    f = facts[0]
    assert b.k == 5 and len(f[5]["picks"]) == 2 and (box_tier == 5).all()
    assert sorted(i for _, mem in f[5]["picks"] for i in mem) == list(range(10))
    for tier in (4, 3, 2):
        assert f[tier]["live"] == 0 and f[tier]["subsets"] == []


# ----------------------------------------------------------------------------- routes in a tier
@pytest.mark.parametrize("name,per_picker,sub_boxes", [("deferred_tier", 2400, 4700),
                                                       ("fused_tier", 1600, 3100)])
def test_route_edges_inside_a_tier(name, per_picker, sub_boxes):
    b, facts, box_tier = _lattice(name)
    f = facts[0]
    assert np.diff(b.box_off).tolist() == [per_picker] * 3
    assert len(b.x) == 3 * per_picker > vm.FUSED_MAX_BOXES       # tier 3: deferred
    assert f[3]["cols"] == [50] and len(f[3]["picks"]) == 50
    assert f[2]["subsets"] == [(S, sub_boxes) for S in vu.subsets(3, 2)]
    assert (sub_boxes > vm.FUSED_MAX_BOXES) == (name == "deferred_tier")
    assert f[2]["cols"] == [60, 60, 60] and len(f[2]["picks"]) == 180
    assert f[3]["comp"] == 1 and f[2]["comp"] == 1
    assert np.bincount(box_tier).tolist() == [3 * per_picker - 510, 0, 360, 150]
    # the file order is shuffled: a picker's explained boxes are not a prefix
    seg = box_tier[:per_picker]
    assert (seg[:170] == 0).any() and (seg[170:] != 0).any()
    # only planted groups overlap: no coordinate leaves its 40-pixel slot
    assert ((b.x % 40 >= 5) & (b.x % 40 <= 6) & (b.y % 40 >= 5) & (b.y % 40 <= 6)).all()


def test_hand_micrograph_goes_in_front():
    """The mixed pseudo-batch of the GPU test: the hand case's tier-2 pseudo-micrographs (a few
    boxes) and the deferred micrograph's in one run."""
    h = vu.hand_batch()
    b = vm.pack(3, 10, [vm.hand_mg(), vm.deferred_tier()])
    assert np.array_equal(b.x[:9], h.x) and np.array_equal(b.score[:9], h.score)
    assert b.box_off[:4].tolist() == h.box_off.tolist() and b.box_size == h.box_size
    assert np.array_equal(b.x[9:], _lattice("deferred_tier")[0].x)
