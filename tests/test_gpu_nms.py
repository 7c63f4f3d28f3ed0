"""Greedy NMS on the device (rgc_nms, ``repic nms``, ``consensus --dedup_ji``) against the
plain-Python oracle of tests/nms_util.py.  The shapes are the smallest at which the kernel can go
wrong: sizes around the 64-lane wave and the 256-thread workgroup, one trip and several trips of
the workgroup, chains that need as many rounds as they have boxes, and one large segment."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

import nms_util
from golden_util import GOLDEN, load_case, make_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _run(ctx, segs, box, t, **kw):
    """segments [(x, y)] -> (keep, kept) of one device call"""
    off = np.concatenate([[0], np.cumsum([len(x) for x, _ in segs])]).astype(np.int64)
    x = np.concatenate([np.asarray(x, np.float64) for x, _ in segs] or [np.zeros(0)])
    y = np.concatenate([np.asarray(y, np.float64) for _, y in segs] or [np.zeros(0)])
    keep, kept = ctx.nms(off, x, y, box, t, **kw)
    assert keep.dtype == np.uint8 and kept.dtype == np.int64
    assert keep.shape == x.shape and kept.shape == (len(segs),)
    return keep, kept, off, x, y


def _assert_oracle(ctx, segs, box, t):
    keep, kept, off, x, y = _run(ctx, segs, box, t)
    wk, wn = nms_util.nms_oracle_segments(off, x, y, box, t)
    assert np.array_equal(keep, wk), np.flatnonzero(keep != wk)[:10]
    assert np.array_equal(kept, wn)
    return keep, kept


# ----------------------------------------------------------------------------- hand cases
def test_no_segments_and_empty_segments(ctx):
    keep, kept = ctx.nms([0], [], [], 10, 0.3)
    assert keep.shape == (0,) and kept.shape == (0,)
    keep, kept = ctx.nms([0, 0, 0], [], [], 10, 0.3)
    assert keep.shape == (0,) and kept.tolist() == [0, 0]
    e = ([], [])
    keep, kept, *_ = _run(ctx, [e, ([0, 1], [0, 0]), e, e, ([7], [7]), e], 10, 0.3)
    assert keep.tolist() == [1, 0, 1] and kept.tolist() == [0, 1, 0, 0, 1, 0]


def test_one_box_identical_boxes_shared_edge(ctx):
    assert _run(ctx, [([3], [4])], 10, 0.3)[0].tolist() == [1]
    assert _run(ctx, [([3, 3], [4, 4])], 10, 0.3)[0].tolist() == [1, 0]
    # two boxes sharing an edge at T = 0: overlap 0, both kept
    assert _run(ctx, [([0, 10], [0, 0])], 10, 0.0)[0].tolist() == [1, 1]
    assert _run(ctx, [([0, 0], [0, 10])], 10, 0.0)[0].tolist() == [1, 1]
    # ... and one pixel of overlap at T = 0 suppresses
    assert _run(ctx, [([0, 9], [0, 9])], 10, 0.0)[0].tolist() == [1, 0]


def test_threshold_boundary(ctx):
    from repic_amd import _lib
    # overlap 5 x 10 = 50: JI = 50 / 150, equal to T = 1/3 in f64 -> kept; suppressed at 0.3
    assert nms_util.jaccard(0.0, 0.0, 5.0, 0.0, 10.0) == 1 / 3
    assert _run(ctx, [([0, 5], [0, 0])], 10, 1 / 3)[0].tolist() == [1, 1]
    assert _run(ctx, [([0, 5], [0, 0])], 10, 0.3)[0].tolist() == [1, 0]
    ic = _lib.ji_cutoff(10, 0.3)[0]          # suppressed <=> area > ic
    assert 45 <= ic < 48
    assert _run(ctx, [([0, 5], [0, 1])], 10, 0.3)[0].tolist() == [1, 1]     # area 45
    assert _run(ctx, [([0, 4], [0, 2])], 10, 0.3)[0].tolist() == [1, 0]     # area 48
    # every offset of a second box, both orders of the pair: the integer cut decides
    offs = [(dx, dy) for dx in range(-10, 11) for dy in range(-10, 11)]
    segs = [([0, dx], [0, dy]) for dx, dy in offs] + [([dx, 0], [dy, 0]) for dx, dy in offs]
    keep = _run(ctx, segs, 10, 0.3)[0].reshape(-1, 2)
    area = np.array([(10 - abs(dx)) * (10 - abs(dy)) for dx, dy in offs] * 2)
    assert keep[:, 0].all() and np.array_equal(keep[:, 1] == 0, area > ic)


# ----------------------------------------------------------------------------- chains
@pytest.mark.parametrize("n", [257, 600])
def test_chains(ctx, n):
    """Boxes at x = 3 i: only i +- 1 conflict (overlap 7 x 10 = 70 > cut, 4 x 10 = 40 not).
    Along the chain the keep / suppress pattern alternates and needs n rounds (the cap is n + 1);
    reversed and shuffled orders too."""
    assert nms_util.jaccard(0.0, 0.0, 3.0, 0.0, 10.0) > 0.3 > nms_util.jaccard(0.0, 0.0, 6.0, 0.0, 10.0)
    pos = 3.0 * np.arange(n)
    zero = np.zeros(n)
    perm = np.random.default_rng(n).permutation(n)
    keep, kept = _assert_oracle(ctx, [(pos, zero), (pos[::-1], zero), (pos[perm], zero),
                                      (zero, pos)], 10, 0.3)
    assert keep[:n].tolist() == [1 - (i & 1) for i in range(n)]
    assert kept[0] == kept[1] == kept[3] == (n + 1) // 2


def test_identical_boxes(ctx):
    keep, kept, *_ = _run(ctx, [(np.full(1000, 12.5), np.full(1000, -3.25))], 10, 0.3)
    assert keep.tolist() == [1] + [0] * 999 and kept.tolist() == [1]


# ----------------------------------------------------------------------------- mixed sizes
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]


def _mixed(decimals):
    """~300 crowded segments, every size of SIZES present (about one box per 25 px^2, box 10)"""
    rng = np.random.default_rng(77)
    sizes = SIZES + rng.choice(SIZES, 290, p=[.12, .12, .12, .12, .12, .12, .08, .08, .08, .04]).tolist()
    segs = []
    for n in sizes:
        side = 10.0 + np.sqrt(25.0 * n)
        xy = rng.uniform(0, side, (2, n))
        xy = np.floor(xy) if decimals == 0 else np.round(xy, decimals)
        segs.append((xy[0], xy[1]))
    return segs


def test_mixed_segment_sizes_integer(ctx):
    keep, kept = _assert_oracle(ctx, _mixed(0), 10, 0.3)
    assert 0.1 * len(keep) < keep.sum() < 0.9 * len(keep)


def test_mixed_segment_sizes_fractional(ctx):
    segs = _mixed(3)
    keep, _ = _assert_oracle(ctx, segs, 10, 0.3)
    assert 0.1 * len(keep) < keep.sum() < 0.9 * len(keep)
    # the same call shifted by 2^40 (the sums round: the oracle rounds the same way)
    _assert_oracle(ctx, [(x + 2.0 ** 40, y + 2.0 ** 40) for x, y in segs[:150]], 10, 0.3)
    _assert_oracle(ctx, [(x + 2.0 ** 40, y - 2.0 ** 40) for x, y in segs[150:]], 10, 0.0)


def test_non_finite_coordinates(ctx):
    rng = np.random.default_rng(5)
    n = 700
    x = np.floor(rng.uniform(0, 140, n))
    y = np.floor(rng.uniform(0, 140, n))
    base = _run(ctx, [(x, y)], 10, 0.3)[0].astype(bool)
    assert np.array_equal(base, nms_util.nms_oracle(x, y, 10, 0.3))
    bad = [(np.nan, 5.0), (5.0, np.nan), (np.inf, 5.0), (5.0, np.inf), (-np.inf, 5.0),
           (5.0, -np.inf), (np.nan, np.nan), (np.inf, -np.inf)]
    at = np.sort(rng.choice(n, 5 * len(bad), replace=False))
    xs, ys, finite = [], [], []
    j = 0
    for i in range(n):
        if j < len(at) and at[j] == i:
            bx, by = bad[j % len(bad)]
            xs.append(bx), ys.append(by), finite.append(False)
            j += 1
        xs.append(x[i]), ys.append(y[i]), finite.append(True)
    finite = np.array(finite)
    keep = _run(ctx, [(xs, ys)], 10, 0.3)[0].astype(bool)
    assert keep[~finite].all()
    assert np.array_equal(keep[finite], base)
    # a segment of non-finite boxes only
    assert _run(ctx, [([np.nan, np.nan, np.inf], [0.0, 0.0, 1.0])], 10, 0.0)[0].tolist() == [1, 1, 1]


def test_one_large_segment(ctx):
    rng = np.random.default_rng(1)
    n = 20000
    x = rng.integers(0, 500, n).astype(np.float64)
    y = rng.integers(0, 500, n).astype(np.float64)
    want = nms_util.nms_oracle(x, y, 10, 0.3)
    assert 0.1 * n < want.sum() < 0.9 * n
    keep, kept, *_ = _run(ctx, [(x, y)], 10, 0.3)
    assert np.array_equal(keep.astype(bool), want) and kept.tolist() == [int(want.sum())]
    assert nms_util.characterised(x, y, keep, 10, 0.3) is None


# ----------------------------------------------------------------------------- refusals
def _raw(c, n_seg, seg_off, x, y, box, t, keep=True, kept=True):
    from repic_amd import _lib
    off = np.ascontiguousarray(seg_off, np.int64)
    xa = None if x is None else np.ascontiguousarray(x, np.float64)
    ya = None if y is None else np.ascontiguousarray(y, np.float64)
    n = max(1, 0 if xa is None else len(xa))
    ko, kn = np.zeros(n, np.uint8), np.zeros(max(1, min(n_seg, 16)), np.int64)
    ni = _lib.NmsIn(n_seg, off.ctypes.data, None if xa is None else xa.ctypes.data,
                    None if ya is None else ya.ctypes.data, int(box), float(t), 0)
    _lib._check(_lib.lib.rgc_nms(c._p, C.byref(ni), ko.ctypes.data if keep else None,
                                 kn.ctypes.data if kept else None))
    return ko, kn


def test_refusals_leave_the_context_usable():
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch
    c = _lib.Context(0)
    x, y = [0.0, 1.0, 50.0], [0.0, 0.0, 0.0]
    good = (1, [0, 3], x, y, 10, 0.3)

    def valid():
        assert _raw(c, *good)[0].tolist() == [1, 0, 1]
    try:
        valid()
        with pytest.raises(_lib.RGCError, match="null argument"):
            _raw(c, 1, [0, 3], None, y, 10, 0.3)
        with pytest.raises(_lib.RGCError, match="null argument"):
            _raw(c, 1, [0, 3], x, None, 10, 0.3)
        with pytest.raises(_lib.RGCError, match="null argument"):
            _raw(c, 1, [0, 3], x, y, 10, 0.3, keep=False)
        with pytest.raises(_lib.RGCError, match="null argument"):
            _raw(c, 1, [0, 3], x, y, 10, 0.3, kept=False)
        with pytest.raises(_lib.RGCError, match="n_seg"):
            _raw(c, -1, [0, 3], x, y, 10, 0.3)
        with pytest.raises(_lib.RGCError, match="n_seg"):
            _raw(c, 2 ** 31, [0, 3], x, y, 10, 0.3)
        with pytest.raises(_lib.RGCError, match="start at 0"):
            _raw(c, 1, [1, 3], x, y, 10, 0.3)
        with pytest.raises(_lib.RGCError, match="non-decreasing"):
            _raw(c, 2, [0, 3, 2], x, y, 10, 0.3)
        with pytest.raises(_lib.RGCError, match="2\\^31 - 1 boxes"):
            _raw(c, 2, [0, 3, 2 ** 31], x, y, 10, 0.3)
        for box in (0, -10, 2 ** 26 + 1):
            with pytest.raises(_lib.RGCError, match="box_size"):
                _raw(c, 1, [0, 3], x, y, box, 0.3)
        for t in (1.0, -0.1, float("nan"), float("inf")):
            with pytest.raises(_lib.RGCError, match="ji_threshold"):
                _raw(c, 1, [0, 3], x, y, 10, t)
        valid()
        assert _raw(c, 1, [0, 3], x, y, 2 ** 26, 0.0)[0].tolist() == [1, 0, 0]
        # a submitted run that awaits rgc_wait
        cfg = synth.SynthConfig(k=3, n_true=20, box=180, width=1024, height=1024, seed=5)
        b = Batch.pack(cfg.k, cfg.box, synth.batch(cfg, 2))
        c.submit(b.n_mg, cfg.k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score)
        with pytest.raises(_lib.RGCError, match="awaits rgc_wait"):
            _raw(c, *good)
        c.wait()
        valid()
    finally:
        c.close()


def test_too_many_conflict_edges_refused_after_the_count(ctx):
    """Two segments of 46,342 identical boxes: 1,073,767,311 conflict edges each, together more
    than 2^31 - 1 (one alone fits).  The call fails after the count launch, names the limit, and
    the context stays usable."""
    from repic_amd import _lib
    n = 46342
    assert n * (n - 1) // 2 <= 2 ** 31 - 1 < n * (n - 1)
    z = np.zeros(2 * n)
    with pytest.raises(_lib.RGCError, match="2\\^31 - 1 conflict edges"):
        ctx.nms([0, n, 2 * n], z, z, 10, 0.3)
    assert _run(ctx, [([0, 1], [0, 0])], 10, 0.3)[0].tolist() == [1, 0]


def test_repeatable_and_timing_names_the_kernels(ctx):
    segs = _mixed(0)[:60]
    a = _run(ctx, segs, 10, 0.3)[0]
    b = _run(ctx, segs, 10, 0.3, timing=True)[0]
    assert np.array_equal(a, b)
    names = [n for n, _ in ctx.kernel_times()]
    assert names == ["k_nms_count", "k_nms"]
    assert all(ms >= 0 for _, ms in ctx.kernel_times())
    h2d, d2h = ctx.nms_bytes
    assert h2d > 36 * len(a) and d2h > len(a)


def test_python_api(ctx):
    from repic_amd import nms
    rng = np.random.default_rng(9)
    n = 400
    x, y = np.floor(rng.uniform(0, 100, (2, n)))
    score = np.round(rng.uniform(-1, 1, n), 1)      # many ties
    score[::37] = np.nan
    mask = nms.nms_boxes(x, y, score, 10, 0.3, ctx)
    order = nms.nms_order(score)
    assert mask.dtype == bool
    assert np.array_equal(mask[order], nms_util.nms_oracle(x[order], y[order], 10, 0.3))
    got = nms.nms_keep([(x, y), ([], []), (y, x)], 10, ctx=ctx)
    assert [len(g) for g in got] == [n, 0, n]
    assert np.array_equal(got[0], nms_util.nms_oracle(x, y, 10, 0.3))
    assert np.array_equal(got[2], nms_util.nms_oracle(y, x, 10, 0.3))
    assert nms.nms_keep([], 10, ctx=ctx) == []


# ----------------------------------------------------------------------------- consensus --dedup_ji
def _gc_args(in_dir, out_dir, meta, **kw):
    a = argparse.Namespace(in_dir=in_dir, out_dir=out_dir, box_size=meta["box"], multi_out=False,
                           get_cc=False, batch_boxes=1 << 25, threads=None, device=None,
                           listing=meta["listing"])
    for k_, v in kw.items():
        setattr(a, k_, v)
    return a


def _boxes(d):
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".box"):
            with open(os.path.join(d, f), "rb") as fh:
                out[f] = fh.read()
    return out


def _tsv(path, header):
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] + "\n" == header
    return [ln.split("\t") for ln in lines[1:]]


@pytest.fixture(scope="module", params=["c1_10017", "syn_k4"])
def dedup_case(request, tmp_path_factory):
    """One plain run and the flagged runs of a golden case, and the oracle's survivors of every
    plain ``.box``."""
    from repic_amd.commands import consensus
    name = request.param
    root = tmp_path_factory.mktemp(name)
    meta, _ = load_case(name)
    in_dir = make_inputs(name, str(root))
    dirs = {k: str(root / k) for k in ("plain", "absent", "dedup", "dedup50")}
    consensus.main(_gc_args(in_dir, dirs["plain"], meta, num_particles=None, node_limit=0,
                            dedup_ji=None))
    consensus.main(_gc_args(in_dir, dirs["absent"], meta, num_particles=None, node_limit=0))
    consensus.main(_gc_args(in_dir, dirs["dedup"], meta, num_particles=None, node_limit=0,
                            dedup_ji=0.3))
    last = dict(consensus.LAST_RUN)
    consensus.main(_gc_args(in_dir, dirs["dedup50"], meta, num_particles=50, node_limit=0,
                            dedup_ji=0.3))
    want = {}
    for f, raw in _boxes(dirs["plain"]).items():
        lines = raw.splitlines(keepends=True)
        x, y, _ = nms_util.box_xys(lines)
        keep = nms_util.nms_oracle(x, y, meta["box"], 0.3)
        want[f] = [ln for ln, k in zip(lines, keep) if k]
    return name, meta, dirs, want, last


def test_dedup_files_equal_the_oracle_on_the_plain_files(dedup_case):
    from repic_amd.commands import consensus
    name, meta, dirs, want, last = dedup_case
    plain, got = _boxes(dirs["plain"]), _boxes(dirs["dedup"])
    assert sorted(got) == sorted(plain) and plain
    for f in plain:
        assert got[f] == b"".join(want[f]), f
        x, y, _ = nms_util.box_xys(got[f].splitlines())
        assert nms_util.characterised(x, y, [1] * len(x), meta["box"], 0.3) is None
    assert sorted(os.listdir(dirs["dedup"])) == sorted(
        list(got) + [consensus.SUMMARY, consensus.DEDUP])
    summ = _tsv(os.path.join(dirs["dedup"], consensus.SUMMARY), consensus.SUMMARY_HEADER)
    ded = _tsv(os.path.join(dirs["dedup"], consensus.DEDUP), consensus.DEDUP_HEADER)
    assert consensus.DEDUP_HEADER == "base\tpicked\tsuppressed\twritten\n"
    ok = [r for r in summ if r[1] == "ok"]
    assert [r[0] for r in ded] == [r[0] for r in ok] and ok
    total = 0
    for s, d in zip(ok, ded):
        f = s[0] + ".box"
        n_plain, n_got = plain[f].count(b"\n"), got[f].count(b"\n")
        assert int(s[3]) == n_got
        assert [int(v) for v in d[1:]] == [n_plain, n_plain - n_got, n_got]
        total += n_plain - n_got
    assert last["suppressed"] == total and last["dedup_s"] >= 0
    if name == "c1_10017":     # (the CPU oracle with a HiGHS packing suppresses 42 of 2470)
        assert total >= 1


def test_dedup_before_num_particles(dedup_case):
    _, meta, dirs, want, _ = dedup_case
    got = _boxes(dirs["dedup50"])
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == b"".join(want[f][:50]), f
    assert max(g.count(b"\n") for g in got.values()) == min(50, max(len(w) for w in want.values()))


def test_without_the_flag_nothing_changes(dedup_case):
    from repic_amd.commands import consensus
    _, _, dirs, _, _ = dedup_case
    assert _boxes(dirs["plain"]) == _boxes(dirs["absent"])
    assert sorted(os.listdir(dirs["plain"])) == sorted(os.listdir(dirs["absent"]))
    assert consensus.DEDUP not in os.listdir(dirs["plain"])
    a = _tsv(os.path.join(dirs["plain"], consensus.SUMMARY), consensus.SUMMARY_HEADER)
    b = _tsv(os.path.join(dirs["absent"], consensus.SUMMARY), consensus.SUMMARY_HEADER)
    assert a == b


# ----------------------------------------------------------------------------- repic nms
def test_repic_nms_on_real_picker_files(tmp_path):
    from repic_amd import nms
    from repic_amd.commands import nms as nms_cmd
    in_dir = os.path.join(GOLDEN, "inputs_10017")
    out_dir = str(tmp_path / "out")
    nms_cmd.main(argparse.Namespace(in_dir=in_dir, out_dir=out_dir, box_size=180,
                                    ji_threshold=0.3, threads=None, device=None))
    rows = _tsv(os.path.join(out_dir, nms_cmd.SUMMARY), nms_cmd.SUMMARY_HEADER)
    pickers = sorted(d for d in os.listdir(in_dir) if os.path.isdir(os.path.join(in_dir, d)))
    assert sorted(os.listdir(out_dir)) == sorted(pickers + [nms_cmd.SUMMARY])
    want_rows, removed = [], dict.fromkeys(pickers, 0)
    for m in pickers:
        names = sorted(f for f in os.listdir(os.path.join(in_dir, m)) if f.endswith(".box"))
        assert sorted(os.listdir(os.path.join(out_dir, m))) == names
        for f in names:
            with open(os.path.join(in_dir, m, f), "rb") as fh:
                head, src = nms_util.parse_box_lines(fh.read())
            with open(os.path.join(out_dir, m, f), "rb") as fh:
                ohead, out = nms_util.parse_box_lines(fh.read())
            assert ohead == head
            # the output's lines are a subsequence of the input's: that is the keep mask
            keep, j = np.zeros(len(src), bool), 0
            for i, ln in enumerate(src):
                if j < len(out) and out[j] == ln:
                    keep[i] = True
                    j += 1
            assert j == len(out), (m, f)
            x, y, s = (np.array(v) for v in nms_util.box_xys(src))
            order = nms.nms_order(s)
            assert nms_util.characterised(x[order], y[order], keep[order], 180, 0.3) is None, (m, f)
            want_rows.append([m, f, "filtered", str(len(src)), str(int(keep.sum()))])
            removed[m] += len(src) - int(keep.sum())
    assert rows == want_rows
    # (the CPU oracle removes 1354 / 321 / 342 boxes of crYOLO / deepPicker / topaz)
    assert all(v >= 1 for v in removed.values()), removed
