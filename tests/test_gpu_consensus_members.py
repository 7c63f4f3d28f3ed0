"""``repic consensus --members`` on the GPU: per written pick its box from every picker, and
every picker's boxes that are in no written pick.

* the members kernels alone (rgc_pick_members) against plain Python - the stable reverse sort
  of test_gpu_consensus.pick_case, then a set complement in file order - with segment sizes on
  the wave and 256-thread tile edges of the compaction and every num_particles case
* its refusals, and two chosen columns sharing a box: an error, and the context still works
* the command on the small goldens: the .box files and the summary are those of the plain
  command, every _members.tsv equals a model put together from rgc_run's members
  (test_gpu_parity pins them to the reference's goldens), a plain consensus' chosen columns
  and the parsed inputs; the same under --num_particles, --get_cc, the multi-kernel route and
  split device batches; failure semantics
"""
import os

import numpy as np
import pytest

from golden_util import load_case, make_inputs
from test_consensus_members_host import _model
from test_gpu_consensus import CONF_VALUES, _boxes, _consensus, _small_batch, _summary

pytestmark = pytest.mark.gpu

K = 3
# (boxes of picker 0, 1, 2), chosen columns, other columns
LAYOUT = [
    ((64, 65, 63), 30, 50),
    ((256, 257, 255), 100, 200),
    ((1025, 1025, 1025), 1025, 100),      # every box of every picker chosen: no leftovers
    ((1, 1, 1), 1, 0),
    ((0, 1, 64), 0, 0),                   # a picker without boxes: zero columns
    ((257, 64, 1025), 0, 60),             # nothing chosen
    ((65, 256, 63), 0, 0),                # zero columns, boxes everywhere
    ((255, 1025, 257), 70, 300),          # more chosen than num_particles = 64
]


@pytest.fixture(scope="module")
def ctx():
    from repic_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def mem_case():
    """One k = 3 batch and, per micrograph, the reference order of its chosen columns."""
    rng = np.random.default_rng(77)
    box_off, col_off = [0], [0]
    members, x = [], []
    for counts, n_ch, n_other in LAYOUT:
        b = [box_off[-1] + int(np.sum(counts[:p])) for p in range(K)]
        box_off += [b[p] + counts[p] for p in range(K)]
        # chosen columns: disjoint members (a prefix of one permutation per picker)
        perm = [rng.permutation(counts[p]) for p in range(K)]
        cols = [[b[p] + int(perm[p][j]) for p in range(K)] for j in range(n_ch)]
        cols += [[b[p] + int(rng.integers(counts[p])) for p in range(K)] for _ in range(n_other)]
        xs = [1] * n_ch + [0] * n_other
        o = rng.permutation(len(cols))
        members += [cols[j] for j in o]
        x += [xs[j] for j in o]
        col_off.append(col_off[-1] + len(cols))
    nc, N = col_off[-1], box_off[-1]
    members = np.array(members, np.int32).reshape(nc, K)
    x = np.array(x, np.uint8)
    conf = CONF_VALUES[rng.integers(0, len(CONF_VALUES), nc)]
    cons = members[np.arange(nc), rng.integers(0, K, nc)]
    bx = rng.integers(-50, 4096, N) + rng.choice([0.0, 0.5, 0.25, -0.25], N)
    by = rng.integers(-50, 4096, N) + rng.choice([0.0, 0.5, 0.75], N)
    order = []
    for m in range(len(LAYOUT)):
        a, b = col_off[m], col_off[m + 1]
        sel = [j for j in range(b - a) if x[a + j] == 1]
        ranked = sorted(zip(sel, [conf[a + j] for j in sel]), key=lambda t: t[1], reverse=True)
        order.append(np.array([j for j, _ in ranked], np.int64))
    col_off, box_off = np.array(col_off, np.int64), np.array(box_off, np.int64)
    for a in (col_off, box_off, members, x, conf, cons, bx, by):
        a.setflags(write=False)
    return col_off, x, conf, cons, members, box_off, bx, by, order


def _same(got, want):
    want = np.asarray(want, np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))


@pytest.mark.parametrize("num_particles", [None, 0, 1, 64])
def test_pick_members_matches_python(mem_case, ctx, num_particles):
    col_off, x, conf, cons, members, box_off, bx, by, order = mem_case
    (pick_off, px, py, pconf, pcol, pmx, pmy, left_off, left_x, left_y,
     in_clique) = ctx.pick_members(K, col_off, x, conf, cons, members, box_off, bx, by,
                                   num_particles)
    w_off, w_col, w_loff, w_lx, w_ly, w_mem, w_cl = [0], [], [0], [], [], [], []
    for m, o in enumerate(order):
        keep = o if num_particles is None else o[:num_particles]
        g = int(col_off[m]) + keep
        w_off.append(w_off[-1] + len(keep))
        w_col.append(keep)
        w_mem.append(members[g])
        used = set(members[g].reshape(-1).tolist())
        for p in range(K):
            s = m * K + p
            left = [b for b in range(int(box_off[s]), int(box_off[s + 1])) if b not in used]
            w_lx += left
            w_loff.append(len(w_lx))
            w_cl.append(len(set(members[col_off[m]:col_off[m + 1], p].tolist())))
    w_col = np.concatenate(w_col).astype(np.int32)
    w_mem = np.concatenate(w_mem)
    g_col = np.repeat(col_off[:-1], np.diff(w_off)) + w_col
    assert np.array_equal(pick_off, np.array(w_off, np.int64))
    assert np.array_equal(pcol, w_col)
    _same(px, np.rint(bx[cons[g_col]]))
    _same(py, np.rint(by[cons[g_col]]))
    assert np.array_equal(pconf.view(np.uint32), conf[g_col].view(np.uint32))
    _same(pmx, np.rint(bx[w_mem]))
    _same(pmy, np.rint(by[w_mem]))
    assert np.array_equal(left_off, np.array(w_loff, np.int64))
    _same(left_x, np.rint(bx[np.array(w_lx, np.int64)]))
    _same(left_y, np.rint(by[np.array(w_lx, np.int64)]))
    assert in_clique.dtype == np.int32 and np.array_equal(in_clique, np.array(w_cl, np.int32))
    # the layout's promised cases
    n_left = np.diff(left_off).reshape(-1, K)
    if num_particles is None:
        assert not n_left[2].any()                                  # no leftovers
    assert np.array_equal(n_left[5], np.array(LAYOUT[5][0]))        # nothing chosen
    assert np.array_equal(n_left[4], np.array(LAYOUT[4][0])) and not in_clique[12:15].any()


def test_pick_members_empty_batches(ctx):
    z = np.zeros(0)
    out = ctx.pick_members(K, [0], z, z, z, z, [0], z, z)
    assert out[0].tolist() == [0] and out[7].tolist() == [0] and out[5].shape == (0, K)
    out = ctx.pick_members(2, [0, 0], z, z, z, z, [0, 2, 3], [1.5, 2.5, -0.5], [0.0, 1.0, 2.0])
    assert out[0].tolist() == [0, 0] and out[7].tolist() == [0, 2, 3]
    _same(out[8], [2.0, 2.0, -0.0])
    assert out[10].tolist() == [0, 0]


def test_pick_members_shared_box_is_an_error_and_context_survives(mem_case, ctx):
    from repic_amd import _lib
    box_off = [0, 4, 8]
    bx = by = np.arange(8.0)
    members = [[0, 4], [1, 5], [0, 6]]              # columns 0 and 2 share box 0
    a = (2, [0, 3], [1, 1, 1], [0.5, 0.4, 0.3], [0, 1, 0], members, box_off, bx, by)
    with pytest.raises(_lib.RGCError, match="share a box"):
        ctx.pick_members(*a)
    # more picks than a picker has boxes
    with pytest.raises(_lib.RGCError, match="share a box"):
        ctx.pick_members(2, [0, 3], [1, 1, 1], [0.5, 0.4, 0.3], [0, 0, 0],
                         [[0, 2], [0, 3], [0, 4]], [0, 1, 5], bx[:5], by[:5])
    z = np.zeros(0)
    for bad, pat in (
            ((9, [0, 0], z, z, z, z, list(range(10)), np.arange(9.0), np.arange(9.0)), "k must be"),
            (a[:1] + ([1, 3],) + a[2:], "start at 0"),
            (a[:5] + ([[0, 4], [1, 5], [0, 8]],) + a[6:], "outside"),   # member out of range
            (a[:5] + ([[0, 4], [1, 5], [4, 6]],) + a[6:], "outside"),   # ... of its picker
            (a[:4] + ([0, 1, 8],) + a[5:], "outside"),                  # consensus box
            (a[:6] + ([0, 5, 4],) + a[7:], "decrease")):
        with pytest.raises(_lib.RGCError, match=pat):
            ctx.pick_members(*bad)
    sb = _small_batch()
    ctx.submit(sb.n_mg, sb.k, sb.box_size, sb.box_off, sb.id_base, sb.x, sb.y, sb.score)
    try:
        with pytest.raises(_lib.RGCError, match="rgc_wait"):
            ctx.pick_members(*a)
    finally:
        ctx.wait()
    out = ctx.pick_members(2, [0, 3], [1, 1, 0], [0.5, 0.4, 0.3], [0, 1, 0], members, box_off,
                           bx, by)
    assert out[4].tolist() == [0, 1] and out[5].tolist() == [[0.0, 4.0], [1.0, 5.0]]
    assert out[8].tolist() == [2.0, 3.0, 6.0, 7.0] and out[10].tolist() == [2, 3]
    test_pick_members_matches_python(mem_case, ctx, 1)


# ----------------------------------------------------------------------------- the command
def _listing(d):
    out = {}
    for f in sorted(os.listdir(d)):
        with open(os.path.join(d, f), "rb") as fh:
            out[f] = fh.read()
    return out


def _chunk(name, root, in_dir):
    from repic_amd.ingest import DirIndex, list_methods, micrograph_names, plan_chunk
    meta, _ = load_case(name)
    methods = list_methods(in_dir)
    index = DirIndex(in_dir, methods, meta["listing"])
    names = micrograph_names(index, methods)
    return methods, plan_chunk(in_dir, methods, index, names, len(methods), meta["box"], 0, None)


def _expected_tables(ctx, methods, ch, num_particles=None, get_cc=False, no_fused=False):
    """{base: (table text, boxes per picker, in_clique per picker, picks, .box coordinates)} of
    the chunk's ok micrographs, from rgc_run's members, a plain consensus and the inputs."""
    from repic_amd import _lib
    b, k = ch.batch, len(methods)
    fl = (_lib.F_GET_CC if get_cc else 0) | (_lib.F_NO_FUSED if no_fused else 0)
    a = (b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score)
    run = ctx.run(*a, flags=fl | _lib.F_MEMBERS | _lib.F_HOST_OUTPUTS)
    by_rows = []
    for m in range(b.n_mg):
        c0, C = int(run.clique_base[m]), int(run.clique_cnt[m])
        by_rows.append({tuple(r): mem for r, mem in zip(run.rows[c0:c0 + C].tolist(),
                                                        run.members[c0:c0 + C].tolist())})
    r = ctx.consensus(*a, flags=fl | _lib.F_HOST_OUTPUTS, num_particles=num_particles)
    out = {}
    for mg in ch.mgs:
        if mg.status != "ok":
            continue
        m = mg.slot
        assert r.run.status[m] == _lib.OK
        c0 = int(r.run.clique_base[m])
        picks, used, xy = [], set(), []
        for i in range(int(r.pick_off[m]), int(r.pick_off[m + 1])):
            c = c0 + int(r.pcol[i])
            mem = by_rows[m][tuple(r.run.rows[c].tolist())]
            picks.append(([(b.x[g], b.y[g]) for g in mem], r.pconf[i]))
            used.update(mem)
            xy.append((r.px[i], r.py[i]))
        assert len(used) == k * len(picks)
        left, boxes, incl = [], [], []
        for p in range(k):
            lo, hi = int(b.box_off[m * k + p]), int(b.box_off[m * k + p + 1])
            left.append([(b.x[g], b.y[g]) for g in range(lo, hi) if g not in used])
            boxes.append(hi - lo)
            incl.append(len({mem[p] for mem in by_rows[m].values()}))
        out[mg.base] = (_model(methods, (picks, left)), boxes, incl, len(picks), xy)
    return out


def _check_command(name, tmp_path, ctx, num_particles=None, get_cc=False, no_fused=False, **kw):
    from repic_amd.commands import consensus
    from repic_amd.writers import read_members
    meta, _ = load_case(name)
    in_dir = make_inputs(name, str(tmp_path))
    plain, mem = str(tmp_path / "plain"), str(tmp_path / "mem")
    opts = dict(num_particles=num_particles, get_cc=get_cc, **kw)
    if no_fused:
        opts["no_fused"] = True
    assert _consensus(in_dir, plain, meta, **opts) is None
    assert _consensus(in_dir, mem, meta, members=True, **opts) is None
    want, got = _listing(plain), _listing(mem)
    methods, ch = _chunk(name, str(tmp_path), in_dir)
    assert ch.crash is None
    exp = _expected_tables(ctx, methods, ch, num_particles, get_cc, no_fused)
    assert exp
    # the plain command's files, unchanged, plus one table per ok micrograph and the run's file
    assert sorted(got) == sorted(list(want) + [b + "_members.tsv" for b in exp]
                                 + [consensus.PICKERS])
    for f in want:
        assert got[f] == want[f], f
    k = len(methods)
    lines = got[consensus.PICKERS].decode().split("\n")
    assert lines[0] + "\n" == consensus.PICKERS_HEADER and lines[-1] == ""
    pick_rows = [ln.split("\t") for ln in lines[1:-1]]
    ok_bases = [r[0] for r in _summary(mem) if r[1] == "ok"]
    assert [r[0] for r in pick_rows] == [b for b in ok_bases for _ in range(k)]
    assert sorted(ok_bases) == sorted(exp)
    for j, base in enumerate(ok_bases):
        table, boxes, incl, n, xy = exp[base]
        assert got[base + "_members.tsv"].decode() == table, base
        for p in range(k):
            assert pick_rows[j * k + p][1:] == [methods[p], str(boxes[p]), str(incl[p]), str(n)]
        # invariants, from the files alone
        coords, labels, weights = read_members(os.path.join(mem, base + "_members.tsv"))
        assert labels == methods
        box = [ln.split("\t") for ln in got[base + ".box"].decode().splitlines()]
        assert len(box) == n
        for i, ln in enumerate(box):
            assert (float(ln[0]), float(ln[1])) in coords[i] and all(coords[i])
            assert (float(ln[0]), float(ln[1])) == tuple(xy[i])
        for p in range(k):
            assert sum(1 for row in coords if row[p]) == boxes[p]
            assert all(sum(1 for v in row if v) == 1 for row in coords[n:])
    return exp


@pytest.mark.parametrize("name", ["c1_10017", "ties", "skips", "syn_k3_frac", "syn_k5", "syn_k8"])
def test_members_command_matches_model(name, tmp_path, ctx):
    _check_command(name, tmp_path, ctx)


def test_members_command_num_particles(tmp_path, ctx):
    exp = _check_command("c1_10017", tmp_path, ctx, num_particles=5)
    assert max(v[3] for v in exp.values()) == 5


def test_members_command_get_cc(tmp_path, ctx):
    _check_command("c1_10017", tmp_path, ctx, get_cc=True)


def test_members_command_multikernel_route(tmp_path, ctx):
    _check_command("c1_10017", tmp_path, ctx, no_fused=True)


def test_members_command_split_batches(tmp_path, ctx):
    """Several device batches per chunk give the same files as one."""
    one = _check_command("c1_10017", tmp_path, ctx)
    meta, _ = load_case("c1_10017")
    split = str(tmp_path / "split")
    assert _consensus(os.path.join(str(tmp_path), "in"), split, meta, members=True,
                      batch_boxes=2000) is None
    assert one and _listing(split) == _listing(str(tmp_path / "mem"))


def test_members_command_failure_semantics(tmp_path):
    meta, _ = load_case("crash_noedges")
    in_dir = make_inputs("crash_noedges", str(tmp_path))
    plain, mem = str(tmp_path / "plain"), str(tmp_path / "mem")
    e0 = _consensus(in_dir, plain, meta)
    e1 = _consensus(in_dir, mem, meta, members=True)
    assert e0 is not None and type(e1) is type(e0) and str(e1) == str(e0)
    assert _boxes(mem) == _boxes(plain)
    ok = [r[0] for r in _summary(mem) if r[1] == "ok"]
    assert _summary(mem) == _summary(plain)
    tables = sorted(f for f in os.listdir(mem) if f.endswith("_members.tsv"))
    assert tables == sorted(b + "_members.tsv" for b in ok)
    for b in ok:
        assert os.path.exists(os.path.join(mem, b + ".box"))


# ----------------------------------------------------------------------------- the library call
def test_consensus_members_call_timing_and_bytes(ctx):
    """Context.consensus(members=True): the plain call's picks, the new timing section after
    k_pick_emit, and the bus bytes of the new arrays: 16 k B per pick, 16 B per leftover, 8 B
    per segment and the 4-byte flag down; 16 B per segment + 16 B and 1 B per micrograph up."""
    from repic_amd import _lib
    b = _small_batch()
    a = (b.n_mg, b.k, b.box_size, b.box_off, b.id_base, b.x, b.y, b.score)
    plain = ctx.consensus(*a, timing=True)
    assert "k_pick_members" not in [n for n, _ in ctx.kernel_times()]
    assert plain.pmx is None and plain.left_off is None
    r = ctx.consensus(*a, timing=True, members=True)
    names = [n for n, _ in ctx.kernel_times()]
    assert names.index("k_pick_emit") < names.index("k_pick_members")
    for f in ("pick_off", "px", "py", "pconf", "pcol", "sel_cnt", "ilp_status"):
        assert np.array_equal(getattr(r, f), getattr(plain, f)), f
    S, n = b.n_mg * b.k, r.n_picked
    assert r.pmx.shape == r.pmy.shape == (n, b.k) and n > 0
    picks = np.diff(r.pick_off)
    assert np.array_equal(np.diff(r.left_off),
                          np.diff(b.box_off) - np.repeat(picks, b.k))
    L = int(r.left_off[-1])
    assert len(r.left_x) == len(r.left_y) == L > 0 and r.in_clique.shape == (S,)
    assert (r.in_clique >= np.repeat(picks, b.k)).all()
    assert (r.in_clique <= np.diff(b.box_off)).all()
    # each pick's consensus coordinate is one of its members'
    assert ((r.pmx == r.px[:, None]) & (r.pmy == r.py[:, None])).any(axis=1).all()
    assert r.d2h_bytes - plain.d2h_bytes == 16 * b.k * n + 16 * L + 8 * S + 4
    assert r.h2d_bytes - plain.h2d_bytes == 16 * (S + 1) + b.n_mg
    with pytest.raises(_lib.RGCError, match="MULTI_OUT"):
        ctx.consensus(*a, flags=_lib.F_MULTI_OUT, members=True)
    # the per-clique members in HBM are the run's: with host outputs they come back as well
    rh = ctx.consensus(*a, flags=_lib.F_HOST_OUTPUTS, members=True)
    assert rh.run.members is not None and np.array_equal(rh.pmx, r.pmx)
    g = rh.run.members[np.repeat(rh.run.clique_base, picks) + rh.pcol]
    assert np.array_equal(rh.pmx, np.rint(b.x[g])) and np.array_equal(rh.pmy, np.rint(b.y[g]))
