"""Host side of ``repic consensus --members``, CPU only.

* the parser takes ``--members`` (default False) and still has no ``--multi_out``
* the library exports the three additive symbols and ``has_members()`` finds them
* rgc_write_members writes byte for byte the table reference run_ilp.py:110-119 would build
  from exact picker columns (restated here with np.rint, str(int(...)), str(np.float32(...))),
  next to an unchanged ``.box``; a skipped micrograph gets no table
* read_members reads those files back
* an I/O error names the file that failed
"""
import argparse
import os

import numpy as np
import pytest

from repic_amd import _lib, writers
from repic_amd.commands import consensus
from test_consensus_host import LISTED, _reference_lines

EDGE = [-0.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, -37.25, 1e7, 1234.0]


def test_parser_takes_members_and_still_rejects_multi_out():
    p = argparse.ArgumentParser()
    consensus.add_arguments(p)
    assert p.parse_args(["in", "out", "180"]).members is False
    assert p.parse_args(["in", "out", "180", "--members"]).members is True
    with pytest.raises(SystemExit) as e:
        p.parse_args(["in", "out", "180", "--multi_out"])
    assert e.value.code != 0
    with pytest.raises(SystemExit) as e:
        p.parse_args(["in", "out", "180", "--members", "--multi_out"])
    assert e.value.code != 0


def test_members_symbols_exported():
    assert _lib.has_members()
    for n in ("rgc_consensus_members", "rgc_pick_members", "rgc_write_members"):
        assert n in _lib.EXPORTS and hasattr(_lib.lib, n)
    assert _lib.abi_version() == 11


def _model(methods, mg):
    """The table of one micrograph: ``mg`` = (picks, left); picks = [(members, conf)] with
    members the k raw (x, y) in picker order, left[p] = raw (x, y) of picker p's leftovers."""
    k = len(methods)
    picks, left = mg

    def r(v):
        return str(int(np.rint(v)))
    rows = ["\t".join(["\t".join([r(x), r(y)]) for x, y in mem] + [str(np.float32(conf))])
            for mem, conf in picks]
    for p in range(k):
        for x, y in left[p]:
            rows.append("\t".join(["\t".join([r(x), r(y)]) if q == p else "N/A\tN/A"
                                   for q in range(k)] + [str(0.)]))
    return "\t".join(methods) + "\n" + "\n".join(rows)


def _cases(k, rng):
    """None (skipped), or (picks, left, consensus member of each pick)."""
    def pt():
        return (float(rng.choice(EDGE)) if rng.random() < 0.5 else rng.random() * 4096 - 50,
                float(rng.choice(EDGE)) if rng.random() < 0.5 else rng.random() * 4096)

    def picks(n, confs=None):
        return [([pt() for _ in range(k)],
                 np.float32(confs[i % len(confs)] if confs else rng.random()))
                for i in range(n)]

    def left(ns):
        return [[pt() for _ in range(n)] for n in ns]
    listed = [v for v, _ in LISTED]
    return [
        None,                                              # skipped: empty .box, no table
        ([], left([0] * k)),                               # ok, nothing at all: header only
        (picks(len(LISTED), listed), left([0] * k)),       # picks without leftovers
        ([], left([3] + [0] * (k - 2) + [2])),             # leftovers without picks
        (picks(40), left([(7 * p) % 5 for p in range(k)])),
        (picks(1), left([1] * k)),
        None,
    ]


def _write(tmp_path, k, n_threads):
    rng = np.random.default_rng(100 + k)
    methods = [f"picker_{chr(ord('a') + p)}" for p in range(k)]
    cases = _cases(k, rng)
    bases = [f"mg_{i}" for i in range(len(cases))]
    off, cnt, seg = [], [], []
    px, py, pc, pmx, pmy, lx, ly, loff = [], [], [], [], [], [], [], [0]
    n = 0
    cons = []
    for c in cases:
        off.append(n)
        seg.append(len(loff) - 1)
        if c is None:
            cnt.append(-1)
            cons.append(None)
            continue
        pk, lf = c
        which = [int(rng.integers(k)) for _ in pk]
        cons.append(which)
        cnt.append(len(pk))
        for (mem, conf), w in zip(pk, which):
            px.append(np.rint(mem[w][0])), py.append(np.rint(mem[w][1])), pc.append(conf)
            pmx.append([np.rint(x) for x, _ in mem]), pmy.append([np.rint(y) for _, y in mem])
        n += len(pk)
        for p in range(k):
            lx += [np.rint(x) for x, _ in lf[p]]
            ly += [np.rint(y) for _, y in lf[p]]
            loff.append(len(lx))
    out = str(tmp_path)
    _lib.write_members(out, bases, 180, off, cnt, np.array(px), np.array(py),
                       np.array(pc, np.float32), methods,
                       np.array(pmx, np.float64).reshape(-1, k),
                       np.array(pmy, np.float64).reshape(-1, k), seg, loff, np.array(lx),
                       np.array(ly), n_threads=n_threads)
    return out, methods, bases, cases, cons


@pytest.mark.parametrize("k,n_threads", [(2, 1), (8, 3)])
def test_write_members_bytes_and_round_trip(tmp_path, k, n_threads):
    out, methods, bases, cases, cons = _write(tmp_path, k, n_threads)
    files = []
    for b, c, w in zip(bases, cases, cons):
        with open(os.path.join(out, b + ".box"), "rb") as f:
            box = f.read()
        files.append(b + ".box")
        tsv = os.path.join(out, b + "_members.tsv")
        if c is None:
            assert box == b"" and not os.path.exists(tsv)
            continue
        files.append(b + "_members.tsv")
        pk, lf = c
        assert box == _reference_lines([m[i][0] for (m, _), i in zip(pk, w)],
                                       [m[i][1] for (m, _), i in zip(pk, w)],
                                       [cf for _, cf in pk], 180).encode(), b
        want = _model(methods, c)
        with open(tsv, "rb") as f:
            got = f.read()
        assert got == want.encode(), b
        assert not got.endswith(b"\n") or not (pk or any(lf))
        # row i describes .box line i; read_members gives the reference reader's shape
        coords, labels, weights = writers.read_members(tsv)
        assert labels == methods
        n_left = sum(len(v) for v in lf)
        assert len(coords) == len(weights) == len(pk) + n_left
        for i, (mem, conf) in enumerate(pk):
            assert coords[i] == [(float(np.rint(x)), float(np.rint(y))) for x, y in mem]
            assert np.float32(weights[i]) == conf or (np.isnan(conf) and np.isnan(weights[i]))
        i = len(pk)
        for p in range(k):
            for x, y in lf[p]:
                assert coords[i] == [(float(np.rint(x)), float(np.rint(y))) if q == p else ()
                                     for q in range(k)]
                assert weights[i] == 0.0
                i += 1
    assert sorted(os.listdir(out)) == sorted(files)
    # the header-only table and the listed confidences, spelled out
    with open(os.path.join(out, "mg_1_members.tsv"), "rb") as f:
        assert f.read() == ("\t".join(methods) + "\n").encode()
    with open(os.path.join(out, "mg_2_members.tsv")) as f:
        lines = f.read().split("\n")
    assert [ln.split("\t")[-1] for ln in lines[1:]] == [s for _, s in LISTED]
    assert all(len(ln.split("\t")) == 2 * k + 1 for ln in lines[1:])


def test_write_members_edge_coordinates(tmp_path):
    """-0.0, halves both ways, negatives and 1e7 in member and leftover columns."""
    methods = ["a", "b"]
    mem = [[(v, EDGE[::-1][i]), (EDGE[::-1][i], v)] for i, v in enumerate(EDGE)]
    picks = [(m, np.float32(0.5)) for m in mem]
    left = [[(v, v) for v in EDGE], [(-v, v) for v in EDGE]]
    n = len(picks)
    pmx = np.array([[np.rint(x) for x, _ in m] for m in mem])
    pmy = np.array([[np.rint(y) for _, y in m] for m in mem])
    lx = np.rint(np.array([x for p in left for x, _ in p]))
    ly = np.rint(np.array([y for p in left for _, y in p]))
    _lib.write_members(str(tmp_path), ["e"], 64, [0], [n], pmx[:, 0], pmy[:, 0],
                       np.full(n, 0.5, np.float32), methods, pmx, pmy, [0],
                       [0, len(EDGE), 2 * len(EDGE)], lx, ly)
    with open(tmp_path / "e_members.tsv", "rb") as f:
        got = f.read().decode()
    assert got == _model(methods, (picks, left))
    first = got.split("\n")[1].split("\t")
    assert first[0] == "0" and first[1] == "1234" and first[-1] == "0.5"
    assert "\t10000000\t" in got and "-37" in got and "-0" not in got.replace("-0.", "")


def test_write_members_io_error_names_the_file(tmp_path):
    z, zf = np.zeros(0), np.zeros(0, np.float32)
    a = ([0], [0], z, z, zf, ["a", "b"], np.zeros((0, 2)), np.zeros((0, 2)), [0], [0, 0, 0], z, z)
    with pytest.raises(OSError) as e:
        _lib.write_members(str(tmp_path / "missing"), ["m"], 10, *a)
    assert str(e.value.filename).endswith(os.path.join("missing", "m.box"))
    # the .box can be written, the table cannot (a directory has its name)
    os.mkdir(tmp_path / "m_members.tsv")
    with pytest.raises(OSError) as e:
        _lib.write_members(str(tmp_path), ["m"], 10, *a)
    assert str(e.value.filename).endswith("m_members.tsv")
    assert (tmp_path / "m.box").read_bytes() == b""
