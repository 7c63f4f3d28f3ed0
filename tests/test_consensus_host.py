"""Host side of ``repic consensus`` (ABI 10), CPU only.

* rgc_np_float_str prints exactly what str(numpy.float32(v)) prints (the confidence column of
  the final .box files; not CPython's float repr)
* rgc_write_boxes writes byte for byte the lines reference run_ilp.py:126-131 builds
* the dispatcher knows the subcommand, its parser takes the documented arguments and has no
  --multi_out
* with WORLD_SIZE > 1 the command raises before it creates a device context or touches out_dir
"""
import argparse
import os

import numpy as np
import pytest

from repic_amd import _lib
from repic_amd.commands import consensus
from repic_amd.main import main as cli_main

LISTED = [(1e-4, "1e-04"), (1e-5, "1e-05"), (9.9999e-5, "9.9999e-05"),
          (0.12345679, "0.12345679"), (1e16, "1e+16"), (3.4e38, "3.4e+38"), (-0.0, "-0.0"),
          (1.0, "1.0")]


def test_np_float_str_listed_values():
    for v, want in LISTED:
        assert str(np.float32(v)) == want          # what this numpy prints
        assert _lib.np_float_str(np.float32(v)) == want


def test_np_float_str_special_values():
    fi = np.finfo(np.float32)
    vals = [0.0, -0.0, fi.tiny, -fi.tiny, fi.smallest_subnormal, fi.tiny / 8, fi.max, -fi.max,
            0.1, 0.3, 1 / 3, 1e15, 1e16, 9.999999e15, 1e-4, 1.0001e-4, 123456.0, 1e7, 16777216.0]
    for v in np.array(vals, np.float32):
        assert _lib.np_float_str(v) == str(v), repr(v)


def test_np_float_str_random_bit_patterns():
    rng = np.random.default_rng(11)
    v = rng.integers(0, 2 ** 32, 30000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    v = v[np.isfinite(v)][:20000]
    assert len(v) == 20000
    bad = [(x, _lib.np_float_str(x), str(x)) for x in v if _lib.np_float_str(x) != str(x)]
    assert not bad, bad[:5]


def test_np_float_str_uniform_unit_interval():
    rng = np.random.default_rng(12)
    v = rng.random(20000).astype(np.float32)
    v = v[v > 0]
    bad = [(x, _lib.np_float_str(x), str(x)) for x in v if _lib.np_float_str(x) != str(x)]
    assert not bad, bad[:5]


def _reference_lines(px, py, conf, box_size):
    """run_ilp.py:126-131 for picks already in output order."""
    bs = str(box_size)
    return "".join("\t".join([str(int(np.rint(a))), str(int(np.rint(b))), bs, bs, str(w)]) + "\n"
                   for a, b, w in zip(px, py, conf))


def test_write_boxes_bytes(tmp_path):
    rng = np.random.default_rng(3)
    # raw coordinates as run_ilp sees them; the library gets np.rint of them (k_pick_emit)
    edge = np.array([-0.0, 0.5, 1.5, 2.5, -1.5, 1e7])
    segs = [
        None,                                                   # skipped micrograph
        (np.array([1234.5]), np.array([77.0]), np.array([0.5], np.float32)),
        (edge, edge[::-1].copy(), np.array([1.0, 1e-4, 1e-5, -0.0, 0.12345679, 3.4e38],
                                            np.float32)),
        (rng.random(40) * 4096 - 100, rng.random(40) * 4096,
         rng.random(40).astype(np.float32)),
        (np.zeros(0), np.zeros(0), np.zeros(0, np.float32)),    # ok micrograph, nothing kept
    ]
    bases = [f"mg_{i}" for i in range(len(segs))]
    off, cnt, px, py, pc = [], [], [], [], []
    n = 0
    for s in segs:
        off.append(n)
        if s is None:
            cnt.append(-1)
            continue
        cnt.append(len(s[0]))
        px.append(np.rint(s[0])), py.append(np.rint(s[1])), pc.append(s[2])
        n += len(s[0])
    out = str(tmp_path)
    _lib.write_boxes(out, bases, 180, off, cnt, np.concatenate(px), np.concatenate(py),
                     np.concatenate(pc), n_threads=3)
    for b, s in zip(bases, segs):
        with open(os.path.join(out, b + ".box"), "rb") as f:
            got = f.read()
        want = "" if s is None else _reference_lines(s[0], s[1], s[2], 180)
        assert got == want.encode(), b
    assert sorted(os.listdir(out)) == sorted(b + ".box" for b in bases)
    with open(os.path.join(out, "mg_2.box")) as f:
        first = f.readline().split("\t")
    assert first[0] == "0" and first[1] == "10000000" and first[2:4] == ["180", "180"]


def test_write_boxes_reports_io_error(tmp_path):
    with pytest.raises(OSError) as e:
        _lib.write_boxes(str(tmp_path / "missing"), ["a"], 10, [0], [0], np.zeros(0),
                         np.zeros(0), np.zeros(0, np.float32))
    assert "a.box" in str(e.value.filename)


def test_dispatcher_and_parser(capsys):
    with pytest.raises(SystemExit) as e:
        cli_main(["consensus", "-h"])
    assert e.value.code == 0
    assert "--num_particles" in capsys.readouterr().out
    p = argparse.ArgumentParser()
    consensus.add_arguments(p)
    a = p.parse_args(["in", "out", "180", "--num_particles", "7", "--get_cc", "--node_limit",
                      "99", "--batch_boxes", "1000", "--threads", "2", "--device", "0"])
    assert (a.in_dir, a.out_dir, a.box_size) == ("in", "out", 180)
    assert (a.num_particles, a.get_cc, a.node_limit) == (7, True, 99)
    assert (a.batch_boxes, a.threads, a.device) == (1000, 2, 0)
    d = p.parse_args(["in", "out", "180"])
    assert d.num_particles is None and d.get_cc is False and d.listing is None
    with pytest.raises(SystemExit) as e:
        p.parse_args(["in", "out", "180", "--multi_out"])
    assert e.value.code != 0
    assert consensus.name == "consensus"


def test_world_size_rejected_before_any_side_effect(tmp_path, monkeypatch):
    in_dir, out_dir = tmp_path / "in", tmp_path / "out"
    (in_dir / "a").mkdir(parents=True)
    out_dir.mkdir()
    sentinel = out_dir / "keep.txt"
    sentinel.write_text("x")
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")

    def no_ctx(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", no_ctx)
    args = argparse.Namespace(in_dir=str(in_dir), out_dir=str(out_dir), box_size=180,
                              num_particles=None, get_cc=False, node_limit=0,
                              batch_boxes=1 << 25, threads=None, device=None, listing=None)
    with pytest.raises(_lib.RGCError, match="WORLD_SIZE"):
        consensus.main(args)
    assert sentinel.read_text() == "x"
