#!/usr/bin/env python3
"""File-to-file time of ``repic consensus`` against the two-step path it replaces
(``repic get_cliques`` then ``repic run_ilp``): BOX directories in, final ``.box`` files out.

  python tools/consensus_bench.py [--config C2] [--n_mg 2000] [--repeats 3]
                                  [--baseline-root DIR] [--workdir DIR] [--timeout S]

Writes a synthetic BOX directory (``synth.write_box_dirs``, not timed), then ``--repeats``
times, interleaved, (a) get_cliques + run_ilp and (b) consensus, each into a fresh output
directory.  This driver never opens the GPU: every command runs in a fresh child process under
its own ``timeout -k 10``, one at a time, and the chain stops at the first non-zero exit.
A run's time is the wall time of its child processes (interpreter start and imports included:
what a user of the CLI waits for).  The ``.box`` files of (a) and (b) must be byte-identical.
``--baseline-root`` runs (a) from another checkout (e.g. the parent commit, built there).
``--members`` measures ``consensus --members`` instead: per repeat, interleaved, (a) plain
consensus from ``--baseline-root`` (the parent commit, built there; this checkout without it),
(b) plain consensus from this checkout and (c) ``consensus --members`` from this checkout; the
``.box`` files of all three must be byte-identical.
``--dedup_ji T`` measures ``consensus --dedup_ji T`` instead: per repeat, interleaved, (a) plain
consensus and (b) ``consensus --dedup_ji T``, both from this checkout; every ``.box`` of (b) must
be a subsequence of (a)'s lines and the lines missing must add up to the run's ``suppressed``.
One more run of (b), outside the medians, records the device milliseconds of ``k_nms_count`` and
``k_nms`` (RGC_F_TIMING).  The result also goes to ``--out`` (default
``profiles/consensus_dedup_f2f_<config>.json``).
``--min_pickers M`` measures ``consensus --min_pickers M`` instead: per repeat, interleaved, (a)
plain consensus with the library ``--baseline-lib`` names (the parent commit's build; without it
this checkout's), (b) plain consensus and (c) ``consensus --min_pickers M`` from this checkout.
The ``.box`` files of (a) and (b) must be byte-identical and every ``.box`` of (c) must start with
(b)'s bytes.  One more run of (c), outside the medians, records the per-kernel device
milliseconds (RGC_F_TIMING).  The result also goes to ``--out`` (default
``profiles/consensus_tiers_f2f_<config>.json``).
Prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(a):
    """One command in this (fresh) process; phases of the run go to --result as JSON."""
    sys.path.insert(0, os.path.join(a.root, "repic-copy_amd"))
    import importlib
    t0 = time.perf_counter()
    mod = importlib.import_module(f"repic_amd.commands.{a.child}")
    t_imp = time.perf_counter() - t0
    if a.child == "run_ilp":
        ns = argparse.Namespace(in_dir=a.out_dir, box_size=a.box, num_particles=None,
                                node_limit=0, device=None)
    else:
        ns = argparse.Namespace(in_dir=a.in_dir, out_dir=a.out_dir, box_size=a.box,
                                multi_out=False, get_cc=False, batch_boxes=1 << 25, threads=None,
                                device=None, listing=None, num_particles=None, node_limit=0)
        if a.with_members:
            ns.members = True
        if a.with_dedup is not None:
            ns.dedup_ji = a.with_dedup
            ns.dedup_timing = a.dedup_timing
        if a.with_min_pickers is not None:
            ns.min_pickers = a.with_min_pickers
            ns.tiers_timing = a.tiers_timing
    with open(os.devnull, "w") as null:
        so, sys.stdout = sys.stdout, null     # the per-micrograph banner lines
        try:
            mod.main(ns)
        finally:
            sys.stdout = so
    res = {"import_s": t_imp, "main_s": time.perf_counter() - t0 - t_imp}
    last = getattr(mod, "LAST_RUN", None)
    if last:
        res.update({k: v for k, v in last.items() if isinstance(v, (int, float))})
    with open(a.result, "w") as f:
        json.dump(res, f)


def _run_child(cmd, root, in_dir, out_dir, box, limit, work, members=False, dedup=None,
               dedup_timing=False, min_pickers=None, tiers_timing=False, lib=None):
    """-> (wall seconds, the child's phase dict); raises on a non-zero exit."""
    result = os.path.join(work, f"res_{cmd}.json")
    if os.path.exists(result):
        os.remove(result)
    argv = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
            "--child", cmd, "--root", root, "--in_dir", in_dir, "--out_dir", out_dir,
            "--box", str(box), "--result", result] + (["--with_members"] if members else [])
    if dedup is not None:
        argv += ["--with_dedup", repr(float(dedup))] + (["--dedup_timing"] if dedup_timing else [])
    if min_pickers is not None:
        argv += ["--with_min_pickers", str(min_pickers)] + (["--tiers_timing"] if tiers_timing else [])
    env = dict(os.environ, REPIC_GC_LIB=os.path.abspath(lib)) if lib else None
    t0 = time.perf_counter()
    r = subprocess.run(argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=env)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"consensus_bench: `{cmd}` from {root} exited {r.returncode} after "
                         f"{wall:.1f} s; stopping\n{r.stderr[-2000:]}")
    with open(result) as f:
        return wall, json.load(f)


def _boxes(d):
    out = {}
    for e in os.scandir(d):
        if e.name.endswith(".box"):
            with open(e.path, "rb") as f:
                out[e.name] = f.read()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", help="synth.CONFIGS name (C2, C4, ...)")
    ap.add_argument("--n_mg", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-root", default=None,
                    help="checkout whose get_cliques / run_ilp are the two-step path")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    for n in ("--root", "--in_dir", "--out_dir", "--result"):
        ap.add_argument(n, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--box", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--with_members", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--members", action="store_true",
                    help="time consensus --members against plain consensus (see above)")
    ap.add_argument("--with_dedup", type=float, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dedup_timing", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dedup_ji", type=float, default=None, metavar="T",
                    help="time consensus --dedup_ji T against plain consensus (see above)")
    ap.add_argument("--with_min_pickers", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--tiers_timing", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--min_pickers", type=int, default=None, metavar="M",
                    help="time consensus --min_pickers M against plain consensus (see above)")
    ap.add_argument("--baseline-lib", default=None,
                    help="--min_pickers: librepic_gc.so of the baseline arm (the parent commit's)")
    ap.add_argument("--out", default=None,
                    help="--dedup_ji / --min_pickers: also write the JSON result here")
    a = ap.parse_args()
    if a.child:
        return _child(a)
    if a.members:
        return _members(a)
    if a.dedup_ji is not None:
        return _dedup(a)
    if a.min_pickers is not None:
        return _tiers(a)

    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    from repic_amd import synth
    cfg = synth.SynthConfig(**synth.CONFIGS[a.config], seed=0)
    base_root = os.path.abspath(a.baseline_root) if a.baseline_root else ROOT
    work = tempfile.mkdtemp(prefix="rgc_cons_", dir=a.workdir)
    out = {"metric": "file-to-file seconds, BOX directories -> final .box files (1 GPU)",
           "config": a.config, "n_mg": a.n_mg, "k": cfg.k, "repeats": a.repeats,
           "baseline": "other checkout" if a.baseline_root else "this checkout"}
    try:
        in_dir = os.path.join(work, "in")
        synth.write_box_dirs(in_dir, cfg, a.n_mg)
        two, one, ph_gc, ph_ilp, ph_c = [], [], [], [], []
        for i in range(a.repeats):
            d2, d1 = os.path.join(work, f"two_{i}"), os.path.join(work, f"one_{i}")
            t_gc, p_gc = _run_child("get_cliques", base_root, in_dir, d2, cfg.box, a.timeout, work)
            t_il, p_il = _run_child("run_ilp", base_root, in_dir, d2, cfg.box, a.timeout, work)
            t_c, p_c = _run_child("consensus", ROOT, in_dir, d1, cfg.box, a.timeout, work)
            two.append(t_gc + t_il)
            one.append(t_c)
            ph_gc.append(dict(p_gc, wall_s=t_gc))
            ph_ilp.append(dict(p_il, wall_s=t_il))
            ph_c.append(dict(p_c, wall_s=t_c))
            want, got = _boxes(d2), _boxes(d1)
            assert sorted(want) == sorted(got), "consensus wrote another set of .box files"
            bad = [n for n in want if want[n] != got[n]]
            assert not bad, f".box files differ: {bad[:5]}"
            out["files_two_step"] = len(os.listdir(d2))
            out["files_consensus"] = len(os.listdir(d1))
            out["box_files"] = len(want)
            shutil.rmtree(d2)
            shutil.rmtree(d1)
        out["box_files_identical"] = True

        def med(rows, key):
            v = [r[key] for r in rows if key in r]
            return statistics.median(v) if v else None
        out["two_step_s"] = two
        out["consensus_s"] = one
        out["two_step_median_s"] = statistics.median(two)
        out["consensus_median_s"] = statistics.median(one)
        out["speedup_median"] = out["two_step_median_s"] / out["consensus_median_s"]
        out["slowest_consensus_faster_than_fastest_two_step"] = max(one) < min(two)
        keys = ("wall_s", "import_s", "main_s", "index_s", "parse_s", "device_s", "write_s",
                "write_tail_s")
        out["phases_get_cliques"] = {k: med(ph_gc, k) for k in keys if med(ph_gc, k) is not None}
        out["phases_run_ilp"] = {k: med(ph_ilp, k) for k in keys if med(ph_ilp, k) is not None}
        out["phases_consensus"] = {k: med(ph_c, k) for k in keys if med(ph_c, k) is not None}
        c = ph_c[-1]
        out["cliques"], out["picks"] = c.get("cliques"), c.get("picks")
        out["h2d_bytes"], out["d2h_bytes"] = c.get("h2d_bytes"), c.get("d2h_bytes")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out))


def _members(a):
    """--members: baseline consensus | consensus | consensus --members, interleaved."""
    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    from repic_amd import synth
    cfg = synth.SynthConfig(**synth.CONFIGS[a.config], seed=0)
    base_root = os.path.abspath(a.baseline_root) if a.baseline_root else ROOT
    work = tempfile.mkdtemp(prefix="rgc_cons_", dir=a.workdir)
    out = {"metric": "file-to-file seconds, BOX directories -> final .box files (1 GPU)",
           "config": a.config, "n_mg": a.n_mg, "k": cfg.k, "repeats": a.repeats,
           "baseline": "other checkout" if a.baseline_root else "this checkout"}
    arms = (("baseline_consensus", base_root, False), ("consensus", ROOT, False),
            ("consensus_members", ROOT, True))
    try:
        in_dir = os.path.join(work, "in")
        synth.write_box_dirs(in_dir, cfg, a.n_mg)
        secs = {n: [] for n, _, _ in arms}
        last = {}
        for i in range(a.repeats):
            want = None
            for n, root, mem in arms:
                d = os.path.join(work, f"{n}_{i}")
                t, ph = _run_child("consensus", root, in_dir, d, cfg.box, a.timeout, work, mem)
                secs[n].append(t)
                last[n] = ph
                got = _boxes(d)
                assert want is None or got == want, f"{n}: .box files differ from the baseline's"
                want = got
                out["files_" + n] = len(os.listdir(d))
                shutil.rmtree(d)
        out["box_files"] = len(want)
        out["box_files_identical"] = True
        for n, _, _ in arms:
            out[n + "_s"] = secs[n]
            out[n + "_median_s"] = statistics.median(secs[n])
            out[n + "_range_s"] = [min(secs[n]), max(secs[n])]
            out[n + "_h2d_bytes"] = last[n].get("h2d_bytes")
            out[n + "_d2h_bytes"] = last[n].get("d2h_bytes")
            out[n + "_device_s"] = last[n].get("device_s")
            out[n + "_write_s"] = last[n].get("write_s")
        lo, hi = out["baseline_consensus_range_s"]
        out["plain_median_inside_baseline_range"] = lo <= out["consensus_median_s"] <= hi
        out["cliques"], out["picks"] = last["consensus"].get("cliques"), last["consensus"].get("picks")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out))


def _is_subsequence(short, full):
    it = iter(full)
    return all(any(ln == x for x in it) for ln in short)


def _dedup(a):
    """--dedup_ji T: consensus | consensus --dedup_ji T, interleaved, then one timed run."""
    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    from repic_amd import synth
    cfg = synth.SynthConfig(**synth.CONFIGS[a.config], seed=0)
    work = tempfile.mkdtemp(prefix="rgc_cons_", dir=a.workdir)
    out = {"metric": "file-to-file seconds, BOX directories -> final .box files (1 GPU)",
           "config": a.config, "n_mg": a.n_mg, "k": cfg.k, "repeats": a.repeats,
           "dedup_ji": a.dedup_ji, "baseline": "plain consensus, this checkout"}
    arms = (("consensus", None), ("consensus_dedup", a.dedup_ji))
    try:
        in_dir = os.path.join(work, "in")
        synth.write_box_dirs(in_dir, cfg, a.n_mg)
        secs = {n: [] for n, _ in arms}
        last = {}
        for i in range(a.repeats):
            boxes = {}
            for n, t in arms:
                d = os.path.join(work, f"{n}_{i}")
                w, ph = _run_child("consensus", ROOT, in_dir, d, cfg.box, a.timeout, work,
                                   dedup=t)
                secs[n].append(w)
                last[n] = ph
                boxes[n] = _boxes(d)
                out["files_" + n] = len(os.listdir(d))
                shutil.rmtree(d)
            plain, ded = boxes["consensus"], boxes["consensus_dedup"]
            assert sorted(plain) == sorted(ded), "--dedup_ji wrote another set of .box files"
            gone = 0
            for f in plain:
                pl, dl = plain[f].splitlines(), ded[f].splitlines()
                assert _is_subsequence(dl, pl), f"{f}: not a subsequence of the plain file"
                gone += len(pl) - len(dl)
            assert gone == last["consensus_dedup"].get("suppressed"), "suppressed != lines missing"
        d = os.path.join(work, "timed")
        _, ph = _run_child("consensus", ROOT, in_dir, d, cfg.box, a.timeout, work,
                           dedup=a.dedup_ji, dedup_timing=True)
        shutil.rmtree(d)
        out["box_files"] = len(plain)
        for n, _ in arms:
            out[n + "_s"] = secs[n]
            out[n + "_median_s"] = statistics.median(secs[n])
            out[n + "_range_s"] = [min(secs[n]), max(secs[n])]
            out[n + "_h2d_bytes"] = last[n].get("h2d_bytes")
            out[n + "_d2h_bytes"] = last[n].get("d2h_bytes")
            out[n + "_device_s"] = last[n].get("device_s")
            out[n + "_write_s"] = last[n].get("write_s")
        dd = last["consensus_dedup"]
        out["added_median_s"] = out["consensus_dedup_median_s"] - out["consensus_median_s"]
        out["added_h2d_bytes"] = dd.get("dedup_h2d_bytes")
        out["added_d2h_bytes"] = dd.get("dedup_d2h_bytes")
        out["dedup_s"] = dd.get("dedup_s")
        out["picks_plain"] = last["consensus"].get("picks")
        out["picks_written"] = dd.get("picks")
        out["suppressed"] = dd.get("suppressed")
        out["k_nms_count_ms"] = ph.get("k_nms_count_ms")
        out["k_nms_ms"] = ph.get("k_nms_ms")
        out["cliques"] = dd.get("cliques")
    finally:
        shutil.rmtree(work, ignore_errors=True)
    path = a.out or os.path.join(ROOT, "profiles", f"consensus_dedup_f2f_{a.config}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def _tiers(a):
    """--min_pickers M: baseline-library consensus | consensus | consensus --min_pickers M,
    interleaved, then one timed run of the last."""
    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    from repic_amd import synth
    cfg = synth.SynthConfig(**synth.CONFIGS[a.config], seed=0)
    work = tempfile.mkdtemp(prefix="rgc_cons_", dir=a.workdir)
    out = {"metric": "file-to-file seconds, BOX directories -> final .box files (1 GPU)",
           "config": a.config, "n_mg": a.n_mg, "k": cfg.k, "repeats": a.repeats,
           "min_pickers": a.min_pickers,
           "baseline": "plain consensus, " + ("the baseline library" if a.baseline_lib
                                              else "this checkout")}
    arms = (("baseline_consensus", {"lib": a.baseline_lib}), ("consensus", {}),
            ("consensus_tiers", {"min_pickers": a.min_pickers}))
    try:
        in_dir = os.path.join(work, "in")
        synth.write_box_dirs(in_dir, cfg, a.n_mg)
        secs = {n: [] for n, _ in arms}
        last = {}
        for i in range(a.repeats):
            boxes = {}
            for n, kw in arms:
                d = os.path.join(work, f"{n}_{i}")
                w, ph = _run_child("consensus", ROOT, in_dir, d, cfg.box, a.timeout, work, **kw)
                secs[n].append(w)
                last[n] = ph
                boxes[n] = _boxes(d)
                out["files_" + n] = len(os.listdir(d))
                shutil.rmtree(d)
            assert boxes["consensus"] == boxes["baseline_consensus"], ".box files differ from the baseline's"
            plain, tiers = boxes["consensus"], boxes["consensus_tiers"]
            assert sorted(plain) == sorted(tiers), "--min_pickers wrote another set of .box files"
            bad = [f for f in plain if not tiers[f].startswith(plain[f])]
            assert not bad, f".box files do not start with the plain file's bytes: {bad[:5]}"
        d = os.path.join(work, "timed")
        _, ph = _run_child("consensus", ROOT, in_dir, d, cfg.box, a.timeout, work,
                           min_pickers=a.min_pickers, tiers_timing=True)
        shutil.rmtree(d)
        out["box_files"] = len(plain)
        for n, _ in arms:
            out[n + "_s"] = secs[n]
            out[n + "_median_s"] = statistics.median(secs[n])
            out[n + "_range_s"] = [min(secs[n]), max(secs[n])]
            for key in ("h2d_bytes", "d2h_bytes", "device_s", "write_s", "cliques", "picks"):
                out[f"{n}_{key}"] = last[n].get(key)
        lo, hi = out["baseline_consensus_range_s"]
        out["plain_median_inside_baseline_range"] = lo <= out["consensus_median_s"] <= hi
        out["plain_bytes_identical_to_baseline"] = (
            out["consensus_h2d_bytes"] == out["baseline_consensus_h2d_bytes"]
            and out["consensus_d2h_bytes"] == out["baseline_consensus_d2h_bytes"])
        out["added_median_s"] = out["consensus_tiers_median_s"] - out["consensus_median_s"]
        tl = last["consensus_tiers"]
        out["picks_per_tier"] = {k_[len("picks_tier_"):]: v for k_, v in sorted(tl.items())
                                 if k_.startswith("picks_tier_")}
        out["kernel_ms"] = {k_[:-3]: round(v, 3) for k_, v in ph.items() if k_.endswith("_ms")}
    finally:
        shutil.rmtree(work, ignore_errors=True)
    path = a.out or os.path.join(ROOT, "profiles", f"consensus_tiers_f2f_{a.config}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
