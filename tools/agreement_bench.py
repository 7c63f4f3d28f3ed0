#!/usr/bin/env python3
"""File-to-file time of ``repic agreement`` next to plain ``repic consensus`` on the same inputs.

  python tools/agreement_bench.py [--config C2] [--n_mg 2000] [--repeats 3] [--workdir DIR]
                                  [--timeout S] [--no_c5] [--out FILE]

Writes a synthetic BOX directory (``synth.write_box_dirs``, not timed), then ``--repeats`` times,
interleaved, (a) plain consensus, (b) ``agreement`` and (c) ``agreement --per_box``, each into a
fresh output directory.  As tools/consensus_bench.py, this driver never opens the GPU: every
command runs in a fresh child process under its own ``timeout -k 10``, one at a time, and the
chain stops at the first non-zero exit; a run's time is the wall time of its child process.  The
tables of (b) and (c) must be byte-identical.  One more run of (b) and of (c), outside the
medians, records the device milliseconds of ``k_agree_partner`` and ``k_agree_mutual``
(RGC_F_TIMING).  For scale, one more child takes a C5-sized batch (k = 8, 64 micrographs of about
27.5k boxes) through ``Context.agreement`` and through ``Context.run``, both with RGC_F_TIMING, and
records the kernels' device milliseconds of either.  The result goes to ``--out`` (default
``profiles/agreement_f2f_<config>.json``).  Prints one JSON line.
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
TABLES = ("agreement_summary.tsv", "agreement_pairs.tsv", "agreement_matrix.tsv",
          "agreement_venn.tsv")


def _child(a):
    """One command in this (fresh) process; phases of the run go to --result as JSON."""
    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    import importlib
    t0 = time.perf_counter()
    mod = importlib.import_module(f"repic_amd.commands.{a.child}")
    t_imp = time.perf_counter() - t0
    ns = argparse.Namespace(in_dir=a.in_dir, out_dir=a.out_dir, box_size=a.box, multi_out=False,
                            get_cc=False, batch_boxes=1 << 25, threads=None, device=None,
                            listing=None, num_particles=None, node_limit=0, ji_threshold=0.3,
                            per_box=a.per_box, agreement_timing=a.agreement_timing)
    with open(os.devnull, "w") as null:
        so, sys.stdout = sys.stdout, null
        try:
            mod.main(ns)
        finally:
            sys.stdout = so
    res = {"import_s": t_imp, "main_s": time.perf_counter() - t0 - t_imp}
    res.update({k: v for k, v in mod.LAST_RUN.items() if isinstance(v, (int, float))})
    with open(a.result, "w") as f:
        json.dump(res, f)


def _child_c5(a):
    """A C5-sized batch through Context.agreement and through Context.run, kernels timed."""
    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    import numpy as np
    from repic_amd import _lib, synth
    from repic_amd.pipeline import Batch
    cfg = synth.SynthConfig(**synth.CONFIGS["C5"], seed=0)
    b = Batch.from_counts(cfg.k, cfg.box, *synth.packed(cfg, a.c5_mg))
    ctx = _lib.Context(0)
    res = {"k": cfg.k, "n_mg": b.n_mg, "boxes": b.n_boxes, "box_size": cfg.box}
    try:
        for tag, partners in (("", False), ("_per_box", True)):
            ctx.agreement(b.n_mg, cfg.k, cfg.box, b.box_off, b.x, b.y, partners=partners)  # warm
            t0 = time.perf_counter()
            r = ctx.agreement(b.n_mg, cfg.k, cfg.box, b.box_off, b.x, b.y, partners=partners,
                              timing=True)
            res["call_s" + tag] = time.perf_counter() - t0
            res["kernel_ms" + tag] = {n: round(ms, 3) for n, ms in ctx.kernel_times()}
            res["h2d_bytes" + tag], res["d2h_bytes" + tag] = ctx.agreement_bytes
        res["joined_pairs"] = int(np.triu(r.pair_edges.sum(0)).sum())
        fl = _lib.F_TIMING
        ctx.run(b.n_mg, cfg.k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score, fl)   # warm
        t0 = time.perf_counter()
        rr = ctx.run(b.n_mg, cfg.k, cfg.box, b.box_off, b.id_base, b.x, b.y, b.score, fl)
        res["run_call_s"] = time.perf_counter() - t0
        times = {}
        for n, ms in ctx.kernel_times():
            times[n] = round(times.get(n, 0.0) + ms, 3)
        res["run_kernel_ms"] = times
        res["run_kernel_ms_total"] = round(sum(times.values()), 3)
        res["run_edges"] = int(rr.n_edges)
    finally:
        ctx.close()
    with open(a.result, "w") as f:
        json.dump(res, f)


def _run_child(cmd, in_dir, out_dir, box, limit, work, extra=()):
    """-> (wall seconds, the child's result dict); raises on a non-zero exit."""
    result = os.path.join(work, f"res_{cmd}.json")
    if os.path.exists(result):
        os.remove(result)
    argv = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
            "--child", cmd, "--in_dir", str(in_dir), "--out_dir", str(out_dir), "--box", str(box),
            "--result", result, *extra]
    t0 = time.perf_counter()
    r = subprocess.run(argv, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit(f"agreement_bench: `{cmd}` exited {r.returncode} after {wall:.1f} s; "
                         f"stopping\n{r.stderr[-2000:]}")
    with open(result) as f:
        return wall, json.load(f)


def _tables(d):
    out = {}
    for n in TABLES:
        with open(os.path.join(d, n), "rb") as f:
            out[n] = f.read()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", help="synth.CONFIGS name (C2, C4, ...)")
    ap.add_argument("--n_mg", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--no_c5", action="store_true", help="leave the C5-sized batch out")
    ap.add_argument("--c5_mg", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    for n in ("--in_dir", "--out_dir", "--result"):
        ap.add_argument(n, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--box", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--per_box", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--agreement_timing", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child == "c5":
        return _child_c5(a)
    if a.child:
        return _child(a)

    sys.path.insert(0, os.path.join(ROOT, "repic-copy_amd"))
    from repic_amd import synth
    cfg = synth.SynthConfig(**synth.CONFIGS[a.config], seed=0)
    work = tempfile.mkdtemp(prefix="rgc_agree_", dir=a.workdir)
    out = {"metric": "file-to-file seconds, BOX directories -> report tables (1 GPU)",
           "config": a.config, "n_mg": a.n_mg, "k": cfg.k, "repeats": a.repeats,
           "baseline": "plain consensus, this checkout, same session"}
    arms = (("consensus", "consensus", ()), ("agreement", "agreement", ()),
            ("agreement_per_box", "agreement", ("--per_box",)))
    try:
        in_dir = os.path.join(work, "in")
        synth.write_box_dirs(in_dir, cfg, a.n_mg)
        secs = {n: [] for n, _, _ in arms}
        last = {}
        for i in range(a.repeats):
            tabs = {}
            for n, cmd, extra in arms:
                d = os.path.join(work, f"{n}_{i}")
                w, ph = _run_child(cmd, in_dir, d, cfg.box, a.timeout, work, extra)
                secs[n].append(w)
                last[n] = ph
                if cmd == "agreement":
                    tabs[n] = _tables(d)
                out["files_" + n] = len(os.listdir(d))
                shutil.rmtree(d)
            assert tabs["agreement"] == tabs["agreement_per_box"], "--per_box changed a table"
        for n, _, extra in arms[1:]:
            d = os.path.join(work, "timed_" + n)
            _, ph = _run_child("agreement", in_dir, d, cfg.box, a.timeout, work,
                               extra + ("--agreement_timing",))
            shutil.rmtree(d)
            out[n + "_kernel_ms"] = {k_[:-3]: round(v, 3) for k_, v in ph.items()
                                     if k_.endswith("_ms")}
        for n, _, _ in arms:
            out[n + "_s"] = secs[n]
            out[n + "_median_s"] = statistics.median(secs[n])
            out[n + "_range_s"] = [min(secs[n]), max(secs[n])]
            for key in ("import_s", "index_s", "parse_s", "device_s", "write_s", "h2d_bytes",
                        "d2h_bytes"):
                out[f"{n}_{key}"] = last[n].get(key)
        for key in ("micrographs", "boxes", "edges"):
            out[key] = last["agreement"].get(key)
        out["consensus_edges"] = last["consensus"].get("edges")
        if not a.no_c5:
            _, out["c5_batch"] = _run_child("c5", in_dir, os.path.join(work, "unused"), cfg.box,
                                            a.timeout, work, ("--c5_mg", str(a.c5_mg)))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    path = a.out or os.path.join(ROOT, "profiles", f"agreement_f2f_{a.config}.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
