#!/usr/bin/env python3
"""Golden fixtures of the REAL reference ``get_cliques`` at other Jaccard thresholds.

The reference passes its threshold to ``get_jaccard(set_a, set_b, box_size, threshold)`` and
fixes it at 0.3 at the one call site.  This generator runs ``repic.commands.get_cliques.main``
in a fresh process (as ``make_golden.py`` does) with ``gc.get_jaccard`` wrapped at run time so
that the threshold it receives is ``t``; the wrapper below is this project's code, nothing of
the reference is copied.  Like ``make_golden.py`` it touches the reference checkout only at
fixture-generation time.

Each (case, t) of ``THRESHOLD_CASES`` reuses the inputs of ``cases.CASES[case]`` and is stored
as ``thr_<case>_<t>/{meta.json,data.npz}`` in ``make_golden.py``'s canonical form, with two more
keys in the meta: ``base_case`` and ``ji_threshold``.  The directory names are not in
``cases.CASES``, so the parametrised tests over ``golden_cases()`` do not pick them up.

Usage:  python tests/golden/make_golden_threshold.py [thr_<case>_<t> ...]
"""
from __future__ import annotations

import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from cases import CASES, materialise  # noqa: E402
from make_golden import REFERENCE, collect, tree_digest  # noqa: E402

THRESHOLD_CASES = [("syn_k3", 0.2), ("syn_k3", 0.5), ("syn_k3_frac", 0.05), ("syn_k5", 0.45),
                   ("ties", 0.0), ("tiny_k4", 0.15)]


def thr_name(case, t):
    return f"thr_{case}_{t}"


DRIVER = (
    "import sys, argparse\n"
    f"sys.path.insert(0, {REFERENCE!r})\n"
    "import repic.commands.get_cliques as gc\n"
    "T = float(sys.argv[1])\n"
    "_get_jaccard = gc.get_jaccard\n"
    "def _at_t(set_a, set_b, box_size, threshold):\n"
    "    return _get_jaccard(set_a, set_b, box_size, T)\n"
    "gc.get_jaccard = _at_t\n"
    "p = argparse.ArgumentParser(); gc.add_arguments(p)\n"
    "gc.main(p.parse_args(sys.argv[2:]))\n"
)


def run_reference(in_dir, out_dir, box, flags, t):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", MPLBACKEND="Agg")
    cmd = [sys.executable, "-c", DRIVER, repr(float(t)), in_dir, out_dir, str(box)] + list(flags)
    r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True)
    order = [ln.strip()[4:-4] for ln in r.stdout.splitlines()
             if ln.startswith("--- ") and ln.rstrip().endswith(" ---")]
    exc = None
    if r.returncode != 0:
        last = [ln for ln in r.stderr.strip().splitlines() if ln.strip()][-1]
        exc = last.split(":")[0].strip()
    return order, exc, r


def make_case(base, t):
    case = CASES[base]
    name = thr_name(base, t)
    tmp = tempfile.mkdtemp(prefix="golden_thr_")
    try:
        in_dir, out_dir = os.path.join(tmp, "in"), os.path.join(tmp, "out")
        materialise(case, in_dir)
        digest = tree_digest(in_dir)
        methods = sorted([d for d in os.listdir(in_dir) if os.path.isdir(os.path.join(in_dir, d))],
                         key=str)
        listing = {m: os.listdir(os.path.join(in_dir, m)) for m in methods}
        order, exc, r = run_reference(in_dir, out_dir, case["box"], case.get("flags", ()), t)
        mgs, arrays = collect(case, out_dir, order, exc, methods)
        meta = {"case": name, "base_case": base, "ji_threshold": float(t), "box": case["box"],
                "flags": list(case.get("flags", ())), "methods": methods, "listing": listing,
                "order": order, "exception": exc, "input_sha256": digest, "micrographs": mgs}
        d = os.path.join(HERE, name)
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "meta.json"), "w") as f:
            json.dump(meta, f, indent=1)
        np.savez_compressed(os.path.join(d, "data.npz"), **arrays)
        print(f"{name}: rc={r.returncode}, {len(order)} micrographs "
              f"({sum(m['status'] == 'ok' for m in mgs)} ok), exception={exc}, "
              f"cliques={sum(m.get('C', 0) for m in mgs)}", flush=True)
        if exc is None and r.returncode != 0:
            print(r.stderr[-2000:])
    finally:
        shutil.rmtree(tmp)


def main(argv):
    for base, t in THRESHOLD_CASES:
        if not argv or thr_name(base, t) in argv:
            make_case(base, t)


if __name__ == "__main__":
    main(sys.argv[1:])
