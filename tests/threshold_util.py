"""Shared by the Jaccard-threshold tests (test_ji_threshold_host.py, test_gpu_ji_threshold.py):
the ``thr_*`` goldens recorded from the reference at other thresholds
(tests/golden/make_golden_threshold.py) and the threshold's geometry."""
from __future__ import annotations

import json
import os

import numpy as np

from golden_util import CASES, GOLDEN, materialise, tree_digest
from make_golden_threshold import THRESHOLD_CASES, thr_name

THR = [thr_name(c, t) for c, t in THRESHOLD_CASES]


def load_thr(name):
    d = os.path.join(GOLDEN, name)
    with open(os.path.join(d, "meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(d, "data.npz"), allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    return meta, data


def make_thr_inputs(meta, root):
    in_dir = os.path.join(root, "in")
    materialise(CASES[meta["base_case"]], in_dir)
    assert tree_digest(in_dir) == meta["input_sha256"], "fixture inputs not reproduced"
    return in_dir


def patch_oracles(monkeypatch, t):
    """The CPU oracles read their module-level THRESHOLD at call time."""
    from oracle import cpu_ref, cpu_vec
    monkeypatch.setattr(cpu_ref, "THRESHOLD", t)
    monkeypatch.setattr(cpu_vec, "THRESHOLD", t)


def rho(t):
    """JI > t needs |dx|, |dy| < rho(t) B."""
    return (1.0 - t) / (1.0 + t)


def c_of(t):
    """JI > t <=> I > c(t) B^2 in exact arithmetic."""
    return 2.0 * t / (1.0 + t)


def ref_q(I, B):
    """The reference quotient on an overlap area I (f64, get_cliques.py:45-46)."""
    I = np.asarray(I, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return I / (np.float64(2 * B * B) - I)


def ref_ji(x, y, a, b, B):
    """calc_jaccard's f64 op order (oracle/cpu_ref.jaccard, vectorised)."""
    xo = np.maximum((np.minimum(x, a) + B) - np.maximum(x, a), 0.0)
    yo = np.maximum((np.minimum(y, b) + B) - np.maximum(y, b), 0.0)
    return ref_q(xo * yo, B)
