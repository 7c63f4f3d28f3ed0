"""Shared by the score sweep tests: the goldens of tests/golden/make_score_sweep_golden.py and
the comparison of score tuples (types and bit patterns, NaN equal to NaN)."""
import json
import os
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "score_sweep")


def cases():
    """-> (case, gt (n, 5), picks (n, 5), thresholds) of every golden case."""
    meta = json.load(open(os.path.join(GOLD, "meta.json")))
    arr = np.load(os.path.join(GOLD, "cases.npz"))
    for c in meta["cases"]:
        yield (c, arr[c["name"] + "_gt"], arr[c["name"] + "_pk"],
               [float.fromhex(h) for h in c["thresh_hex"]])


def recs(a):
    return [tuple(r) for r in a.tolist()]


def same_as_golden(got, case, j):
    want = [float.fromhex(h) for h in case["result_hex"][j]]
    for g, w, t in zip(got, want, case["result_type"][j]):
        assert type(g).__name__ == t, (case["name"], j, type(g), t)
        assert (np.isnan(g) and np.isnan(w)) or float(g).hex() == w.hex(), (case["name"], j, g, w)


def same_scores(got, want, what=""):
    assert len(got) == len(want) == 4
    for a, b in zip(got, want):
        assert type(a) is type(b), (what, type(a), type(b))
        assert (np.isnan(a) and np.isnan(b)) or float(a).hex() == float(b).hex(), (what, a, b)


def oracle_scores(g, p, t, **kw):
    from oracle import score_ref
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return score_ref.get_segmentation_scores(recs(g), recs(p), t, **kw)
