"""Host parts of the picker-agreement report (``repic agreement``): the device call on a packed
batch, Venn counts from the support masks, the summed pair matrix and the rows of the report's
tables.  The device side is ``rgc_agreement`` (``Context.agreement``); nothing here decides an
edge.

Two boxes of one micrograph and different pickers are *joined* iff ``|dx| <= box_size`` and the
reference's f64 Jaccard quotient exceeds the threshold, strictly (the edge set of the consensus
graph).  ``support[b]`` has bit q set iff box b is joined to a box of picker q; ``mutual`` counts
reciprocal best partners, a one-to-one pairing that is not a maximum matching.
"""
from __future__ import annotations

import numpy as np

SUMMARY_HEADER = "base\tstatus\tboxes\tunsupported\tfully_supported\n"
PAIRS_HEADER = "base\tpicker\tother\tboxes\tsupported\tedges\tmutual\n"
MATRIX_HEADER = "picker\tother\tboxes\tsupported\tedges\tmutual\n"
VENN_HEADER = "picker\tsupported_by\tboxes\n"


def device_call(ctx, batch, ji_threshold, partners=False, timing=False):
    """``Context.agreement`` on a ``pipeline.Batch`` -> (Agreement, (H2D, D2H) bytes, kernel
    times).  ``ctx`` is a context or an object whose ``get()`` makes one (the command opens the
    device only here)."""
    c = ctx.get() if hasattr(ctx, "get") else ctx
    r = c.agreement(batch.n_mg, batch.k, batch.box_size, batch.box_off, batch.x, batch.y,
                    ji_threshold=ji_threshold, partners=partners, timing=timing)
    return r, c.agreement_bytes, (c.kernel_times() if timing else [])


def venn_counts(support, picker_of_box, k):
    """int64 [k, 2^k]: per picker the number of its boxes with each support mask (the bit of a
    box's own picker is never set, so half of each row stays 0)."""
    out = np.zeros((k, 1 << k), np.int64)
    support = np.asarray(support, np.uint8)
    picker_of_box = np.asarray(picker_of_box)
    for p in range(k):
        out[p] = np.bincount(support[picker_of_box == p], minlength=1 << k)[:1 << k]
    return out


def box_pickers(box_off, k):
    """The picker of every box of a batch with offsets ``box_off`` [n_mg*k+1]."""
    cnt = np.diff(np.asarray(box_off, np.int64))
    return np.tile(np.arange(k, dtype=np.int64), len(cnt) // k).repeat(cnt)


def support_counts(support, picker_of_box, k):
    """(unsupported, fully supported) boxes: mask 0, and every other picker's bit set."""
    support = np.asarray(support, np.int64)
    full = ((1 << k) - 1) ^ (1 << np.asarray(picker_of_box, np.int64))
    return int((support == 0).sum()), int((support == full).sum())


def pair_rows(methods, boxes, supported, edges, mutual, base=None):
    """The k (k - 1) rows of one micrograph (or, without ``base``, of the summed matrix): p
    ascending, then q != p ascending."""
    k = len(methods)
    head = "" if base is None else base + "\t"
    return [f"{head}{methods[p]}\t{methods[q]}\t{int(boxes[p])}\t{int(supported[p][q])}\t"
            f"{int(edges[p][q])}\t{int(mutual[p][q])}\n"
            for p in range(k) for q in range(k) if q != p]


def venn_rows(methods, counts):
    """Per picker all 2^(k-1) subsets of the other pickers in ascending mask order, zero counts
    included; the subset as comma-joined names in picker order, ``-`` for the empty set."""
    k = len(methods)
    rows = []
    for p in range(k):
        for mask in range(1 << k):
            if (mask >> p) & 1:
                continue
            names = ",".join(methods[q] for q in range(k) if (mask >> q) & 1) or "-"
            rows.append(f"{methods[p]}\t{names}\t{int(counts[p][mask])}\n")
    return rows


def per_box_rows(methods, box_off, x, y, partner, partner_ji):
    """``<base>_agreement.tsv`` of one micrograph: ``box_off`` its k + 1 offsets, the arrays
    indexed like its boxes from ``box_off[0]`` on, partners as indices in the same frame.
    -> the header and one row per box in batch order."""
    k = len(methods)
    off = np.asarray(box_off, np.int64)
    head = "picker\tline\tx\ty" + "".join(f"\t{m}_line\t{m}_ji" for m in methods) + "\n"
    rows = [head]
    xs, ys = np.asarray(x, np.float64).tolist(), np.asarray(y, np.float64).tolist()
    part = np.asarray(partner).tolist()
    pji = np.asarray(partner_ji, np.float64).tolist()
    for p in range(k):
        for b in range(int(off[p] - off[0]), int(off[p + 1] - off[0])):
            cells = [methods[p], str(b - int(off[p] - off[0])), repr(xs[b]), repr(ys[b])]
            for q in range(k):
                c = part[b][q]
                if q == p or c < 0:
                    cells += ["-", "-"]
                else:
                    cells += [str(c - int(off[q] - off[0])), repr(pji[b][q])]
            rows.append("\t".join(cells) + "\n")
    return rows


def check_box_size(box_size) -> int:
    b = int(box_size)
    if not 1 <= b <= 1 << 26:
        raise ValueError(f"box_size must be in 1..2^26, got {b}")
    return b
