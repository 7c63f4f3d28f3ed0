"""``repic nms`` — remove duplicate picks inside every picker's BOX files.

``in_dir`` holds picker subdirectories, as for ``get_cliques``.  Every non-hidden ``*.box`` of
each goes to ``out_dir/<picker>/<same name>``, so ``repic consensus out_dir ...`` runs on the
result directly.  Within a file, boxes are taken in descending order of their raw score (no
sigmoid; NaN last, ties in file order) and a box is kept iff no box kept before it overlaps it
with a Jaccard index above ``--ji_threshold`` (``repic_amd.nms``, one device pass for all files).

A file is *filtered* iff it parsed without exception and every data line gave a box; its output
is the header line, if any, followed by the kept lines in their original order, byte for byte
(line endings and a missing final newline are preserved).  Every other file (parse exception,
dropped non-float coordinate tokens, empty) is *copied* unchanged, so later commands meet the
same skip / crash behaviour.  ``out_dir/nms_summary.tsv`` has one row per file.

``out_dir`` must not exist or must be empty, and nothing is ever deleted.  One rank only.
"""
from __future__ import annotations

import os
import time

import numpy as np

from .. import _lib, ingest, nms
from . import get_cliques as gc

name = "nms"

SUMMARY = "nms_summary.tsv"
SUMMARY_HEADER = "picker\tfile\tstatus\tboxes\tkept\n"

# counts and seconds of the last run in this process
LAST_RUN: dict = {}


def add_arguments(parser):
    parser.add_argument("in_dir",
                        help="path to input directory containing subdirectories of particle coordinate files ")
    parser.add_argument("out_dir",
                        help="path to output directory (must not exist or be empty; nothing is deleted)")
    parser.add_argument("box_size", type=int,
                        help="particle detection box size (in int[pixels])")
    parser.add_argument("--ji_threshold", type=gc._ji_type, default=_lib.JI_DEFAULT, metavar="T",
                        help="suppress a pick whose Jaccard index with a higher-scored pick of "
                             "the same file exceeds T (float, 0 <= T < 1; default: 0.3)")
    parser.add_argument("--threads", type=int, default=None,
                        help="host BOX-parser threads (does not change outputs)")
    parser.add_argument("--device", type=int, default=None,
                        help="HIP device (default: $LOCAL_RANK or 0)")


def _split(raw: bytes):
    """(header line or None, data lines) of a BOX file's bytes, line endings kept.  The header
    rule is the parser's: line 1 is a header iff its first token is not a Python float."""
    lines = raw.splitlines(keepends=True)
    if not lines:
        return None, []
    tok = lines[0].decode("utf-8", "replace").split()
    if tok and ingest._is_float(tok[0]):
        return None, lines
    return lines[0], lines[1:]


def main(args):
    assert os.path.exists(args.in_dir), "Error - input directory does not exist"
    t = getattr(args, "ji_threshold", None)
    t = _lib.JI_DEFAULT if t is None else _lib.check_ji_threshold(t)
    box_size = int(args.box_size)
    if not 1 <= box_size <= 1 << 26:
        raise ValueError(f"box_size must be in 1..2^26, got {box_size}")
    world, _, local = gc._dist_env()
    if world > 1:
        raise _lib.RGCError(
            f"repic nms runs on one rank (WORLD_SIZE={world}): files are independent, so split "
            "the picker directories between runs instead (nothing was written)")
    out_dir = args.out_dir
    if os.path.lexists(out_dir) and (not os.path.isdir(out_dir) or os.listdir(out_dir)):
        raise _lib.RGCError(f"repic nms: {out_dir} exists and is not an empty directory; "
                            "nothing is ever deleted here, so name a new one "
                            "(nothing was written)")
    t0 = time.time()
    methods = ingest.list_methods(args.in_dir)
    files = []   # (picker, name)
    for m in methods:
        d = os.path.join(args.in_dir, m)
        files.extend((m, f) for f in sorted(os.listdir(d), key=str)
                     if f.endswith(".box") and not f.startswith(".")
                     and os.path.isfile(os.path.join(d, f)))
    paths = [os.path.join(args.in_dir, m, f) for m, f in files]
    parsed = ingest.parse_many(paths, getattr(args, "threads", None)) if paths else []
    raws, splits, todo, segs, orders = [], [], [], [], []
    for i, (p, pf) in enumerate(zip(paths, parsed)):
        with open(p, "rb") as f:
            raws.append(f.read())
        splits.append(_split(raws[-1]))
        if pf.exc is None and pf.n > 0 and pf.n == len(splits[-1][1]):
            order = nms.nms_order(pf.s)
            todo.append(i)
            orders.append(order)
            segs.append((np.asarray(pf.x)[order], np.asarray(pf.y)[order]))
    t_parse = time.time() - t0
    masks = []
    if segs:   # (the context is nms_keep's own: nothing touches a device before this line)
        dev = args.device if getattr(args, "device", None) is not None else local
        masks = nms.nms_keep(segs, box_size, t, device=dev)
    t_dev = time.time() - t0 - t_parse
    keep_of = {}
    for i, order, mk in zip(todo, orders, masks):
        mask = np.zeros(len(order), bool)
        mask[order] = mk
        keep_of[i] = mask
    os.makedirs(out_dir, exist_ok=True)
    rows, n_boxes, n_kept = [], 0, 0
    for m in methods:
        os.makedirs(os.path.join(out_dir, m), exist_ok=True)
    for i, (m, f) in enumerate(files):
        mask = keep_of.get(i)
        if mask is None:
            data, status, nb = raws[i], "copied", parsed[i].n
            nk = nb
        else:
            head, lines = splits[i]
            data = (head or b"") + b"".join(ln for ln, k in zip(lines, mask) if k)
            status, nb, nk = "filtered", len(mask), int(mask.sum())
        with open(os.path.join(out_dir, m, f), "wb") as o:
            o.write(data)
        rows.append(f"{m}\t{f}\t{status}\t{nb}\t{nk}\n")
        n_boxes += nb
        n_kept += nk
    with open(os.path.join(out_dir, SUMMARY), "wt") as o:
        o.write(SUMMARY_HEADER)
        o.writelines(rows)
    LAST_RUN.clear()
    LAST_RUN.update(files=len(files), filtered=len(todo), boxes=n_boxes, kept=n_kept,
                    parse_s=t_parse, device_s=t_dev, total_s=time.time() - t0)
    print(f"repic nms: {len(files)} files ({len(todo)} filtered), {n_boxes} boxes, "
          f"{n_boxes - n_kept} suppressed")
