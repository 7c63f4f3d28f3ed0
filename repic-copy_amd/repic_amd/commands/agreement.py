"""``repic agreement`` — how much the pickers agree, per box and per picker pair.

``repic consensus`` writes a particle only where all k pickers meet (or M of them with
``--min_pickers``); how many it finds is decided by the overlaps between picker pairs.  This
command reports them before a consensus is chosen: for every box which other pickers have a box
joined to it, and for every ordered picker pair the boxes supported, the joined pairs and the
reciprocal best partners (``rgc_agreement``, one device pass per batch).  Two boxes of one
micrograph and different pickers are joined iff ``|dx| <= box_size`` and the reference's f64
Jaccard quotient exceeds ``--ji_threshold``, strictly: the edge set of the consensus graph.

Same plugin protocol (``name``, ``add_arguments``, ``main``).  The front half is ``get_cliques``'
own, by import, as for ``consensus``: ``DirIndex``, ``probe_start_method``, ``plan_chunk`` on a
parser thread, ``split_batches``; so micrograph pairing, processing order and skip rules are the
consensus commands'.  Scores are not used.

Files in ``out_dir`` (pickers in ``list_methods`` order, ok micrographs in processing order):

``agreement_summary.tsv``  one row per micrograph: its boxes, those with no support at all and
    those supported by every other picker (``skip`` rows carry zeros)
``agreement_pairs.tsv``    per ok micrograph and ordered pair (picker, other): the picker's
    boxes, how many have a box of ``other`` joined to them, the joined pairs, and the reciprocal
    best partners (a one-to-one pairing; not a maximum matching)
``agreement_matrix.tsv``   the same summed over the ok micrographs, k (k - 1) rows
``agreement_venn.tsv``     per picker and subset of the other pickers, the boxes supported by
    exactly that subset (all 2^(k-1) subsets, zero counts included)
``<base>_agreement.tsv``   only with ``--per_box``: one row per box with, for every other picker,
    the line of its best partner in that picker's file and their Jaccard index

A skipped micrograph (not all pickers have a file) gets a ``skip`` row.  At the first micrograph
whose files make the reference's parser raise, the rows so far are written and the same exception
is raised.  A micrograph without any joined pair is ok here, with zeros: this is a report, not a
consensus.  ``out_dir`` must not exist or must be empty, and nothing is ever deleted.  One rank
only.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from .. import _lib, agreement as ag
from ..pipeline import split_batches
from . import get_cliques as gc

name = "agreement"

SUMMARY = "agreement_summary.tsv"
PAIRS = "agreement_pairs.tsv"
MATRIX = "agreement_matrix.tsv"
VENN = "agreement_venn.tsv"
PER_BOX_SUFFIX = "_agreement.tsv"

# phase seconds, counts and the library's host<->device byte counts of the last run in this
# process (tools/agreement_bench.py reads them)
LAST_RUN: dict = {}


def add_arguments(parser):
    parser.add_argument("in_dir",
                        help="path to input directory containing subdirectories of particle coordinate files ")
    parser.add_argument("out_dir",
                        help="path to output directory (must not exist or be empty; nothing is deleted)")
    parser.add_argument("box_size", type=int,
                        help="particle detection box size (in int[pixels])")
    gc.add_ji_threshold(parser)
    parser.add_argument("--per_box", action="store_true",
                        help="also write <base>_agreement.tsv: per box its best partner from "
                             "every other picker and their Jaccard index")
    parser.add_argument("--batch_boxes", type=int, default=1 << 25,
                        help="max boxes per device batch (does not change outputs)")
    parser.add_argument("--threads", type=int, default=None,
                        help="host BOX-parser threads (does not change outputs)")
    parser.add_argument("--device", type=int, default=None,
                        help="HIP device (default: $LOCAL_RANK or 0)")
    parser.add_argument("--listing", type=gc._load_listing, default=None, help=argparse.SUPPRESS)


class _LazyContext:
    """The device context, opened by the first device call (``agreement.device_call``)."""

    def __init__(self, device):
        self.device, self._ctx = device, None

    def get(self):
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
        return self._ctx

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None


class _NoWriter:
    """The front half's writer slot: this command writes its few tables itself."""

    def close(self):
        pass


def main(args):
    assert os.path.exists(args.in_dir), "Error - input directory does not exist"
    # every check comes before a device context exists or anything is written
    t = getattr(args, "ji_threshold", None)
    args.ji_threshold = _lib.JI_DEFAULT if t is None else _lib.check_ji_threshold(t)
    args.box_size = ag.check_box_size(args.box_size)
    world, _, local = gc._dist_env()
    if world > 1:
        raise _lib.RGCError(
            f"repic agreement runs on one rank (WORLD_SIZE={world}): micrographs are "
            "independent, so split them between runs instead (nothing was written)")
    out_dir = args.out_dir
    k_pre = len(gc._methods_after_reset(args.in_dir, out_dir))
    if k_pre > _lib.MAX_K:
        raise _lib.RGCError(f"{k_pre} picker directories in {args.in_dir}: this build supports "
                            f"at most {_lib.MAX_K} (nothing was written)")
    if os.path.lexists(out_dir) and (not os.path.isdir(out_dir) or os.listdir(out_dir)):
        raise _lib.RGCError(f"repic agreement: {out_dir} exists and is not an empty directory; "
                            "nothing is ever deleted here, so name a new one "
                            "(nothing was written)")
    dev = args.device if getattr(args, "device", None) is not None else local
    ctx = _LazyContext(dev)
    runs = []

    def run_cls(*a):
        runs.append(_Run(*a))
        return runs[-1]
    t0 = time.time()
    try:
        try:
            # (the shared front half resets out_dir: an empty directory at most, checked above)
            gc._main(args, ctx, 1, 0, run_cls=run_cls, make_writer=lambda a: _NoWriter())
        except BaseException:
            # the reference's parser raised at a micrograph: the rows so far are written, and
            # the parser's exception is the one that leaves (any other failure writes nothing)
            if runs and runs[0].parser_raised:
                try:
                    runs[0].write_tables()
                except OSError as e:
                    print(f"repic agreement: the tables were not written: {e}", file=sys.stderr)
            raise
        runs[0].write_tables()
    finally:
        ctx.close()
        LAST_RUN.clear()
        if runs:   # (gc._main fills its LAST_RUN once the run exists)
            LAST_RUN.update(gc.LAST_RUN)
        LAST_RUN["total_s"] = time.time() - t0
    r = runs[0]
    print(f"repic agreement: {r.stats['micrographs']} micrographs, {r.stats['boxes']} boxes, "
          f"{r.stats['edges']} joined pairs")


class _Res:
    """Flat host results of a chunk (copies): per box, per micrograph, and with --per_box the
    partners as chunk-batch indices."""

    def __init__(self, r, box0=0):
        self.support = r.support
        self.pair_edges, self.pair_supported = r.pair_edges, r.pair_supported
        self.pair_mutual = r.pair_mutual
        self.partner, self.partner_ji = r.partner, r.partner_ji
        if self.partner is not None and box0:
            self.partner = np.where(self.partner >= 0, self.partner + box0, -1).astype(np.int32)

    def append(self, o):
        for f in ("support", "pair_edges", "pair_supported", "pair_mutual"):
            setattr(self, f, np.concatenate([getattr(self, f), getattr(o, f)]))
        if self.partner is not None:
            self.partner = np.concatenate([self.partner, o.partner])
            self.partner_ji = np.concatenate([self.partner_ji, o.partner_ji])
        return self


class _Run(gc._Run):
    """get_cliques' chunk pipeline with the device stage replaced by the agreement call and the
    write stage by the report's rows."""

    def __init__(self, *a):
        super().__init__(*a)
        self.per_box = bool(getattr(self.args, "per_box", False))
        self.parser_raised = False
        self.timing = bool(getattr(self.args, "agreement_timing", False))
        self.stats.update(boxes=0, skipped=0, h2d_bytes=0, d2h_bytes=0)
        k = self.k
        self.summary, self.pairs = [], []
        self.tot_boxes = np.zeros(k, np.int64)
        self.tot = {f: np.zeros((k, k), np.int64) for f in ("supported", "edges", "mutual")}
        self.venn = np.zeros((k, 1 << k), np.int64)

    def device(self, ch):
        ch.res = None
        if ch.batch is None:
            return
        t0 = time.time()
        b = ch.batch
        for m0, m1 in split_batches(np.diff(b.box_off[::self.k]).tolist(),
                                    getattr(self.args, "batch_boxes", 1 << 25)):
            part = b if (m0 == 0 and m1 == b.n_mg) else b.slice(m0, m1)
            r, (h2d, d2h), times = ag.device_call(self.ctx, part, self.args.ji_threshold,
                                                  partners=self.per_box, timing=self.timing)
            for nm, ms in times:
                self.stats[nm + "_ms"] = self.stats.get(nm + "_ms", 0.0) + ms
            self.stats["h2d_bytes"] += h2d
            self.stats["d2h_bytes"] += d2h
            res = _Res(r, int(b.box_off[m0 * self.k]))
            ch.res = res if ch.res is None else ch.res.append(res)
        self.stats["device_s"] += time.time() - t0

    def write(self, ch, writer, stop=None):
        mgs = ch.mgs if stop is None else ch.mgs[:stop]
        t0 = time.time()
        k, r, b = self.k, ch.res, ch.batch
        raise_at = None
        for mg in mgs:
            if mg.status == "skip":
                self.summary.append(f"{mg.base}\tskip\t0\t0\t0\n")
                self.stats["skipped"] += 1
                continue
            if mg.status == "crash":
                raise_at, self.parser_raised = mg, True
                break
            s = mg.slot
            off = b.box_off[s * k:s * k + k + 1]
            b0, b1 = int(off[0]), int(off[-1])
            sup = r.support[b0:b1]
            pick = np.arange(k).repeat(np.diff(off))
            uns, full = ag.support_counts(sup, pick, k)
            self.summary.append(f"{mg.base}\tok\t{b1 - b0}\t{uns}\t{full}\n")
            boxes = np.diff(off)
            self.pairs.extend(ag.pair_rows(self.methods, boxes, r.pair_supported[s],
                                           r.pair_edges[s], r.pair_mutual[s], base=mg.base))
            self.tot_boxes += boxes
            self.tot["supported"] += r.pair_supported[s]
            self.tot["edges"] += r.pair_edges[s]
            self.tot["mutual"] += r.pair_mutual[s]
            self.venn += ag.venn_counts(sup, pick, k)
            if self.per_box:
                part = r.partner[b0:b1]
                rows = ag.per_box_rows(self.methods, off, b.x[b0:b1], b.y[b0:b1],
                                       np.where(part >= 0, part - b0, -1), r.partner_ji[b0:b1])
                with open(os.path.join(self.args.out_dir, mg.base + PER_BOX_SUFFIX), "wt") as o:
                    o.writelines(rows)
            self.stats["micrographs"] += 1
            self.stats["boxes"] += b1 - b0
            self.stats["edges"] += int(np.triu(r.pair_edges[s]).sum())
        self.stats["write_s"] += time.time() - t0
        return raise_at

    def write_tables(self):
        """The four tables of the run, from the rows so far."""
        out = self.args.out_dir
        tables = (
            (SUMMARY, ag.SUMMARY_HEADER, self.summary),
            (PAIRS, ag.PAIRS_HEADER, self.pairs),
            (MATRIX, ag.MATRIX_HEADER,
             ag.pair_rows(self.methods, self.tot_boxes, self.tot["supported"], self.tot["edges"],
                          self.tot["mutual"])),
            (VENN, ag.VENN_HEADER, ag.venn_rows(self.methods, self.venn)))
        for fname, head, rows in tables:
            with open(os.path.join(out, fname), "wt") as o:
                o.write(head)
                o.writelines(rows)
