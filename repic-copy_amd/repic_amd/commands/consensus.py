"""``repic consensus`` — picker BOX directories to the final consensus ``.box`` files in one
device pass.

The reference workflow is always ``get_cliques`` followed at once by ``run_ilp`` (run.sh):
the four pickles and the TSV ``get_cliques`` writes per micrograph exist only so that
``run_ilp`` can read them again.  This command does both halves on the device without the
files in between (``rgc_consensus``, ABI 10): the per-clique arrays (rows, weights,
confidences, consensus ids) stay in HBM from the clique kernels through the set-packing solver,
and only the picked particles come back.

Same plugin protocol (``name``, ``add_arguments``, ``main``).  The front half is
``get_cliques``' own, by import: the ``MAX_K`` check before anything is deleted, the ``out_dir``
reset, ``DirIndex``, ``probe_start_method``, ``plan_chunk`` on a parser thread that overlaps the
device, ``split_batches``.  Outputs in ``out_dir``: one ``<base>.box`` per micrograph, byte for
byte what ``get_cliques`` + ``run_ilp`` write (empty for a skipped micrograph), and one
``consensus_summary.tsv`` for the run.  No pickles, no ``_runtime.tsv``, no per-micrograph
status files.

Failure semantics are the two-step path's: at the first micrograph where ``get_cliques`` would
raise (parse crash, no edges -> ValueError, no cliques -> UnboundLocalError) every earlier
micrograph's ``.box`` exists and the same exception class is raised; an ok micrograph whose
packing is empty raises ``run_ilp``'s AssertionError; NODE_LIMIT / HEURISTIC micrographs get
``run_ilp``'s warnings on stderr.  There is no ``--multi_out`` (the reference's ``run_ilp``
raises on such inputs); ``--members`` gives what that path was meant to: next to each
``<base>.box`` a ``<base>_members.tsv`` whose row i holds, picker by picker, the boxes that
made up ``.box`` line i, followed by every picker's boxes that are in no written pick
(``rgc_consensus_members`` / ``rgc_write_members``), and one ``consensus_pickers.tsv`` for the
run.  Without the flag nothing changes.

``--dedup_ji T`` applies the consensus rule to the written picks themselves: the set packing
makes the chosen cliques vertex-disjoint, which does not keep two of them from sitting on the
same particle.  Each micrograph's lines, in their written order (confidence descending, which is
the priority order) and with the rounded coordinates that go into the file, are one segment of a
greedy non-maximum suppression on the device (``rgc_nms``): a line is dropped iff a line kept
before it has a Jaccard index with it above T, so no two lines of a written ``.box`` have
JI > T.  With ``--num_particles N`` the device returns all picks, the suppression runs, and the
first N survivors are written.  ``consensus_dedup.tsv`` (one row per ok micrograph) counts what
was picked, suppressed and written.  ``--dedup_ji`` with ``--members`` is refused (the members of
a suppressed pick would have to become leftovers, which is not defined yet).

``--min_pickers M`` (2 <= M <= k) adds the particles on which at least M of the k pickers agree,
in tiers: full agreement first (exactly the plain output, which every ``.box`` starts with), then
for t = k-1 .. M the cliques of every subset of t pickers among the boxes that no pick so far
explains (a box is explained when its JI with a pick's consensus box exceeds the run's
threshold), one set packing per micrograph and tier (``rgc_consensus_tiers``).  Next to each
``<base>.box`` a ``<base>_tiers.tsv`` names, line by line, the tier and the pickers of each
written pick, and ``consensus_tiers.tsv`` counts the columns and picks per tier.  A micrograph is
ok when some tier has a clique.  ``--min_pickers`` with ``--get_cc`` or ``--members`` is refused.

There is no multi-rank form yet: with ``WORLD_SIZE > 1`` the command raises
before it creates a device context or touches ``out_dir``.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from .. import _lib, ilp
from ..pipeline import split_batches
from ..writers import BoxWriter
from . import get_cliques as gc
from .run_ilp import STATUS_NAMES

name = "consensus"

SUMMARY = "consensus_summary.tsv"
SUMMARY_HEADER = "base\tstatus\tcliques\tpicks\tcc_max\tcc_cnt\tilp_status\trel_gap\n"
# --members: one line per ok micrograph and picker
PICKERS = "consensus_pickers.tsv"
PICKERS_HEADER = "base\tpicker\tboxes\tin_clique\tin_consensus\n"
# --dedup_ji: one line per ok micrograph
DEDUP = "consensus_dedup.tsv"
DEDUP_HEADER = "base\tpicked\tsuppressed\twritten\n"
# --min_pickers: one line per ok micrograph (columns and picks per tier k..M), and next to every
# <base>.box the tier and pickers of each of its lines
TIERS = "consensus_tiers.tsv"
TIERS_SUFFIX = _lib.TIERS_SUFFIX

# phase seconds, counts and the library's host<->device byte counts of the last run in this
# process (tools/consensus_bench.py reads them)
LAST_RUN: dict = {}


def add_arguments(parser):
    parser.add_argument("in_dir",
                        help="path to input directory containing subdirectories of particle coordinate files ")
    parser.add_argument("out_dir",
                        help="path to output directory (WARNING - script will delete directory if it exists)")
    parser.add_argument("box_size", type=int,
                        help="particle detection box size (in int[pixels])")
    parser.add_argument("--num_particles", type=int,
                        help="filter for the number of expected particles (int)")
    parser.add_argument("--get_cc", action="store_true",
                        help="filters cliques for those in the largest Connected Component (CC)")
    parser.add_argument("--members", action="store_true",
                        help="also write <base>_members.tsv (per pick its box from every picker, "
                             "then every picker's boxes in no pick) and consensus_pickers.tsv")
    parser.add_argument("--min_pickers", type=int, default=None, metavar="M",
                        help="also pick particles on which at least M of the k pickers agree "
                             "(int, 2 <= M <= k; default: all k), in tiers below the full "
                             "agreement; also writes <base>_tiers.tsv and consensus_tiers.tsv")
    gc.add_ji_threshold(parser)
    parser.add_argument("--dedup_ji", type=gc._ji_type, default=None, metavar="T",
                        help="drop a written pick whose Jaccard index with a pick written before "
                             "it exceeds T (float, 0 <= T < 1; default: no suppression); also "
                             "writes consensus_dedup.tsv")
    parser.add_argument("--node_limit", type=int, default=0,
                        help="branch-and-bound nodes per conflict component (0: the library "
                             "default), as for run_ilp")
    parser.add_argument("--batch_boxes", type=int, default=1 << 25,
                        help="max boxes per device batch (does not change outputs)")
    parser.add_argument("--threads", type=int, default=None,
                        help="host BOX-parser threads (does not change outputs)")
    parser.add_argument("--device", type=int, default=None,
                        help="HIP device (default: $LOCAL_RANK or 0)")
    parser.add_argument("--listing", type=gc._load_listing, default=None, help=argparse.SUPPRESS)


def main(args):
    assert os.path.exists(args.in_dir), "Error - input directory does not exist"
    gc.ji_threshold_of(args)   # (ValueError before a context exists or anything is deleted)
    dedup = dedup_ji_of(args)  # (likewise)
    if dedup is not None and getattr(args, "members", False):
        raise _lib.RGCError(
            "repic consensus: --dedup_ji and --members cannot be combined: the members of a "
            "suppressed pick would have to become leftovers, which is not defined yet "
            "(nothing was deleted or written)")
    min_pickers_of(args)       # (likewise)
    world, rank, local = gc._dist_env()
    if world > 1:
        raise _lib.RGCError(
            f"repic consensus runs on one rank (WORLD_SIZE={world}): the sharded form needs "
            "the box-id exchange of get_cliques' multi-rank path and is not built yet; run "
            "get_cliques and run_ilp under torchrun instead (nothing was deleted or written)")
    args.multi_out = False
    dev = args.device if getattr(args, "device", None) is not None else local
    ctx = _lib.Context(dev)
    runs = []

    def run_cls(*a):
        runs.append(_Run(*a))
        return runs[-1]
    t0 = time.time()
    try:
        gc._main(args, ctx, 1, 0, run_cls=run_cls,
                 make_writer=lambda a: BoxWriter(getattr(a, "threads", None)))
    finally:
        ctx.close()
        LAST_RUN.clear()
        LAST_RUN.update(gc.LAST_RUN)
        LAST_RUN["total_s"] = time.time() - t0
        if runs and os.path.isdir(args.out_dir):
            with open(os.path.join(args.out_dir, SUMMARY), "wt") as o:
                o.write(SUMMARY_HEADER)
                o.writelines(runs[0].summary)
            if runs[0].members:
                with open(os.path.join(args.out_dir, PICKERS), "wt") as o:
                    o.write(PICKERS_HEADER)
                    o.writelines(runs[0].pickers)
            if runs[0].dedup is not None:
                with open(os.path.join(args.out_dir, DEDUP), "wt") as o:
                    o.write(DEDUP_HEADER)
                    o.writelines(runs[0].dedup_rows)
            if runs[0].min_pickers is not None:
                with open(os.path.join(args.out_dir, TIERS), "wt") as o:
                    o.write(tiers_header(runs[0].k, runs[0].min_pickers))
                    o.writelines(runs[0].tier_rows)


def dedup_ji_of(args):
    """The run's ``--dedup_ji`` threshold, validated (ValueError outside [0, 1)), or None without
    the option (also when a hand-built namespace lacks it)."""
    t = getattr(args, "dedup_ji", None)
    return None if t is None else _lib.check_ji_threshold(t)


def min_pickers_of(args):
    """The run's ``--min_pickers`` M, validated before a context exists or anything is deleted
    (RGCError: with --get_cc or --members, or outside 2..k), or None without the option."""
    m = getattr(args, "min_pickers", None)
    if m is None:
        return None
    for flag in ("get_cc", "members"):
        if getattr(args, flag, False):
            raise _lib.RGCError(
                f"repic consensus: --min_pickers and --{flag} cannot be combined "
                "(nothing was deleted or written)")
    k = len(gc._methods_after_reset(args.in_dir, args.out_dir))
    if not 2 <= int(m) <= k:
        raise _lib.RGCError(
            f"repic consensus: --min_pickers must be in 2..{k} (the picker directories of "
            f"{args.in_dir}), got {m} (nothing was deleted or written)")
    return int(m)


def tiers_header(k, m):
    return "base" + "".join(f"\tcols_{t}\tpicks_{t}" for t in range(k, m - 1, -1)) + "\n"


class _Res:
    """Flat host results of a chunk: per-micrograph arrays and the pick arrays (copies)."""

    PER_MG = ("status", "cc_max", "cc_cnt", "n_vert", "n_edges_mg", "clique_cnt", "sel_cnt",
              "ilp_status", "ilp_gap")

    # --members: per pick (rows of k), per segment (micrograph, picker), per leftover
    MEMBERS = ("pmx", "pmy", "seg_boxes", "in_clique", "left_x", "left_y")

    # --min_pickers: per pick, and per micrograph the columns of each tier
    TIERS = ("ptier", "pmask", "tier_cols")

    def __init__(self, r, box_off=None, dedup=None):
        # --dedup_ji: (picks the device returned, picks suppressed) per micrograph
        self.dedup = dedup is not None
        if self.dedup:
            self.picked, self.suppressed = dedup
        for f in ("status", "cc_max", "cc_cnt", "n_vert", "n_edges_mg", "clique_cnt"):
            setattr(self, f, np.array(getattr(r.run, f)))
        self.sel_cnt, self.ilp_status, self.ilp_gap = r.sel_cnt, r.ilp_status, r.ilp_gap
        self.pick_off = r.pick_off
        self.px, self.py, self.pconf = r.px, r.py, r.pconf
        self.tiers = r.ptier is not None
        if self.tiers:
            self.ptier, self.pmask, self.tier_cols = r.ptier, r.pmask, r.tier_cols
        self.members = r.pmx is not None
        if self.members:
            self.pmx, self.pmy, self.in_clique = r.pmx, r.pmy, r.in_clique
            self.left_off, self.left_x, self.left_y = r.left_off, r.left_x, r.left_y
            self.seg_boxes = np.diff(np.asarray(box_off, np.int64))

    def append(self, o):
        for f in self.PER_MG:
            setattr(self, f, np.concatenate([getattr(self, f), getattr(o, f)]))
        self.pick_off = np.concatenate([self.pick_off, o.pick_off[1:] + self.pick_off[-1]])
        self.px = np.concatenate([self.px, o.px])
        self.py = np.concatenate([self.py, o.py])
        self.pconf = np.concatenate([self.pconf, o.pconf])
        if self.dedup:
            self.picked = np.concatenate([self.picked, o.picked])
            self.suppressed = np.concatenate([self.suppressed, o.suppressed])
        if self.tiers:
            for f in self.TIERS:
                setattr(self, f, np.concatenate([getattr(self, f), getattr(o, f)]))
        if self.members:
            for f in self.MEMBERS:
                setattr(self, f, np.concatenate([getattr(self, f), getattr(o, f)]))
            self.left_off = np.concatenate([self.left_off, o.left_off[1:] + self.left_off[-1]])
        return self


class _Run(gc._Run):
    """get_cliques' chunk pipeline with the device stage replaced by ``Context.consensus`` and
    the write stage by the BOX writer."""

    def __init__(self, *a):
        super().__init__(*a)
        self.stats.update(picks=0, h2d_bytes=0, d2h_bytes=0)
        self.summary = []
        self._empty = None
        self.members = bool(getattr(self.args, "members", False))
        self.pickers = []
        self.dedup = dedup_ji_of(self.args)
        self.dedup_rows = []
        if self.dedup is not None:
            self.stats.update(suppressed=0, dedup_s=0.0, dedup_h2d_bytes=0, dedup_d2h_bytes=0)
        self.min_pickers = getattr(self.args, "min_pickers", None)
        self.tier_rows = []
        if self.min_pickers is not None:
            self.stats.update({f"picks_tier_{t}": 0 for t in range(self.min_pickers, self.k + 1)})

    def device(self, ch):
        ch.res = None
        if ch.batch is None:
            return
        t0 = time.time()
        b = ch.batch
        flags = 0
        if getattr(self.args, "no_fused", False):
            flags |= _lib.F_NO_FUSED
        if self.args.get_cc:
            flags |= _lib.F_GET_CC
        for m0, m1 in split_batches(np.diff(b.box_off[::self.k]).tolist(),
                                    getattr(self.args, "batch_boxes", 1 << 25)):
            part = b if (m0 == 0 and m1 == b.n_mg) else b.slice(m0, m1)
            more = {"members": True} if self.members else {}
            call = self.ctx.consensus
            if self.min_pickers is not None and self.min_pickers < self.k:
                call, more = self.ctx.consensus_tiers, {"min_pickers": self.min_pickers}
                if getattr(self.args, "tiers_timing", False):
                    more["timing"] = True
            r = call(part.n_mg, part.k, part.box_size, part.box_off, part.id_base,
                     part.x, part.y, part.score, flags=flags,
                     node_limit=getattr(self.args, "node_limit", 0) or 0,
                     num_particles=(self.args.num_particles if self.dedup is None else None),
                     ji_threshold=self.ji, **more)
            if more.get("timing"):
                for nm, ms in self.ctx.kernel_times():
                    self.stats[nm + "_ms"] = self.stats.get(nm + "_ms", 0.0) + ms
            if self.min_pickers is not None and r.ptier is None:
                # --min_pickers k: the plain call; every pick is of tier k, by all pickers
                r.ptier = np.full(r.n_picked, self.k, np.int32)
                r.pmask = np.full(r.n_picked, (1 << self.k) - 1, np.int32)
                okc = np.asarray(r.run.status) == _lib.OK
                r.tier_cols = np.where(okc, np.asarray(r.run.clique_cnt), 0)[:, None].astype(np.int64)
            self.stats["h2d_bytes"] += r.h2d_bytes
            self.stats["d2h_bytes"] += r.d2h_bytes
            if self.dedup is not None:
                res = _Res(r, dedup=self._suppress(r, part.box_size))
            else:
                res = _Res(r, part.box_off) if self.members else _Res(r)
            ch.res = res if ch.res is None else ch.res.append(res)
        self.stats["device_s"] += time.time() - t0
        ok = ch.res.status == _lib.OK
        self.stats["edges"] += int(ch.res.n_edges_mg[ok].sum())
        self.stats["cliques"] += int(ch.res.tier_cols[ok].sum() if ch.res.tiers
                                     else ch.res.clique_cnt[ok].sum())

    def _suppress(self, r, box_size):
        """--dedup_ji on one consensus call's picks, in place: every micrograph's lines are one
        NMS segment in their written order, with the coordinates that go into the file;
        suppressed lines are dropped and, with --num_particles N, the first N survivors stay.
        -> per micrograph (picks the device returned, picks suppressed)."""
        t0 = time.time()
        timing = bool(getattr(self.args, "dedup_timing", False))
        keep, kept = self.ctx.nms(r.pick_off, r.px, r.py, box_size, self.dedup, timing=timing)
        if timing:
            for nm, ms in self.ctx.kernel_times():
                self.stats[nm + "_ms"] = self.stats.get(nm + "_ms", 0.0) + ms
        h2d, d2h = self.ctx.nms_bytes
        for f, v in (("h2d_bytes", h2d), ("d2h_bytes", d2h), ("dedup_h2d_bytes", h2d),
                     ("dedup_d2h_bytes", d2h)):
            self.stats[f] += v
        picked = np.diff(r.pick_off)
        keep = keep.astype(bool)
        n_par = self.args.num_particles
        written = keep
        if n_par is not None and n_par >= 0:
            # rank of each survivor within its micrograph (the library's rule: < 0 keeps all)
            before = np.concatenate([[0], np.cumsum(keep)])   # survivors before each line
            rank = before[:-1] - np.repeat(before[r.pick_off[:-1]], picked)
            written = keep & (rank < n_par)
        off = np.concatenate([[0], np.cumsum(written)])[r.pick_off].astype(np.int64)
        r.pick_off = off
        r.px, r.py, r.pconf, r.pcol = r.px[written], r.py[written], r.pconf[written], r.pcol[written]
        if r.ptier is not None:
            r.ptier, r.pmask = r.ptier[written], r.pmask[written]
        r.n_picked = int(off[-1])
        self.stats["suppressed"] += int(picked.sum() - kept.sum())
        self.stats["dedup_s"] += time.time() - t0
        return picked.astype(np.int64), (picked - kept).astype(np.int64)

    def write(self, ch, writer, stop=None):
        mgs = ch.mgs if stop is None else ch.mgs[:stop]
        t0 = time.time()
        r = ch.res
        bases, offs, counts, segs = [], [], [], []
        raise_at = None
        k = self.k

        def flush():
            if bases:
                more = {}
                if self.members:
                    more["members"] = (list(self.methods),) + tuple(
                        getattr(r, f) if r is not None else None
                        for f in ("pmx", "pmy")) + (list(segs),) + tuple(
                        getattr(r, f) if r is not None else None
                        for f in ("left_off", "left_x", "left_y"))
                writer.boxes(self.args.out_dir, list(bases), self.args.box_size, list(offs),
                             list(counts), r.px if r is not None else None,
                             r.py if r is not None else None,
                             r.pconf if r is not None else None, **more)
                bases.clear(), offs.clear(), counts.clear(), segs.clear()
        for mg in mgs:
            print(f"\n--- {mg.base} ---\n")
            if mg.status == "skip":
                print("Skipping micrograph - not all methods have picked particles...")
                bases.append(mg.base), offs.append(0), counts.append(-1), segs.append(0)
                self.summary.append(f"{mg.base}\tskip\t0\t0\t0\t0\t-\t-\n")
            elif mg.status == "crash" or r.status[mg.slot] != _lib.OK:
                raise_at = mg
                break
            else:
                s = mg.slot
                st = int(r.ilp_status[s])
                if st == ilp.NODE_LIMIT:
                    print(f"Warning - {mg.base}: node limit reached in a conflict component and "
                          f"its Lagrangian bound leaves a gap above 1e-4: the packing is the "
                          f"best found, not proven optimal", file=sys.stderr)
                elif st == ilp.HEURISTIC:
                    print(f"Warning - {mg.base}: a conflict component of more than "
                          f"{_lib.ilp_big_max()} cliques was not searched; the packing is greedy "
                          f"+ swap local search and its Lagrangian bound leaves a gap above 1e-4",
                          file=sys.stderr)
                if r.sel_cnt[s] < 1:      # run_ilp.py:66-69: at least one clique chosen
                    raise_at = self._empty = mg
                    break
                n = int(r.pick_off[s + 1] - r.pick_off[s])
                bases.append(mg.base), offs.append(int(r.pick_off[s])), counts.append(n)
                segs.append(s * k)
                if self.members:
                    self.pickers.extend(
                        f"{mg.base}\t{self.methods[p]}\t{int(r.seg_boxes[s * k + p])}\t"
                        f"{int(r.in_clique[s * k + p])}\t{n}\n" for p in range(k))
                if r.dedup:
                    self.dedup_rows.append(
                        f"{mg.base}\t{int(r.picked[s])}\t{int(r.suppressed[s])}\t{n}\n")
                n_cl = int(r.clique_cnt[s])
                if r.tiers:
                    n_cl = self._write_tiers(mg.base, r, s)
                self.summary.append(
                    f"{mg.base}\tok\t{n_cl}\t{n}\t{int(r.cc_max[s])}\t"
                    f"{int(r.cc_cnt[s])}\t{STATUS_NAMES[st]}\t{float(r.ilp_gap[s]):.3e}\n")
                self.stats["micrographs"] += 1
                self.stats["picks"] += n
            if len(bases) >= gc.GROUP_MG:
                flush()
        flush()
        self.stats["write_s"] += time.time() - t0
        return raise_at

    def _write_tiers(self, base, r, s):
        """--min_pickers: ``<base>_tiers.tsv`` (line i: the tier and the comma-joined pickers of
        ``.box`` line i, from the arrays the ``.box`` is written from) and the micrograph's row of
        consensus_tiers.tsv -> its columns summed over the tiers."""
        k, p0, p1 = self.k, int(r.pick_off[s]), int(r.pick_off[s + 1])
        tier, mask = r.ptier[p0:p1], r.pmask[p0:p1]
        # one string per distinct (tier, subset), then one join: no per-line formatting
        codes, inv = np.unique(tier.astype(np.int64) << 8 | mask, return_inverse=True)
        kinds = np.array([f"{c >> 8}\t" + ",".join(self.methods[p] for p in range(k)
                                                   if (c >> p) & 1) + "\n"
                          for c in codes.tolist()], dtype=object)
        with open(os.path.join(self.args.out_dir, base + TIERS_SUFFIX), "wt") as o:
            o.write("".join(kinds[inv].tolist()))
        cols = r.tier_cols[s]
        row = [base]
        for j, t in enumerate(range(k, self.min_pickers - 1, -1)):
            picks = int((tier == t).sum())
            row += [str(int(cols[j]) if j < len(cols) else 0), str(picks)]
            self.stats[f"picks_tier_{t}"] += picks
        self.tier_rows.append("\t".join(row) + "\n")
        return int(cols.sum())

    def raise_for(self, mg, ch):
        if mg is self._empty:
            raise AssertionError("Error - vertices are assigned to multiple cliques")
        gc._Run.raise_for(mg, ch)
