"""ctypes binding of ``librepic_gc.so`` (C-ABI declared in ``include/repic_gc.h``).

The library is built in-tree by ``repic-copy_amd/csrc/Makefile`` (``__graft_entry__.build``).
Importing this module without the built library raises ImportError: there is no CPU
fallback for the hot path.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# REPIC_GC_LIB selects the diagnostic build (librepic_gc_diag.so) for tools/phase_stamps.py
LIB_PATH = os.environ.get("REPIC_GC_LIB") or os.path.join(_HERE, "librepic_gc.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C repic-copy_amd/csrc` "
        "(or __graft_entry__.build()); the get_cliques hot path has no CPU fallback")

lib = C.CDLL(LIB_PATH)

F_GET_CC, F_MULTI_OUT, F_DEVICE_INPUTS, F_HOST_OUTPUTS, F_TIMING = 1, 2, 4, 8, 16
F_MEMBERS, F_NO_FUSED, F_DEVICE_META, F_EDGES = 32, 64, 128, 256
F_LAZY_STATS = 512   # ABI 6: per-micrograph outputs fetched on first use (rgc_fetch_stats)
F_JI_THRESHOLD = 1024   # ABI 11: BatchIn.ji_threshold holds the Jaccard threshold (else 0.3)
JI_DEFAULT = 0.3   # the reference's threshold (get_cliques.py:138)
OK, NO_EDGES, NO_CLIQUES = 0, 1, 2
PARSE_OK, PARSE_INDEX, PARSE_VALUE, PARSE_ASSERT, PARSE_FALLBACK, PARSE_OSERROR = range(6)
MAX_K = 8
MEMBERS_SUFFIX = "_members.tsv"

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_f32p = C.POINTER(C.c_float)
_u8p = C.POINTER(C.c_uint8)


class BatchIn(C.Structure):
    _fields_ = [("n_mg", C.c_int32), ("k", C.c_int32), ("box_size", C.c_int64),
                ("flags", C.c_uint32), ("box_off", C.c_void_p), ("id_base", C.c_void_p),
                ("x", C.c_void_p), ("y", C.c_void_p), ("score", C.c_void_p),
                ("dev_box_off", C.c_void_p), ("dev_id_base", C.c_void_p),
                ("ji_threshold", C.c_double)]


class BatchOut(C.Structure):
    _fields_ = [("n_boxes", C.c_int64), ("n_edges", C.c_int64), ("n_cliques", C.c_int64),
                ("status", _i32p), ("cc_max", _i32p), ("cc_cnt", _i32p), ("n_nodes", _i32p),
                ("n_vert", _i32p), ("n_edges_mg", _i64p), ("clique_base", _i64p),
                ("clique_cnt", _i64p),
                ("rows", C.c_void_p), ("w", C.c_void_p), ("conf", C.c_void_p),
                ("consensus", C.c_void_p), ("members", C.c_void_p), ("order", C.c_void_p)]


class Parsed(C.Structure):
    _fields_ = [("n_files", C.c_int64), ("status", _i32p), ("off", _i64p), ("x", _f64p),
                ("y", _f64p), ("score", _f64p), ("sigmoid", _u8p)]


class PickleFmt(C.Structure):
    _fields_ = [("arr_mod", C.c_char_p), ("arr_fn", C.c_char_p), ("dtype_mod", C.c_char_p),
                ("dtype_cls", C.c_char_p), ("coo_mod", C.c_char_p), ("coo_cls", C.c_char_p),
                ("maxprint", C.c_int32)]


class WriteIn(C.Structure):
    _fields_ = [("out_dir", C.c_char_p), ("n_mg", C.c_int32), ("k", C.c_int32),
                ("bases", C.POINTER(C.c_char_p)), ("clique_off", C.c_void_p),
                ("n_vert", C.c_void_p), ("cc_max", C.c_void_p), ("cc_cnt", C.c_void_p),
                ("seconds", C.c_void_p), ("w", C.c_void_p), ("conf", C.c_void_p),
                ("rows", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p),
                ("cid", C.c_void_p)]


class ConsensusOpts(C.Structure):
    _fields_ = [("node_limit", C.c_int64), ("num_particles", C.c_int64), ("flags", C.c_uint32)]


class ConsensusOut(C.Structure):
    _fields_ = [("run", BatchOut), ("n_picked", C.c_int64), ("pick_off", _i64p),
                ("px", _f64p), ("py", _f64p), ("pconf", _f32p), ("pcol", _i32p),
                ("sel_cnt", _i32p), ("ilp_status", _i32p), ("ilp_gap", _f64p),
                ("h2d_bytes", C.c_int64), ("d2h_bytes", C.c_int64)]


class PickIn(C.Structure):
    _fields_ = [("n_mg", C.c_int32), ("col_off", C.c_void_p), ("x", C.c_void_p),
                ("conf", C.c_void_p), ("cx", C.c_void_p), ("cy", C.c_void_p),
                ("num_particles", C.c_int64)]


class PickOut(C.Structure):
    _fields_ = [("n_picked", C.c_int64), ("pick_off", _i64p), ("px", _f64p), ("py", _f64p),
                ("pconf", _f32p), ("pcol", _i32p)]


class BoxWriteIn(C.Structure):
    _fields_ = [("out_dir", C.c_char_p), ("n_mg", C.c_int32), ("box_size", C.c_int64),
                ("bases", C.POINTER(C.c_char_p)), ("pick_off", C.c_void_p),
                ("count", C.c_void_p), ("px", C.c_void_p), ("py", C.c_void_p),
                ("pconf", C.c_void_p)]


class MembersOut(C.Structure):
    _fields_ = [("pmx", _f64p), ("pmy", _f64p), ("left_off", _i64p), ("left_x", _f64p),
                ("left_y", _f64p), ("in_clique", _i32p)]


class PickMembersIn(C.Structure):
    _fields_ = [("n_mg", C.c_int32), ("k", C.c_int32), ("col_off", C.c_void_p),
                ("x", C.c_void_p), ("conf", C.c_void_p), ("cons", C.c_void_p),
                ("members", C.c_void_p), ("box_off", C.c_void_p), ("bx", C.c_void_p),
                ("by", C.c_void_p), ("num_particles", C.c_int64)]


class MembersWriteIn(C.Structure):
    _fields_ = [("box", BoxWriteIn), ("k", C.c_int32), ("header", C.c_char_p),
                ("pmx", C.c_void_p), ("pmy", C.c_void_p), ("seg", C.c_void_p),
                ("left_off", C.c_void_p), ("left_x", C.c_void_p), ("left_y", C.c_void_p)]


MEMBERS_SYMBOLS = ("rgc_consensus_members", "rgc_pick_members", "rgc_write_members")


def has_members() -> bool:
    """The loaded library has the ``consensus --members`` entry points (additive symbols: the
    ABI version does not tell)."""
    return all(hasattr(lib, n) for n in MEMBERS_SYMBOLS)


if has_members():
    lib.rgc_consensus_members.argtypes = [C.c_void_p, C.POINTER(BatchIn),
                                          C.POINTER(ConsensusOpts), C.POINTER(ConsensusOut),
                                          C.POINTER(MembersOut)]
    lib.rgc_pick_members.argtypes = [C.c_void_p, C.POINTER(PickMembersIn), C.POINTER(PickOut),
                                     C.POINTER(MembersOut)]
    lib.rgc_write_members.argtypes = [C.POINTER(MembersWriteIn), C.c_int, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int32)]

class NmsIn(C.Structure):
    _fields_ = [("n_seg", C.c_int64), ("seg_off", C.c_void_p), ("x", C.c_void_p),
                ("y", C.c_void_p), ("box_size", C.c_int64), ("ji_threshold", C.c_double),
                ("flags", C.c_uint32)]


NMS_SYMBOLS = ("rgc_nms", "rgc_nms_last_bytes")


def has_nms() -> bool:
    """The loaded library has the greedy-NMS entry points (additive symbols: the ABI version
    does not tell)."""
    return all(hasattr(lib, n) for n in NMS_SYMBOLS)


if has_nms():
    lib.rgc_nms.argtypes = [C.c_void_p, C.POINTER(NmsIn), C.c_void_p, C.c_void_p]
    lib.rgc_nms_last_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]

F_PARTNERS = 2048   # rgc_agreement: also return partner / partner_ji


class AgreeIn(C.Structure):
    _fields_ = [("n_mg", C.c_int32), ("k", C.c_int32), ("box_size", C.c_int64),
                ("ji_threshold", C.c_double), ("flags", C.c_uint32), ("box_off", C.c_void_p),
                ("x", C.c_void_p), ("y", C.c_void_p)]


class AgreeOut(C.Structure):
    _fields_ = [("support", _u8p), ("partner", _i32p), ("partner_ji", _f64p),
                ("pair_edges", _i64p), ("pair_supported", _i64p), ("pair_mutual", _i64p)]


AGREE_SYMBOLS = ("rgc_agreement", "rgc_agreement_last_bytes")


def has_agreement() -> bool:
    """The loaded library has the picker-agreement entry points (additive symbols: the ABI
    version does not tell)."""
    return all(hasattr(lib, n) for n in AGREE_SYMBOLS)


if has_agreement():
    lib.rgc_agreement.argtypes = [C.c_void_p, C.POINTER(AgreeIn), C.POINTER(AgreeOut)]
    lib.rgc_agreement_last_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64),
                                             C.POINTER(C.c_int64)]


class TiersOut(C.Structure):
    _fields_ = [("n_tiers", C.c_int32), ("ptier", _i32p), ("pmask", _i32p), ("pw", _f32p),
                ("pmember", _i32p), ("box_tier", _i32p), ("tier_cols", _i64p),
                ("tier_picks", _i64p)]


class VoteGatherIn(C.Structure):
    _fields_ = [("n_mg", C.c_int32), ("k", C.c_int32), ("t", C.c_int32),
                ("pick_tier", C.c_int32), ("box_size", C.c_int64), ("ji_threshold", C.c_double),
                ("box_off", C.c_void_p), ("x", C.c_void_p), ("y", C.c_void_p),
                ("score", C.c_void_p), ("pick_off", C.c_void_p), ("pcx", C.c_void_p),
                ("pcy", C.c_void_p), ("box_tier_in", C.c_void_p)]


class VoteGatherOut(C.Structure):
    _fields_ = [("n_sub", C.c_int32), ("sub_mg", _i32p), ("sub_mask", _i32p),
                ("box_off", _i64p), ("box_tier", _i32p), ("origin", _i32p), ("x", _f64p),
                ("y", _f64p), ("score", _f64p)]


TIERS_SYMBOLS = ("rgc_consensus_tiers", "rgc_vote_gather")
TIERS_SUFFIX = "_tiers.tsv"


def has_tiers() -> bool:
    """The loaded library has the ``consensus --min_pickers`` entry points (additive symbols:
    the ABI version does not tell)."""
    return all(hasattr(lib, n) for n in TIERS_SYMBOLS)


if has_tiers():
    lib.rgc_consensus_tiers.argtypes = [C.c_void_p, C.POINTER(BatchIn), C.POINTER(ConsensusOpts),
                                        C.c_int, C.POINTER(ConsensusOut), C.POINTER(TiersOut)]
    lib.rgc_vote_gather.argtypes = [C.c_void_p, C.POINTER(VoteGatherIn),
                                    C.POINTER(VoteGatherOut)]

lib.rgc_abi_version.restype = C.c_int
lib.rgc_consensus.argtypes = [C.c_void_p, C.POINTER(BatchIn), C.POINTER(ConsensusOpts),
                              C.POINTER(ConsensusOut)]
lib.rgc_pick_select.argtypes = [C.c_void_p, C.POINTER(PickIn), C.POINTER(PickOut)]
lib.rgc_write_boxes.argtypes = [C.POINTER(BoxWriteIn), C.c_int, C.POINTER(C.c_int64)]
lib.rgc_np_float_str.argtypes = [C.c_float, C.c_char_p, C.c_int]
lib.rgc_last_error.restype = C.c_char_p
lib.rgc_device_count.argtypes = [C.POINTER(C.c_int)]
lib.rgc_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
lib.rgc_ctx_destroy.argtypes = [C.c_void_p]
lib.rgc_ctx_set_copy_stream.argtypes = [C.c_void_p, C.c_void_p]
lib.rgc_ctx_destroy.restype = None
lib.rgc_run.argtypes = [C.c_void_p, C.POINTER(BatchIn), C.POINTER(BatchOut)]
lib.rgc_submit.argtypes = [C.c_void_p, C.POINTER(BatchIn)]
lib.rgc_wait.argtypes = [C.c_void_p, C.POINTER(BatchOut)]
lib.rgc_fetch_stats.argtypes = [C.c_void_p]
lib.rgc_detach_host.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
lib.rgc_host_block_free.argtypes = [C.c_void_p]
lib.rgc_host_block_free.restype = None
lib.rgc_last_edges.argtypes = [C.c_void_p, C.POINTER(_i32p), C.POINTER(_i32p),
                               C.POINTER(_f64p)]
lib.rgc_last_edges.restype = C.c_int64
lib.rgc_kernel_times.argtypes = [C.c_void_p, C.c_int, _f32p, C.POINTER(C.c_char_p)]
lib.rgc_parse_files.argtypes = [C.POINTER(C.c_char_p), C.c_int64, C.c_int,
                                C.POINTER(C.POINTER(Parsed))]
lib.rgc_parsed_free.argtypes = [C.POINTER(Parsed)]
lib.rgc_parsed_free.restype = None
lib.rgc_py_hash_node.argtypes = [C.c_double, C.c_double, C.c_int64]
lib.rgc_py_hash_node.restype = C.c_uint64
lib.rgc_py_set_order.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_int8)]
lib.rgc_test_epilogue.argtypes = [C.c_int, _f64p, _f64p, _f64p, C.POINTER(C.c_int64), _f64p,
                                  C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int),
                                  C.POINTER(C.c_int8), _f32p, _f32p]

lib.rgc_write_outputs.argtypes = [C.POINTER(PickleFmt), C.POINTER(WriteIn), C.c_int,
                                  C.POINTER(C.c_int64)]
lib.rgc_pickle_bytes.argtypes = [C.POINTER(PickleFmt), C.POINTER(WriteIn), C.c_int, C.c_int,
                                 C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
lib.rgc_py_float_repr.argtypes = [C.c_double, C.c_char_p, C.c_int]
lib.rgc_test_ji_cutoff.argtypes = [C.c_int64, C.c_double, C.POINTER(C.c_int64), _f64p, _f64p]

EXPORTS = ["rgc_abi_version", "rgc_last_error", "rgc_device_count", "rgc_ctx_create",
           "rgc_ctx_destroy", "rgc_ctx_set_copy_stream", "rgc_run", "rgc_submit", "rgc_wait", "rgc_fetch_stats", "rgc_detach_host", "rgc_host_block_free", "rgc_kernel_times", "rgc_last_edges", "rgc_parse_files",
           "rgc_parsed_free", "rgc_py_hash_node", "rgc_py_set_order", "rgc_test_epilogue",
           "rgc_score_pairs", "rgc_score_sweep", "rgc_score_match", "rgc_score_match_sweep", "rgc_test_iou_edge", "rgc_ilp_solve", "rgc_write_outputs", "rgc_pickle_bytes",
           "rgc_py_float_repr", "rgc_consensus", "rgc_pick_select", "rgc_write_boxes",
           "rgc_np_float_str", "rgc_test_ji_cutoff", *MEMBERS_SYMBOLS, *NMS_SYMBOLS,
           *TIERS_SYMBOLS, *AGREE_SYMBOLS]


class RGCError(RuntimeError):
    pass


def _check(rc):
    if rc < 0:
        raise RGCError(lib.rgc_last_error().decode(errors="replace"))
    return rc


def abi_version() -> int:
    return lib.rgc_abi_version()


def ilp_big_max() -> int:
    """Largest conflict component (cliques) the run_ilp branch and bound searches
    (rgc_ilp.hip ILP_BIG); larger ones are certified, not searched."""
    return 4096


def check_ji_threshold(t) -> float:
    """``t`` as the Jaccard threshold the library accepts (finite, 0 <= t < 1), else ValueError."""
    t = float(t)
    if not (0.0 <= t < 1.0):   # (false for nan)
        raise ValueError(f"ji_threshold must be finite and in [0, 1), got {t!r}")
    return t


def ji_cutoff(box_size: int, t: float):
    """Test hook (rgc_test_ji_cutoff): (int_cut, f64_lo, f64_hi) the launches pass for
    ``box_size`` and threshold ``t``: an edge is I > int_cut on the integer layout and
    I > f64_hi on the f64 layout (f64_lo == f64_hi: no band of undecided areas)."""
    ic, lo, hi = C.c_int64(0), C.c_double(0), C.c_double(0)
    _check(lib.rgc_test_ji_cutoff(int(box_size), float(t), C.byref(ic), C.byref(lo), C.byref(hi)))
    return ic.value, lo.value, hi.value


# ----------------------------------------------------------------------------- parsing
def parse_files(paths, n_threads=None):
    """Parse BOX files with the C++ parser -> (status[n], off[n+1], x, y, score, sigmoid)."""
    n = len(paths)
    arr = (C.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
    out = C.POINTER(Parsed)()
    if n_threads is None:
        n_threads = min(16, os.cpu_count() or 1)
    _check(lib.rgc_parse_files(arr, n, int(n_threads), C.byref(out)))
    # the library-owned x / y / score arrays are handed out without a copy: each numpy view's
    # base is a ctypes array holding the owner, which frees them when the last view is gone
    owner = _ParsedOwner(out)
    P = out.contents
    status = np.ctypeslib.as_array(P.status, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    off = np.ctypeslib.as_array(P.off, shape=(n + 1,)).copy()
    tot = int(off[-1])
    if tot:
        x, y, s = (owner.view(p, tot) for p in (P.x, P.y, P.score))
    else:
        x = y = s = np.zeros(0, np.float64)
    sig = (np.ctypeslib.as_array(P.sigmoid, shape=(n,)).astype(bool) if n
           else np.zeros(0, bool))
    return status, off, x, y, s, sig


class _ParsedOwner:
    """Frees an rgc_parsed once no numpy view of its arrays is left."""

    def __init__(self, ptr):
        self.ptr = ptr

    def view(self, p, n):
        ca = (C.c_double * n).from_address(C.cast(p, C.c_void_p).value)
        ca._owner = self
        return np.frombuffer(ca, dtype=np.float64)

    def __del__(self):
        try:
            lib.rgc_parsed_free(self.ptr)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


# ----------------------------------------------------------------------------- CPython set order
def py_hash_node(x: float, y: float, node_id: int) -> int:
    return int(lib.rgc_py_hash_node(x, y, node_id))


def py_set_order(hashes):
    n = len(hashes)
    h = (C.c_uint64 * max(n, 1))(*[int(v) & 0xFFFFFFFFFFFFFFFF for v in hashes])
    o = (C.c_int8 * max(n, 1))()
    _check(lib.rgc_py_set_order(h, n, o))
    return [o[i] for i in range(n)]


def test_epilogue(x, y, score, ids, ji, set_order=True, ins=None):
    """The device ILP epilogue of one clique, run on the host (test hook):
    -> (consensus member index, node-iteration order, w, conf)."""
    k = len(x)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    xa, ya, sa, ja = f(x), f(y), f(score), f(np.asarray(ji).reshape(k * k))
    ia = np.ascontiguousarray(ids, dtype=np.int64)
    insa = None if ins is None else (C.c_uint64 * k)(*[int(v) for v in ins])
    arg = C.c_int(0)
    ordr = (C.c_int8 * k)()
    w, conf = C.c_float(0), C.c_float(0)
    p64 = lambda a: a.ctypes.data_as(_f64p)  # noqa: E731
    _check(lib.rgc_test_epilogue(k, p64(xa), p64(ya), p64(sa),
                                 ia.ctypes.data_as(C.POINTER(C.c_int64)), p64(ja),
                                 int(set_order), insa, C.byref(arg), ordr, C.byref(w),
                                 C.byref(conf)))
    return arg.value, [ordr[i] for i in range(k)], np.float32(w.value), np.float32(conf.value)


# ----------------------------------------------------------------------------- device context
def device_count() -> int:
    n = C.c_int(0)
    _check(lib.rgc_device_count(C.byref(n)))
    return n.value


class _HostLease:
    """Owner of one run's host output buffers.  Every numpy view a :class:`Result` hands out
    keeps it alive.  While the context still owns the buffers (``block`` None) nothing is
    done; once the context moves on (next run, ILP / score call, close) while this lease is
    still referenced, the context detaches the buffers into ``block`` (rgc_detach_host, ABI 7)
    and they are freed here when the last view is gone."""

    __slots__ = ("block", "__weakref__")

    def __init__(self):
        self.block = None

    def view(self, p, ct, n):
        """numpy view of n elements of ctypes type ct at address p, owned by this lease"""
        ca = (ct * n).from_address(p)
        ca._owner = self
        return np.ctypeslib.as_array(ca)

    def __del__(self):
        if self.block:
            try:
                lib.rgc_host_block_free(self.block)
            except Exception:  # noqa: BLE001 - interpreter shutdown
                pass


class Context:
    """One device + stream; owns the device workspace arena (grow-only)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._p = C.c_void_p()
        _check(lib.rgc_ctx_create(int(device), C.c_void_p(stream or 0), C.byref(self._p)))
        self.device = device
        self._pending = None
        self._lease = None   # weakref to the _HostLease of the last Result
        # (H2D, D2H) bytes of the last nms / agreement call
        self.nms_bytes = self.agreement_bytes = (0, 0)

    def set_copy_stream(self, stream: int):
        """Stream of the per-micrograph stats copy of non-lazy submits (0: the null stream);
        by default all contexts share one copy stream per device (rgc_ctx_set_copy_stream)."""
        _check(lib.rgc_ctx_set_copy_stream(self._p, C.c_void_p(stream or 0)))

    def _retire(self):
        """Before anything that may reuse or free the context's host buffers: if the last
        Result (or any array taken from it) is still referenced, hand its buffers over to it."""
        ref = self._lease
        lease = ref() if ref is not None else None
        if lease is not None and lease.block is None and self._p:
            h = C.c_void_p()
            # (the lease is dropped only once the hand-over succeeded: after a failed detach
            # the next retire, or close(), tries again)
            _check(lib.rgc_detach_host(self._p, C.byref(h)))
            lease.block = h.value
        self._lease = None

    def _result(self, bo, n_mg, k, flags, lazy_ctx=None):
        lease = _HostLease()
        self._lease = weakref.ref(lease)
        return Result(bo, n_mg, k, flags, lazy_ctx, lease)

    def close(self):
        if self._p:
            if self._pending is None:
                self._retire()
            lib.rgc_ctx_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def run(self, n_mg, k, box_size, box_off, id_base, x, y, score, flags=F_HOST_OUTPUTS,
            dev_meta=None, ji_threshold=None):
        """Run the batched pipeline.  ``box_off``/``id_base`` are host int64 arrays;
        ``x``/``y``/``score`` are host float64 arrays, or device pointers (ints) with
        ``F_DEVICE_INPUTS``.  ``dev_meta`` = (device pointer of box_off as int32, device
        pointer of id_base) sets ``F_DEVICE_META``: the offsets are not uploaded per run.
        ``ji_threshold`` (None: the reference's 0.3) joins two boxes when their JI exceeds it
        (``F_JI_THRESHOLD``; finite, 0 <= t < 1).
        Returns a :class:`Result`; its host arrays stay valid as long as they are referenced
        (rgc_detach_host hands them over when the context moves on)."""
        bi, keep, flags = self._batch_in(n_mg, k, box_size, box_off, id_base, x, y, score, flags,
                                         dev_meta, ji_threshold)
        self._retire()
        bo = BatchOut()
        _check(lib.rgc_run(self._p, C.byref(bi), C.byref(bo)))
        del keep
        return self._result(bo, n_mg, k, flags)

    def submit(self, n_mg, k, box_size, box_off, id_base, x, y, score, flags=F_HOST_OUTPUTS,
               dev_meta=None, ji_threshold=None):
        """``run`` without waiting (rgc_submit): the batch is enqueued on the context's stream
        and :meth:`wait` returns its :class:`Result`.  One submission in flight per context;
        two contexts overlap the host side of batch i+1 with the device work of batch i, and on
        two streams also the two batches' kernels (bench.py's default).  A batch that needs the
        general path (large micrographs) runs on the context's worker thread until ``wait``.
        The arrays passed in must stay alive until ``wait`` (kept here)."""
        bi, keep, flags = self._batch_in(n_mg, k, box_size, box_off, id_base, x, y, score, flags,
                                         dev_meta, ji_threshold)
        self._retire()
        _check(lib.rgc_submit(self._p, C.byref(bi)))
        self._pending = (keep, n_mg, k, flags)

    def wait(self):
        if self._pending is None:
            raise RGCError("rgc_wait: no submission in flight on this context")
        bo = BatchOut()
        keep, n_mg, k, flags = self._pending
        self._pending = None
        _check(lib.rgc_wait(self._p, C.byref(bo)))
        del keep
        return self._result(bo, n_mg, k, flags, self)

    def _batch_in(self, n_mg, k, box_size, box_off, id_base, x, y, score, flags, dev_meta,
                  ji_threshold=None):
        # (kept lean: this runs once per batch inside the bench's timed region)
        if not (type(box_off) is np.ndarray and box_off.dtype == np.int64
                and box_off.flags.c_contiguous):
            box_off = np.ascontiguousarray(box_off, dtype=np.int64)
        if not (type(id_base) is np.ndarray and id_base.dtype == np.int64
                and id_base.flags.c_contiguous):
            id_base = np.ascontiguousarray(id_base, dtype=np.int64)
        assert box_off.shape == (n_mg * k + 1,) and id_base.shape == (n_mg,)
        keep = [box_off, id_base]
        if flags & F_DEVICE_INPUTS:
            px, py, ps = int(x), int(y), int(score)
        else:
            x, y, score = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, score))
            n = int(box_off[-1]) if len(box_off) else 0
            assert x.shape == y.shape == score.shape == (n,)
            keep += [x, y, score]
            px, py, ps = x.ctypes.data, y.ctypes.data, score.ctypes.data
        dbo = did = None
        if dev_meta is not None:
            flags |= F_DEVICE_META
            dbo, did = int(dev_meta[0]), int(dev_meta[1])
        bi = BatchIn(n_mg, k, int(box_size), flags, box_off.ctypes.data, id_base.ctypes.data,
                     px, py, ps, dbo, did)
        if ji_threshold is not None:   # (the library validates it: RGCError before any launch)
            flags |= F_JI_THRESHOLD
            bi.flags = flags
            bi.ji_threshold = float(ji_threshold)
        return bi, keep, flags

    def consensus(self, n_mg, k, box_size, box_off, id_base, x, y, score, flags=0,
                  dev_meta=None, node_limit=0, num_particles=None, timing=False,
                  ji_threshold=None, members=False):
        """get_cliques + run_ilp in one device pass (rgc_consensus, ABI 10): ``run``'s
        arguments, then the solver's ``node_limit`` and run_ilp's ``num_particles`` (None:
        all).  The per-clique arrays stay in HBM unless ``flags`` has ``F_HOST_OUTPUTS``.
        ``ji_threshold`` as for ``run``.  ``members``: rgc_consensus_members instead, the run
        with ``F_MEMBERS``; the result also has ``pmx``, ``pmy``, ``left_off``, ``left_x``,
        ``left_y`` and ``in_clique``.
        Returns a :class:`ConsensusResult` (plain copies of the pick arrays)."""
        bi, keep, flags = self._batch_in(n_mg, k, box_size, box_off, id_base, x, y, score, flags,
                                         dev_meta, ji_threshold)
        self._retire()
        opts = ConsensusOpts(int(node_limit), -1 if num_particles is None else int(num_particles),
                             F_TIMING if timing else 0)
        co = ConsensusOut()
        mo = None
        if members:
            _need_members()
            mo = MembersOut()
            flags |= F_MEMBERS
            _check(lib.rgc_consensus_members(self._p, C.byref(bi), C.byref(opts), C.byref(co),
                                             C.byref(mo)))
        else:
            _check(lib.rgc_consensus(self._p, C.byref(bi), C.byref(opts), C.byref(co)))
        del keep
        return ConsensusResult(co, self._result(co.run, n_mg, k, flags), n_mg, mo, k)

    def consensus_tiers(self, n_mg, k, box_size, box_off, id_base, x, y, score, min_pickers,
                        flags=0, dev_meta=None, node_limit=0, num_particles=None, timing=False,
                        ji_threshold=None):
        """``consensus`` with tiers k, k-1, .., ``min_pickers`` (rgc_consensus_tiers): each lower
        tier packs the cliques of every subset of t pickers among the boxes the picks of the
        tiers above leave unexplained.  The :class:`ConsensusResult` holds every tier's picks
        (per micrograph tier descending, then the tier's order) and also ``ptier``, ``pmask``
        (picker bitmask), ``pw``, ``pmember`` [n_picked, k] (batch box index or -1),
        ``box_tier`` [n_boxes], ``tier_cols`` and ``tier_picks`` [n_mg, k - min_pickers + 1]
        (column j: tier k - j)."""
        _need_tiers()
        bi, keep, flags = self._batch_in(n_mg, k, box_size, box_off, id_base, x, y, score, flags,
                                         dev_meta, ji_threshold)
        self._retire()
        opts = ConsensusOpts(int(node_limit), -1 if num_particles is None else int(num_particles),
                             F_TIMING if timing else 0)
        co, to = ConsensusOut(), TiersOut()
        _check(lib.rgc_consensus_tiers(self._p, C.byref(bi), C.byref(opts), int(min_pickers),
                                       C.byref(co), C.byref(to)))
        n_boxes = int(keep[0][-1]) if len(keep[0]) else 0
        del keep
        # (the run's per-clique arrays are not handed out: the lower tiers reuse them)
        r = ConsensusResult(co, self._result(co.run, n_mg, k, flags & ~F_HOST_OUTPUTS), n_mg)
        n, nt = r.n_picked, int(to.n_tiers)
        r.ptier = _copy(to.ptier, n, np.int32)
        r.pmask = _copy(to.pmask, n, np.int32)
        r.pw = _copy(to.pw, n, np.float32)
        r.pmember = _copy(to.pmember, n * k, np.int32).reshape(n, k)
        r.box_tier = _copy(to.box_tier, n_boxes, np.int32)
        r.tier_cols = _copy(to.tier_cols, n_mg * nt, np.int64).reshape(n_mg, nt)
        r.tier_picks = _copy(to.tier_picks, n_mg * nt, np.int64).reshape(n_mg, nt)
        return r

    def vote_gather(self, k, t, box_size, ji_threshold, box_off, x, y, score, pick_off, pcx, pcy,
                    pick_tier=None, box_tier=None):
        """Test hook of the explain / count / gather kernels (rgc_vote_gather): the picks of
        micrograph m (``pick_off[m]:pick_off[m+1]`` of ``pcx`` / ``pcy``, unrounded) mark the
        boxes they explain with ``pick_tier`` (default t + 1), starting from ``box_tier`` (None:
        all 0); the boxes still at 0 then form the pseudo-batch of tier ``t`` -> (box_tier,
        sub_mg, sub_mask, box_off', origin, x', y', score') copies."""
        _need_tiers()
        box_off = np.ascontiguousarray(box_off, np.int64)
        pick_off = np.ascontiguousarray(pick_off, np.int64)
        x, y, score, pcx, pcy = (np.ascontiguousarray(v, np.float64)
                                 for v in (x, y, score, pcx, pcy))
        n_mg = len(pick_off) - 1
        n = int(box_off[-1])
        assert n_mg >= 0 and len(box_off) == n_mg * k + 1
        assert x.shape == y.shape == score.shape == (n,)
        assert pcx.shape == pcy.shape == (int(pick_off[-1]),)
        bt = None
        if box_tier is not None:
            bt = np.ascontiguousarray(box_tier, np.int32)
            assert bt.shape == (n,)
        gi = VoteGatherIn(n_mg, int(k), int(t), int(t + 1 if pick_tier is None else pick_tier),
                          int(box_size), float(ji_threshold), box_off.ctypes.data, x.ctypes.data,
                          y.ctypes.data, score.ctypes.data, pick_off.ctypes.data,
                          pcx.ctypes.data, pcy.ctypes.data, None if bt is None else bt.ctypes.data)
        go = VoteGatherOut()
        self._retire()
        _check(lib.rgc_vote_gather(self._p, C.byref(gi), C.byref(go)))
        nq = int(go.n_sub)
        boff = _copy(go.box_off, nq * t + 1, np.int64)
        npb = int(boff[-1])
        return (_copy(go.box_tier, n, np.int32), _copy(go.sub_mg, nq, np.int32),
                _copy(go.sub_mask, nq, np.int32), boff, _copy(go.origin, npb, np.int32),
                _copy(go.x, npb, np.float64), _copy(go.y, npb, np.float64),
                _copy(go.score, npb, np.float64))

    def pick_members(self, k, col_off, x, conf, cons, members, box_off, bx, by,
                     num_particles=None):
        """Test hook of the members kernels (rgc_pick_members): ``pick_select`` on columns whose
        consensus coordinates are those of box ``cons[c]``, then the members of every written
        pick and each (micrograph, picker) segment's leftovers -> (pick_off, px, py, pconf,
        pcol, pmx, pmy, left_off, left_x, left_y, in_clique) copies; ``pmx`` / ``pmy`` are
        [n_picked, k]."""
        _need_members()
        col_off = np.ascontiguousarray(col_off, np.int64)
        box_off = np.ascontiguousarray(box_off, np.int64)
        x = np.ascontiguousarray(x, np.uint8)
        conf = np.ascontiguousarray(conf, np.float32)
        cons = np.ascontiguousarray(cons, np.int32)
        members = np.ascontiguousarray(members, np.int32)
        bx = np.ascontiguousarray(bx, np.float64)
        by = np.ascontiguousarray(by, np.float64)
        n_mg = len(col_off) - 1
        nc = int(col_off[-1]) if n_mg >= 0 else 0
        assert n_mg >= 0 and len(x) == len(conf) == len(cons) == nc and members.size == nc * k
        assert len(box_off) == n_mg * k + 1 and len(bx) == len(by) >= int(box_off[-1])
        pi = PickMembersIn(n_mg, int(k), col_off.ctypes.data, x.ctypes.data, conf.ctypes.data,
                           cons.ctypes.data, members.ctypes.data, box_off.ctypes.data,
                           bx.ctypes.data, by.ctypes.data,
                           -1 if num_particles is None else int(num_particles))
        po, mo = PickOut(), MembersOut()
        self._retire()
        _check(lib.rgc_pick_members(self._p, C.byref(pi), C.byref(po), C.byref(mo)))
        n = int(po.n_picked)
        S = n_mg * k
        left_off = _copy(mo.left_off, S + 1, np.int64)
        L = int(left_off[-1])
        return (_copy(po.pick_off, n_mg + 1, np.int64), _copy(po.px, n, np.float64),
                _copy(po.py, n, np.float64), _copy(po.pconf, n, np.float32),
                _copy(po.pcol, n, np.int32), _copy(mo.pmx, n * k, np.float64).reshape(n, k),
                _copy(mo.pmy, n * k, np.float64).reshape(n, k), left_off,
                _copy(mo.left_x, L, np.float64), _copy(mo.left_y, L, np.float64),
                _copy(mo.in_clique, S, np.int32))

    def pick_select(self, col_off, x, conf, cx, cy, num_particles=None):
        """Test hook of the emit kernels (rgc_pick_select): per micrograph (columns
        ``col_off[m]:col_off[m+1]``) the columns with x == 1 by confidence descending, equal
        confidences in column order -> (pick_off, px, py, pconf, pcol) copies."""
        col_off = np.ascontiguousarray(col_off, np.int64)
        x = np.ascontiguousarray(x, np.uint8)
        conf = np.ascontiguousarray(conf, np.float32)
        cx = np.ascontiguousarray(cx, np.float64)
        cy = np.ascontiguousarray(cy, np.float64)
        n_mg = len(col_off) - 1
        nc = int(col_off[-1])
        assert n_mg >= 0 and len(x) == len(conf) == len(cx) == len(cy) == nc
        pi = PickIn(n_mg, col_off.ctypes.data, x.ctypes.data, conf.ctypes.data, cx.ctypes.data,
                    cy.ctypes.data, -1 if num_particles is None else int(num_particles))
        po = PickOut()
        self._retire()
        _check(lib.rgc_pick_select(self._p, C.byref(pi), C.byref(po)))
        n = int(po.n_picked)
        return (_copy(po.pick_off, n_mg + 1, np.int64), _copy(po.px, n, np.float64),
                _copy(po.py, n, np.float64), _copy(po.pconf, n, np.float32),
                _copy(po.pcol, n, np.int32))

    def nms(self, seg_off, x, y, box_size, ji_threshold, timing=False):
        """Greedy non-maximum suppression (rgc_nms): segment s holds the boxes
        ``seg_off[s]:seg_off[s+1]`` of ``x`` / ``y`` (lower-left corners of squares of side
        ``box_size``) in priority order; a box is kept iff no kept box before it in its segment
        has a Jaccard index with it above ``ji_threshold`` (the reference's f64 quotient, strict).
        -> (keep uint8[n], kept int64[n_seg]).  ``nms_bytes`` then holds the (H2D, D2H) bytes
        the call copied.  The context's host buffers are not touched: a Result stays valid."""
        _need_nms()
        seg_off = np.ascontiguousarray(seg_off, np.int64)
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        n_seg = len(seg_off) - 1
        assert seg_off.ndim == 1 and n_seg >= 0
        n = int(seg_off[-1])
        assert x.shape == y.shape == (n,)
        keep = np.zeros(n, np.uint8)
        kept = np.zeros(n_seg, np.int64)
        ni = NmsIn(n_seg, seg_off.ctypes.data, x.ctypes.data, y.ctypes.data, int(box_size),
                   float(ji_threshold), F_TIMING if timing else 0)
        _check(lib.rgc_nms(self._p, C.byref(ni), keep.ctypes.data, kept.ctypes.data))
        h2d, d2h = C.c_int64(0), C.c_int64(0)
        _check(lib.rgc_nms_last_bytes(self._p, C.byref(h2d), C.byref(d2h)))
        self.nms_bytes = (h2d.value, d2h.value)
        return keep, kept

    def agreement(self, n_mg, k, box_size, box_off, x, y, ji_threshold=None, partners=False,
                  timing=False):
        """Picker agreement of a batch in ``rgc_batch_in``'s layout (rgc_agreement): two boxes
        of one micrograph and different pickers are joined iff ``|dx| <= box_size`` and the
        reference's f64 Jaccard quotient exceeds ``ji_threshold`` (None: the reference's 0.3),
        strictly.  -> :class:`Agreement`; ``partners`` also returns the best partner of every
        box per picker (the only mode in which they leave the device).  ``agreement_bytes`` then
        holds the (H2D, D2H) bytes the call copied.  The context's other host buffers are not
        touched: a Result stays valid."""
        _need_agreement()
        box_off = np.ascontiguousarray(box_off, np.int64)
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(y, np.float64)
        n_mg, k = int(n_mg), int(k)
        # (what the library reads must be there; what it refuses unread is left to it)
        valid = n_mg > 0 and 1 <= k <= MAX_K and n_mg * k <= 2 ** 31 - 1
        assert box_off.ndim == 1 and (not valid or len(box_off) == n_mg * k + 1)
        n = int(box_off[-1]) if valid else 0
        assert x.shape == y.shape and x.ndim == 1 and (n > 2 ** 31 - 1 or len(x) >= n)
        t = JI_DEFAULT if ji_threshold is None else float(ji_threshold)
        flags = (F_TIMING if timing else 0) | (F_PARTNERS if partners else 0)
        ai = AgreeIn(n_mg, k, int(box_size), t, flags, box_off.ctypes.data, x.ctypes.data,
                     y.ctypes.data)
        ao = AgreeOut()
        _check(lib.rgc_agreement(self._p, C.byref(ai), C.byref(ao)))
        h2d, d2h = C.c_int64(0), C.c_int64(0)
        _check(lib.rgc_agreement_last_bytes(self._p, C.byref(h2d), C.byref(d2h)))
        self.agreement_bytes = (h2d.value, d2h.value)
        return Agreement(ao, n_mg, k, n, partners)

    def last_edges(self):
        """Test hook: (u, v, ji) copies of the JI > threshold edges of the last run with F_EDGES
        (batch box indices; order unspecified)."""
        u, v, j = _i32p(), _i32p(), _f64p()
        n = _check(lib.rgc_last_edges(self._p, C.byref(u), C.byref(v), C.byref(j)))
        if n == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
        return (np.ctypeslib.as_array(u, shape=(n,)).copy(),
                np.ctypeslib.as_array(v, shape=(n,)).copy(),
                np.ctypeslib.as_array(j, shape=(n,)).copy())

    def kernel_times(self):
        n = lib.rgc_kernel_times(self._p, 0, None, None)
        ms = (C.c_float * max(n, 1))()
        names = (C.c_char_p * max(n, 1))()
        lib.rgc_kernel_times(self._p, n, ms, names)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]


def _copy(p, n, dt):
    """numpy copy of n elements at ctypes pointer p (empty when n == 0 or p is NULL)."""
    if not n or not p:
        return np.zeros(0, dt)
    return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)


class ConsensusResult:
    """One rgc_consensus call: ``run`` is the :class:`Result` rgc_run would have returned;
    the rest are copies.  Picks of micrograph m: ``pick_off[m]:pick_off[m+1]`` of ``px``,
    ``py`` (np.rint of the consensus coordinates), ``pconf`` and ``pcol`` (the column in the
    micrograph's clique range), in run_ilp's output order.  ``sel_cnt`` counts the chosen
    columns before ``num_particles``; ``ilp_status`` / ``ilp_gap`` are the micrograph's
    certification (repic_amd.ilp.mg_status) and relative gap."""

    def __init__(self, co: ConsensusOut, run, n_mg, mo=None, k=0):
        self.run = run
        self.n_picked = int(co.n_picked)
        self.pick_off = (_copy(co.pick_off, n_mg + 1, np.int64) if n_mg
                         else np.zeros(1, np.int64))
        self.px = _copy(co.px, self.n_picked, np.float64)
        self.py = _copy(co.py, self.n_picked, np.float64)
        self.pconf = _copy(co.pconf, self.n_picked, np.float32)
        self.pcol = _copy(co.pcol, self.n_picked, np.int32)
        self.sel_cnt = _copy(co.sel_cnt, n_mg, np.int32)
        self.ilp_status = _copy(co.ilp_status, n_mg, np.int32)
        self.ilp_gap = _copy(co.ilp_gap, n_mg, np.float64)
        self.h2d_bytes, self.d2h_bytes = int(co.h2d_bytes), int(co.d2h_bytes)
        # with members=True: members of pick i (pmx[i, p]), leftovers of segment s = m k + p
        # (left_off[s]:left_off[s+1] of left_x / left_y) and its boxes in some clique
        self.pmx = self.pmy = self.left_off = self.left_x = self.left_y = self.in_clique = None
        # consensus_tiers fills these
        self.ptier = self.pmask = self.pw = self.pmember = self.box_tier = None
        self.tier_cols = self.tier_picks = None
        if mo is not None:
            S = n_mg * k
            self.pmx = _copy(mo.pmx, self.n_picked * k, np.float64).reshape(self.n_picked, k)
            self.pmy = _copy(mo.pmy, self.n_picked * k, np.float64).reshape(self.n_picked, k)
            self.left_off = _copy(mo.left_off, S + 1, np.int64)
            L = int(self.left_off[-1])
            self.left_x = _copy(mo.left_x, L, np.float64)
            self.left_y = _copy(mo.left_y, L, np.float64)
            self.in_clique = _copy(mo.in_clique, S, np.int32)


def write_boxes(out_dir, bases, box_size, pick_off, count, px, py, pconf, n_threads=1):
    """One ``<base>.box`` per micrograph from pick arrays (rgc_write_boxes, run_ilp.py:126-133);
    ``count[m]`` = -1 writes the empty file of a skipped micrograph."""
    n = len(bases)
    arrs = [np.ascontiguousarray(pick_off, np.int64), np.ascontiguousarray(count, np.int64),
            np.ascontiguousarray(px, np.float64), np.ascontiguousarray(py, np.float64),
            np.ascontiguousarray(pconf, np.float32)]
    assert len(arrs[0]) >= n and len(arrs[1]) == n
    bs = (C.c_char_p * max(1, n))(*[os.fsencode(b) for b in bases])
    wi = BoxWriteIn(os.fsencode(out_dir), n, int(box_size), bs, *[a.ctypes.data for a in arrs])
    bad = C.c_int64(-1)
    rc = lib.rgc_write_boxes(C.byref(wi), int(n_threads), C.byref(bad))
    if rc != 0:
        b = bases[bad.value] if 0 <= bad.value < n else ""
        raise OSError(-rc, os.strerror(-rc) if rc < -1 else "rgc_write_boxes failed",
                      os.path.join(out_dir, b + ".box"))


def write_members(out_dir, bases, box_size, pick_off, count, px, py, pconf, methods, pmx, pmy,
                  seg, left_off, left_x, left_y, n_threads=1):
    """``write_boxes`` and, from the same task per micrograph, ``<base>_members.tsv``
    (rgc_write_members): ``methods`` are the k header names, ``pmx`` / ``pmy`` [n, k] the
    members of pick i, ``seg[m]`` micrograph m's first segment in ``left_off``.  A skipped
    micrograph (count -1) gets its empty ``.box`` only."""
    _need_members()
    n, k = len(bases), len(methods)
    arrs = [np.ascontiguousarray(pick_off, np.int64), np.ascontiguousarray(count, np.int64),
            np.ascontiguousarray(px, np.float64), np.ascontiguousarray(py, np.float64),
            np.ascontiguousarray(pconf, np.float32)]
    more = [np.ascontiguousarray(pmx, np.float64), np.ascontiguousarray(pmy, np.float64),
            np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(left_off, np.int64),
            np.ascontiguousarray(left_x, np.float64), np.ascontiguousarray(left_y, np.float64)]
    assert len(arrs[0]) >= n and len(arrs[1]) == n and len(more[2]) == n and k >= 1
    assert more[0].size == more[1].size == len(arrs[2]) * k
    bs = (C.c_char_p * max(1, n))(*[os.fsencode(b) for b in bases])
    wi = MembersWriteIn(BoxWriteIn(os.fsencode(out_dir), n, int(box_size), bs,
                                   *[a.ctypes.data for a in arrs]),
                        k, os.fsencode("\t".join(methods)), *[a.ctypes.data for a in more])
    bad, which = C.c_int64(-1), C.c_int32(0)
    rc = lib.rgc_write_members(C.byref(wi), int(n_threads), C.byref(bad), C.byref(which))
    if rc != 0:
        b = bases[bad.value] if 0 <= bad.value < n else ""
        raise OSError(-rc, os.strerror(-rc) if rc < -1 else "rgc_write_members failed",
                      os.path.join(out_dir, b + (MEMBERS_SUFFIX if which.value else ".box")))


def _need_members():
    if not has_members():
        raise RGCError(f"{LIB_PATH} has no consensus --members entry points "
                       f"({', '.join(MEMBERS_SYMBOLS)}): rebuild it")


def _need_tiers():
    if not has_tiers():
        raise RGCError(f"{LIB_PATH} has no consensus --min_pickers entry points "
                       f"({', '.join(TIERS_SYMBOLS)}): rebuild it")


def _need_nms():
    if not has_nms():
        raise RGCError(f"{LIB_PATH} has no greedy-NMS entry points "
                       f"({', '.join(NMS_SYMBOLS)}): rebuild it")


def _need_agreement():
    if not has_agreement():
        raise RGCError(f"{LIB_PATH} has no picker-agreement entry points "
                       f"({', '.join(AGREE_SYMBOLS)}): rebuild it")


class Agreement:
    """One rgc_agreement call, as numpy copies.  ``support`` uint8 [N]: bit q set iff the box is
    joined to a box of picker q; ``partner`` int32 [N, k] / ``partner_ji`` f64 [N, k] (None
    without ``partners``): the joined box of picker q with the largest JI (ties: the lowest batch
    index; -1 / 0.0 without one); ``pair_edges`` / ``pair_supported`` / ``pair_mutual`` int64
    [n_mg, k, k]: joined pairs, boxes of (m, p) supported by q, reciprocal best partners."""

    def __init__(self, ao: AgreeOut, n_mg, k, n, partners):
        self.n_mg, self.k = n_mg, k
        self.support = _copy(ao.support, n, np.uint8)
        self.partner = self.partner_ji = None
        if partners:
            self.partner = _copy(ao.partner, n * k, np.int32).reshape(n, k)
            self.partner_ji = _copy(ao.partner_ji, n * k, np.float64).reshape(n, k)
        for f in ("pair_edges", "pair_supported", "pair_mutual"):
            setattr(self, f, _copy(getattr(ao, f), n_mg * k * k, np.int64).reshape(n_mg, k, k))


def np_float_str(v) -> str:
    """str(numpy.float32(v)) as the native BOX writer prints it (test hook)."""
    b = C.create_string_buffer(64)
    n = lib.rgc_np_float_str(C.c_float(float(v)), b, 64)
    if n < 0:
        raise RGCError("rgc_np_float_str failed")
    return b.value.decode()


class Result:
    """Host view of one rgc_run.  Per-micrograph and per-clique arrays are numpy views of
    pinned memory (per-clique arrays: device pointers without F_HOST_OUTPUTS).  The host views
    stay valid, with this run's values, for as long as they (or this Result) are referenced:
    each holds the run's :class:`_HostLease`, and the context hands the buffers over to it
    (rgc_detach_host) instead of reusing or freeing them.  Device pointers follow the C-ABI
    rule: valid until the next run on the context."""

    _PER_MG = {"status": ("status", np.int32), "cc_max": ("cc_max", np.int32),
               "cc_cnt": ("cc_cnt", np.int32), "n_nodes": ("n_nodes", np.int32),
               "n_vert": ("n_vert", np.int32), "n_edges_mg": ("n_edges_mg", np.int64),
               "clique_base": ("clique_base", np.int64), "clique_cnt": ("clique_cnt", np.int64)}

    def __getattr__(self, name):
        # per-micrograph arrays are built on first use (views, no copy)
        spec = Result._PER_MG.get(name)
        if spec is None:
            raise AttributeError(name)
        field, dt = spec
        dt = np.dtype(dt)
        if self._lazy is not None:   # F_LAZY_STATS: copied from HBM on first use
            # (once the buffers were detached, rgc_detach_host has fetched them already)
            if self._lease.block is None:
                _check(lib.rgc_fetch_stats(self._lazy._p))
            self._lazy = None
        p = getattr(self._bo, field)
        if not self.n_mg or not p:
            v = np.zeros(0, dt)
        else:
            addr = C.cast(p, C.c_void_p).value
            ct = {4: C.c_int32, 8: C.c_int64}[dt.itemsize]
            v = self._lease.view(addr, ct, self.n_mg).view(dt)
        setattr(self, name, v)
        return v

    def __init__(self, bo: BatchOut, n_mg: int, k: int, flags: int, ctx=None, lease=None):
        self._bo = bo
        self._lease = lease if lease is not None else _HostLease()
        self._lazy = ctx if (flags & F_LAZY_STATS) and ctx is not None else None
        self.n_mg, self.k = n_mg, k
        self.n_boxes, self.n_edges, self.n_cliques = bo.n_boxes, bo.n_edges, bo.n_cliques
        C_ = int(self.n_cliques)
        if flags & F_HOST_OUTPUTS:
            def h(p, ct, n):
                if not n or not p:
                    return np.zeros(n, dtype=np.dtype(ct))
                return self._lease.view(C.cast(p, C.c_void_p).value, ct, n)
            self.rows = h(bo.rows, C.c_int32, C_ * k).reshape(C_, k)
            self.w = h(bo.w, C.c_float, C_)
            self.conf = h(bo.conf, C.c_float, C_)
            self.consensus = h(bo.consensus, C.c_int32, C_)
            self.members = (h(bo.members, C.c_int32, C_ * k).reshape(C_, k)
                            if (flags & (F_MULTI_OUT | F_MEMBERS)) else None)
            self.order = (h(bo.order, C.c_uint8, C_ * k).reshape(C_, k)
                          if (flags & F_MULTI_OUT) else None)
        else:
            self.rows, self.w, self.conf = bo.rows, bo.w, bo.conf
            self.consensus, self.members, self.order = bo.consensus, bo.members, bo.order
