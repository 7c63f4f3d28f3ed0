/* repic_gc.h — C-ABI of librepic_gc.so, the MI355X-native `repic get_cliques` hot path.
 *
 * The reference has no FFI: its boundary is the Python subcommand plugin protocol
 * (`name`, `add_arguments(parser)`, `main(args)`; reference repic/commands/get_cliques.py
 * :13-27,72 registered in repic/main.py:17-29).  The Python host package
 * (repic-copy_amd/repic_amd/commands/get_cliques.py) keeps that protocol and calls the
 * entry points below through ctypes.  Each entry point replaces one stage of the
 * reference's per-micrograph loop (get_cliques.py:108-229):
 *
 *   rgc_parse_files  <- common.py:71-114 get_box_coords (BOX text -> x, y, score)
 *   rgc_write_outputs <- get_cliques.py:204-229 (the four pickles + runtime.tsv of each
 *                       micrograph; ABI 5)
 *   rgc_run          <- get_cliques.py:134-202: Jaccard pairs (:40-69,:134-138), graph
 *                       (:30-37,:142-143), connected components (:145-156), size-k
 *                       cliques (:49-56,:160-161), ILP weight / confidence / consensus
 *                       (:164-190) and constraint-matrix COO (:192-202), for a whole
 *                       batch of micrographs at once.
 *   rgc_ilp_solve    <- run_ilp.py:50-63 (the set packing, exact, instead of Gurobi)
 *   rgc_consensus    <- get_cliques.py:134-202 followed by run_ilp.py:50-124 without the
 *                       files in between (ABI 10): rgc_run, the solver and the ordered picks
 *                       in one call, the per-clique arrays staying in HBM
 *   rgc_write_boxes  <- run_ilp.py:126-133 (the final <base>.box of each micrograph; ABI 10)
 *   rgc_consensus_members, rgc_write_members
 *                    <- what get_cliques --multi_out + run_ilp.py:93-119 are meant to give and
 *                       never do (run_ilp raises on such inputs): per written pick its member
 *                       from every picker, and every picker's boxes left out of the picks
 *   rgc_agreement    <- get_cliques.py:59-69 get_jaccard as a report (beyond the reference): per
 *                       box which pickers have a box joined to it, per picker pair the joined
 *                       pairs, supported boxes and reciprocal best partners
 *
 * Conventions: plain pointers and sizes, no torch types.  Returns 0 on success and a
 * negative code on error (message in rgc_last_error(), thread-local).  Outputs are owned
 * by the context and stay valid until the next rgc_run on it or rgc_ctx_destroy, unless the
 * caller takes over their host buffers with rgc_detach_host (ABI 7).
 */
#ifndef REPIC_GC_H
#define REPIC_GC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGC_ABI_VERSION 11

/* flags for rgc_batch_in.flags */
#define RGC_F_GET_CC         1u  /* --get_cc   (get_cliques.py:151-156) */
#define RGC_F_MULTI_OUT      2u  /* --multi_out (get_cliques.py:175-178,206-213) */
#define RGC_F_DEVICE_INPUTS  4u  /* x/y/score are device pointers (HBM-resident) */
#define RGC_F_HOST_OUTPUTS   8u  /* copy per-clique outputs to pinned host memory */
#define RGC_F_TIMING        16u  /* record per-kernel HIP events (rgc_kernel_times) */
#define RGC_F_MEMBERS       32u  /* also return the k member boxes of every clique */
#define RGC_F_NO_FUSED      64u  /* route every micrograph through the multi-kernel path
                                    (testing / comparison; outputs are identical) */
#define RGC_F_DEVICE_META  128u  /* dev_box_off / dev_id_base hold HBM-resident copies of
                                    box_off (as int32) and id_base: no offset upload per run
                                    (the host arrays are still read for launch planning) */
#define RGC_F_LAZY_STATS   512u  /* rgc_submit (ABI 6): the per-micrograph outputs of a run that
                                  * takes the single fused launch stay in HBM; rgc_wait copies
                                  * only the run's totals and rgc_fetch_stats copies the rest
                                  * (outputs kept in HBM, like RGC_F_HOST_OUTPUTS unset) */
#define RGC_F_EDGES        256u  /* test hook: also record every JI > threshold edge with its
                                    f64 JI (rgc_last_edges); outputs are unchanged */
#define RGC_F_JI_THRESHOLD 1024u /* ABI 11: rgc_batch_in.ji_threshold holds the Jaccard threshold
                                  * (else 0.3, and the field is not read: a caller built against
                                  * the earlier struct layout works unchanged) */

/* per-micrograph status (rgc_batch_out.status) */
#define RGC_OK          0   /* outputs written as in get_cliques.py:215-229 */
#define RGC_NO_EDGES    1   /* reference raises ValueError (np.max([]), :148) */
#define RGC_NO_CLIQUES  2   /* reference raises UnboundLocalError (del clique, :203) */

typedef struct rgc_ctx rgc_ctx;

typedef struct rgc_batch_in {
  int32_t n_mg;            /* micrographs in the batch */
  int32_t k;               /* pickers (= clique size, get_cliques.py:160), 1..8 */
  int64_t box_size;        /* CLI box_size (int pixels, get_cliques.py:22-23) */
  uint32_t flags;
  const int64_t* box_off;  /* HOST [n_mg*k+1]: boxes of (mg m, picker p) are
                              [box_off[m*k+p], box_off[m*k+p+1]) in file order */
  const int64_t* id_base;  /* HOST [n_mg]: global box id of the first box of each
                              micrograph (common.py:23,108-112 counter) */
  const double* x;         /* [N] box x (common.py:87), host or device per flags */
  const double* y;         /* [N] box y */
  const double* score;     /* [N] score, sigmoid already applied on host (common.py:92-94) */
  const int32_t* dev_box_off;  /* DEVICE [n_mg*k+1], int32 copy of box_off (RGC_F_DEVICE_META) */
  const int64_t* dev_id_base;  /* DEVICE [n_mg], copy of id_base (RGC_F_DEVICE_META) */
  double ji_threshold;     /* ABI 11, read only with RGC_F_JI_THRESHOLD: two boxes of different
                              pickers are joined when the reference's f64 JI (get_cliques.py
                              :40-46) exceeds it (get_jaccard's `threshold`, :59-69; the
                              reference passes 0.3, :138).  Finite, 0 <= t < 1, else rgc_run /
                              rgc_submit / rgc_consensus fail before any launch */
} rgc_batch_in;

typedef struct rgc_batch_out {
  int64_t n_boxes, n_edges, n_cliques;
  /* per micrograph [n_mg], host memory */
  int32_t* status;
  int32_t* cc_max;         /* runtime.tsv column 2 (get_cliques.py:228) */
  int32_t* cc_cnt;         /* runtime.tsv column 3 */
  int32_t* n_nodes;        /* graph nodes (boxes with >= 1 edge) */
  int32_t* n_vert;         /* constraint-matrix rows V (get_cliques.py:164) */
  int64_t* n_edges_mg;     /* JI > threshold edges */
  int64_t* clique_base;    /* cliques of mg m are [clique_base[m], +clique_cnt[m]) in the */
  int64_t* clique_cnt;     /* per-clique arrays (ranges of different micrographs do not
                              overlap; their order is unspecified) */
  /* per clique; host (RGC_F_HOST_OUTPUTS) or device pointers */
  int32_t* rows;           /* [C*k] COO row indices of each clique column, ascending */
  float* w;                /* [C] weight vector (get_cliques.py:188-190) */
  float* conf;             /* [C] consensus confidences (:186-187) */
  int32_t* consensus;      /* [C] global box index of the consensus box (:182-183) */
  int32_t* members;        /* [C*k] global box index of each member, picker order
                              (with RGC_F_MEMBERS or RGC_F_MULTI_OUT, else NULL) */
  uint8_t* order;          /* [C*k] networkx node-iteration order as picker indices
                              (only with RGC_F_MULTI_OUT, else NULL) */
} rgc_batch_out;

typedef struct rgc_parsed {
  int64_t n_files;
  int32_t* status;         /* [n_files] RGC_PARSE_* */
  int64_t* off;            /* [n_files+1] boxes of file f are [off[f], off[f+1]) */
  double* x;
  double* y;
  double* score;           /* raw scores (sigmoid NOT applied) */
  uint8_t* sigmoid;        /* [n_files] 1 if min(score) < 0 (common.py:92) */
} rgc_parsed;

/* rgc_parsed.status — the exception get_box_coords would raise for that file */
#define RGC_PARSE_OK          0
#define RGC_PARSE_INDEX       1  /* IndexError: empty file / blank first line / no coords */
#define RGC_PARSE_VALUE       2  /* ValueError: shortest row != 5 tokens, bad weight */
#define RGC_PARSE_ASSERT      3  /* AssertionError: len(X) != len(Y) */
#define RGC_PARSE_FALLBACK    4  /* non-ASCII / unusual bytes: parse in Python instead */
#define RGC_PARSE_OSERROR     5  /* could not open / read */

int rgc_abi_version(void);
const char* rgc_last_error(void);
int rgc_device_count(int* n);

int rgc_ctx_create(int device, void* hip_stream, rgc_ctx** out);
void rgc_ctx_destroy(rgc_ctx* ctx);
/* ABI 9: the stream of a submitted non-lazy run's per-micrograph stats copy (hip_stream may be
 * 0: the device's null stream).  Without a call every context of the process shares one copy
 * stream per device, so N contexts on N launch streams take N + 1 hardware queues, not 2 N
 * (GPU_MAX_HW_QUEUES is 4 on the MI355X boxes). */
int rgc_ctx_set_copy_stream(rgc_ctx* ctx, void* hip_stream);
int rgc_run(rgc_ctx* ctx, const rgc_batch_in* in, rgc_batch_out* out);
/* Asynchronous rgc_run (ABI 3), one run in flight per context: rgc_submit enqueues the batch
 * on the context's stream and returns; rgc_wait blocks until it is done and fills *out exactly
 * as rgc_run would.  Host and device arrays of the batch must stay valid until rgc_wait.  A
 * batch that takes the single fused launch (HBM-resident inputs and offsets, RGC_F_DEVICE_INPUTS
 * | RGC_F_DEVICE_META, device outputs) runs while the caller continues, so with two contexts
 * on one stream the host prepares and launches batch i+1 while the device runs batch i (on
 * two streams the two launches also overlap on the device); any other batch runs through
 * rgc_run's general path on a worker thread of the context (since round 5: it syncs on the
 * host once per clique level, so a second context on its own stream keeps the device busy
 * meanwhile), and one whose micrographs need a second pass re-runs that path inside rgc_wait.
 * Outputs stay valid until the next submit/run on the same context.  While a submitted
 * run awaits rgc_wait, rgc_submit, rgc_run, rgc_score_pairs, rgc_score_sweep, rgc_score_match, rgc_score_match_sweep, rgc_nms, rgc_agreement and rgc_ilp_solve on the same
 * context fail (negative return, rgc_last_error says why). */
int rgc_submit(rgc_ctx* ctx, const rgc_batch_in* in);
int rgc_wait(rgc_ctx* ctx, rgc_batch_out* out);
/* ABI 6: after rgc_wait of an RGC_F_LAZY_STATS run, copy its per-micrograph outputs into the
 * host arrays *out points to (a no-op for any other run).  Valid until the next run on ctx. */
int rgc_fetch_stats(rgc_ctx* ctx);
/* ABI 7: ownership hand-off of the last run's host outputs.  rgc_detach_host moves every
 * pinned host buffer of the context (the per-micrograph arrays, the RGC_F_HOST_OUTPUTS
 * per-clique arrays, a lazy run's stats, fetched first) into *block: the pointers the last
 * rgc_batch_out holds stay valid, and stay unchanged, until rgc_host_block_free(*block), even
 * after further runs or rgc_ctx_destroy; the context allocates new buffers for its next run.
 * Fails while a submitted run awaits rgc_wait.  (repic_amd/_lib.py calls it only when a
 * Result of the last run is still referenced when the next run starts or the context closes.) */
int rgc_detach_host(rgc_ctx* ctx, void** block);
void rgc_host_block_free(void* block);
/* Per-kernel device milliseconds of the last rgc_run with RGC_F_TIMING; returns the count. */
int rgc_kernel_times(rgc_ctx* ctx, int max_n, float* ms, const char** names);

/* Test hook (RGC_F_EDGES): the JI > threshold edges of the last rgc_run as host arrays (batch
 * box indices u < v by picker, JI in the reference's f64 op order, get_cliques.py:40-46,59-69),
 * valid until the next rgc_run; returns the edge count (order unspecified). */
int64_t rgc_last_edges(rgc_ctx* ctx, const int32_t** u, const int32_t** v, const double** ji);

/* score_detections (repic/utils/score_detections.py:16-48 get_segmentation_scores): for every
 * (ground truth, picker) pair, the pixel counts of the int16 masks the reference paints.
 * Boxes are given as numpy slice bounds already normalised on the host (row start < row end
 * <= height, col start < col end <= width; boxes with an empty slice are left out), picked
 * boxes already filtered by the confidence threshold.  counts[3p..3p+2] = sum(gt_arr),
 * sum(pckr_arr), sum(gt_arr * pckr_arr).  RGC_F_TIMING records "k_score_raster". */
typedef struct rgc_score_in {
  int64_t n_pairs;
  const int64_t* height;   /* [n_pairs] mask rows (mrc_h) */
  const int64_t* width;    /* [n_pairs] mask columns (mrc_w) */
  const int64_t* gt_off;   /* [n_pairs + 1] pair p's ground truth: boxes[gt_off[p], gt_off[p+1]) */
  const int64_t* pk_off;   /* [n_pairs + 1] pair p's picks: boxes[pk_off[p], pk_off[p+1]) */
  const int32_t* boxes;    /* [n_boxes][4] row start, row end, col start, col end */
  uint32_t flags;          /* RGC_F_TIMING */
} rgc_score_in;
int rgc_score_pairs(rgc_ctx* ctx, const rgc_score_in* in, int64_t* counts);

/* Confidence-threshold sweep of score_detections: what rgc_score_pairs returns for the picks
 * kept at each of n_thr ascending thresholds (a pick is kept at t iff not conf < t,
 * score_detections.py:34-36), from one launch that paints every box once (k_score_sweep).  The
 * caller orders each pair's picks so that the ones kept at threshold j are a prefix and gives
 * the prefix lengths.  counts[p][j] = sum(gt_arr), sum(pckr_arr at threshold j),
 * sum(gt_arr * pckr_arr at threshold j).  RGC_F_TIMING (pairs.flags) records "k_score_sweep".
 * Refused before any launch, the context staying usable: n_thr outside 1..RGC_SCORE_MAX_THR, a
 * keep that is negative, larger than the pair's pick count or increasing in j, a submitted run
 * awaiting rgc_wait, and whatever rgc_score_pairs refuses.
 * An additive symbol: no struct changes layout and RGC_ABI_VERSION stays 11; a caller finds out
 * whether the library has it by looking the symbol up. */
#define RGC_SCORE_MAX_THR 1024
typedef struct rgc_score_sweep_in {
  rgc_score_in pairs;      /* as for rgc_score_pairs; each pair's picks ordered as above */
  int32_t n_thr;           /* T, 1..RGC_SCORE_MAX_THR */
  const int64_t* keep;     /* [n_pairs * T] picks of pair p kept at threshold j:
                              boxes[pk_off[p], pk_off[p] + keep[p*T+j]) */
} rgc_score_sweep_in;
int rgc_score_sweep(rgc_ctx* ctx, const rgc_score_sweep_in* in, int64_t* counts /* [n_pairs][T][3] */);

/* Particle-level matching (beyond the reference): for every (ground truth, picks) pair the size
 * of a maximum-cardinality one-to-one matching between ground-truth boxes and picks, two boxes
 * being joined iff their exact intersection over union exceeds ji_threshold: with integer
 * rectangles [x0, x1) x [y0, y1), I the intersection area and U the union area in int64,
 * U > 0 and (double)I / (double)U > t, one f64 division.  A box with x1 <= x0 or y1 <= y0 is
 * counted but never matched.  counts[p] = n_gt, n_picked, tp.  match (may be NULL) receives,
 * for every pick in the caller's order (pair after pair), the index of its ground-truth box
 * within the pair or -1; the matching returned is a function of the inputs alone (claims are
 * resolved by lowest index, never by arrival).  RGC_F_TIMING records "k_score_match_count"
 * and "k_score_match".
 * Refused before any launch, the context staying usable: null arguments, a submitted run
 * awaiting rgc_wait, n_pairs outside 0..INT32_MAX, negative or decreasing offsets, a threshold
 * that is NaN or outside [0, 1), |x0| or |y0| above 2^30, x1 - x0 or y1 - y0 above 2^25, more
 * than 2^31 - 1 boxes; refused after the count launch: more than 2^31 - 1 edges.
 * Additive symbols: no struct changes layout and RGC_ABI_VERSION stays 11. */
typedef struct rgc_score_match_in {
  int64_t n_pairs;
  const int64_t* gt_off;   /* [n_pairs + 1] pair p's ground truth: boxes[gt_off[p], gt_off[p+1]) */
  const int64_t* pk_off;   /* [n_pairs + 1] pair p's picks (already filtered by confidence) */
  const int32_t* boxes;    /* [n_boxes][4] x0, x1, y0, y1 (x1 = x0 + w, y1 = y0 + h) */
  double ji_threshold;     /* finite, 0 <= t < 1 */
  uint32_t flags;          /* RGC_F_TIMING */
} rgc_score_match_in;
int rgc_score_match(rgc_ctx* ctx, const rgc_score_match_in* in, int64_t* counts /* [n_pairs][3] */,
                    int32_t* match /* [total picks] or NULL */);
/* Particle-level matching at every confidence threshold of a sweep (the precision / recall
 * curve): what rgc_score_match returns for the picks kept at each of n_thr ascending thresholds,
 * from one call that lays the pairs out, counts the edges and builds the edge lists once
 * (k_score_match_sweep).  The caller orders each pair's picks so that the ones kept at threshold
 * j are a prefix and gives the prefix lengths, as for rgc_score_sweep.  The kernel walks the
 * thresholds from the strictest to the loosest, keeps the matching of the step before and
 * augments it from the picks that are new at the step.  counts[p][j] = n_gt, keep[p][j], tp at
 * threshold j; no assignment is returned.  RGC_F_TIMING (pairs.flags) records
 * "k_score_match_count" and "k_score_match_sweep".
 * Refused before any launch, the context staying usable: whatever rgc_score_match refuses, n_thr
 * outside 1..RGC_MATCH_MAX_THR, a null keep with n_pairs > 0, a keep that is negative, larger
 * than the pair's pick count or increasing in j, a submitted run awaiting rgc_wait.
 * An additive symbol: no struct changes layout and RGC_ABI_VERSION stays 11. */
#define RGC_MATCH_MAX_THR 1024
typedef struct rgc_score_match_sweep_in {
  rgc_score_match_in pairs;  /* as for rgc_score_match; each pair's picks ordered so that the
                                picks kept at threshold j are a prefix */
  int32_t n_thr;             /* T, 1..RGC_MATCH_MAX_THR */
  const int64_t* keep;       /* [n_pairs * T], non-increasing in j, 0 <= keep <= the pair's picks */
} rgc_score_match_sweep_in;
int rgc_score_match_sweep(rgc_ctx* ctx, const rgc_score_match_sweep_in* in,
                          int64_t* counts /* [n_pairs][T][3] */);
/* Host twin of the device edge test of rgc_score_match on two boxes (x0, x1, y0, y1): 1 / 0. */
int rgc_test_iou_edge(const int32_t a[4], const int32_t b[4], double t);

/* Greedy non-maximum suppression (beyond the reference).  A segment is a list of boxes in
 * priority order (index 0 is the highest priority); all boxes are squares of side box_size with
 * lower-left corner (x, y) in f64.  Two boxes conflict iff the reference quotient exceeds the
 * threshold: calc_jaccard of get_cliques.py:40-46 in its f64 operation order (no FMA, one
 * division), strict `> ji_threshold`.  keep[i] = 1 iff no j < i of the same segment has
 * keep[j] = 1 and conflicts with i.  That set is unique (it is the greedy result, and the only
 * set for which the sentence holds at every i), so the output is a function of the input alone.
 * A box with a non-finite coordinate conflicts with nothing (the formula yields 0 or NaN there):
 * it is kept and suppresses nothing.  Boxes of different segments never interact.  kept[s] = the
 * boxes kept of segment s.  n_seg == 0 and empty segments are valid and launch nothing.
 * One workgroup per segment decides its boxes in rounds, at most n + 1 for n boxes; a segment
 * that ran out of rounds fails the call.  RGC_F_TIMING records "k_nms_count" and "k_nms".
 * Refused before any launch, the context staying usable: null arguments with boxes to read or
 * write, a submitted run awaiting rgc_wait, n_seg outside 0..INT32_MAX, offsets that do not
 * start at 0 or decrease, more than 2^31 - 1 boxes, box_size outside 1..2^26, a threshold that is
 * NaN or outside [0, 1); refused after the count launch: more than 2^31 - 1 conflict edges.
 * Additive symbols: no struct changes layout and RGC_ABI_VERSION stays 11; a caller finds out
 * whether the library has them by looking the symbols up. */
typedef struct rgc_nms_in {
  int64_t n_seg;
  const int64_t* seg_off;   /* HOST [n_seg + 1], starts at 0, non-decreasing */
  const double* x;          /* HOST [n] lower-left x, each segment in priority order */
  const double* y;
  int64_t box_size;         /* 1..2^26 */
  double ji_threshold;      /* finite, 0 <= t < 1 */
  uint32_t flags;           /* RGC_F_TIMING */
} rgc_nms_in;
int rgc_nms(rgc_ctx* ctx, const rgc_nms_in* in, uint8_t* keep /* [n] */,
            int64_t* kept /* [n_seg] */);
/* Bytes the last rgc_nms on ctx copied to and from the device (0, 0 when it launched nothing). */
int rgc_nms_last_bytes(rgc_ctx* ctx, int64_t* h2d, int64_t* d2h);

/* Picker agreement (beyond the reference): how much the pickers of a batch agree, per box and per
 * picker pair.  The batch layout is rgc_batch_in's: segment s = m*k + p holds the boxes of picker
 * p of micrograph m in file order, squares of side box_size with corner (x, y) in f64.  Two boxes
 * b, c of the same micrograph and different pickers are joined iff |x_b - x_c| <= box_size and the
 * reference quotient exceeds the threshold, strictly: get_jaccard (get_cliques.py:59-69) on
 * calc_jaccard (:40-46) in its f64 operation order (no FMA, one division) - exactly the edge set
 * of the consensus graph at that threshold.  The quotient is symmetric in its two boxes bit for
 * bit, so "joined" is symmetric; a box with a non-finite coordinate is joined to nothing (the
 * formula yields 0 or NaN there).  N = box_off[n_mg*k]; indices are batch box indices.
 *   support[b]              bit q set iff b is joined to at least one box of picker q (never the
 *                           bit of b's own picker)
 *   partner[b*k+q]          the box of picker q joined to b with the largest JI, ties to the
 *                           lowest batch index; -1 if none, and for b's own picker
 *   partner_ji[b*k+q]       that partner's JI, bit for bit the reference quotient; 0.0 where
 *                           partner is -1
 *   pair_edges[(m*k+p)*k+q]     joined pairs between segments (m,p) and (m,q): symmetric,
 *                               diagonal 0
 *   pair_supported[(m*k+p)*k+q] boxes of (m,p) whose bit q is set (directed), diagonal 0
 *   pair_mutual[(m*k+p)*k+q]    boxes b of (m,p) with c = partner[b][q] >= 0 and
 *                               partner[c][p] == b: reciprocal best partners, a one-to-one
 *                               pairing, symmetric and deterministic (not a maximum matching)
 * Every output is a function of the inputs alone.  The outputs are host memory owned by the
 * context, valid until its next call.  Without RGC_F_PARTNERS partner / partner_ji are NULL and
 * never leave the device: the call copies back 1 B per box and 24 k^2 B per micrograph.
 * n_mg == 0 and all-empty batches are valid and launch nothing (n_mg == 0: every pointer NULL);
 * k == 1: every mask 0, every partner -1.  One workgroup per segment with a finite box, two
 * launches; RGC_F_TIMING records "k_agree_partner" and "k_agree_mutual".
 * Refused before any launch, the context staying usable: null arguments with boxes to read, a
 * submitted run awaiting rgc_wait, n_mg < 0 or n_mg*k above INT32_MAX, k outside 1..8, offsets
 * that do not start at 0 or decrease, more than 2^31 - 1 boxes, box_size outside 1..2^26, a
 * threshold that is NaN or outside [0, 1).
 * Additive symbols: no struct changes layout and RGC_ABI_VERSION stays 11; a caller finds out
 * whether the library has them by looking the symbols up. */
#define RGC_F_PARTNERS 2048u     /* rgc_agree_in.flags: also return partner / partner_ji */
typedef struct rgc_agree_in {
  int32_t n_mg;
  int32_t k;                /* 1..8 */
  int64_t box_size;         /* 1..2^26 */
  double ji_threshold;      /* finite, 0 <= t < 1 */
  uint32_t flags;           /* RGC_F_TIMING | RGC_F_PARTNERS */
  const int64_t* box_off;   /* HOST [n_mg*k+1], starts at 0, non-decreasing */
  const double* x;          /* HOST [N] */
  const double* y;
} rgc_agree_in;
typedef struct rgc_agree_out {
  uint8_t* support;         /* [N] */
  int32_t* partner;         /* [N*k], NULL without RGC_F_PARTNERS */
  double* partner_ji;       /* [N*k], NULL without RGC_F_PARTNERS */
  int64_t* pair_edges;      /* [n_mg*k*k] */
  int64_t* pair_supported;
  int64_t* pair_mutual;
} rgc_agree_out;
int rgc_agreement(rgc_ctx* ctx, const rgc_agree_in* in, rgc_agree_out* out);
/* Bytes the last rgc_agreement on ctx copied to and from the device (0, 0 when it launched
 * nothing). */
int rgc_agreement_last_bytes(rgc_ctx* ctx, int64_t* h2d, int64_t* d2h);

/* run_ilp (repic/commands/run_ilp.py:50-63): maximise w.x over binary x subject to A x <= 1,
 * exactly, for a batch of micrographs at once (rows are global box ids: micrographs never
 * share a row).  A is given in CSC form.  x[c] = 1 for the chosen columns (cliques);
 * exact[c] is the status of column c's conflict component:
 *   RGC_ILP_OPTIMAL  (1) proven optimal: by the branch and bound, or (ABI 9) for a component
 *                        the search could not finish, by the exact search of the columns its
 *                        Lagrangian reduced costs leave (reduced-cost fixing: every packing
 *                        that uses another column is worth less than the certified one);
 *   RGC_ILP_GAP_OK   (2) not searched to the end (more than 4096 cliques, or node_limit hit),
 *                        but a Lagrangian dual bound certifies x within a relative gap of 1e-4,
 *                        the default MIPGap at which Gurobi reports a model optimal;
 *   RGC_ILP_NODE_LIMIT (0) node_limit hit, x is the best packing found, gap above 1e-4;
 *   RGC_ILP_HEURISTIC (3) too large to search, x is a greedy + swap local-search packing,
 *                        gap above 1e-4.
 * RGC_F_TIMING records the stages in rgc_kernel_times. */
#define RGC_ILP_NODE_LIMIT 0
#define RGC_ILP_OPTIMAL 1
#define RGC_ILP_GAP_OK 2
#define RGC_ILP_HEURISTIC 3
#define RGC_ILP_DEFAULT_NODES (1 << 14)
typedef struct rgc_ilp_in {
  int64_t n_cols;          /* cliques */
  int64_t n_rows;          /* boxes */
  const int64_t* col_ptr;  /* [n_cols + 1] column c's rows: row_idx[col_ptr[c], col_ptr[c+1]) */
  const int32_t* row_idx;  /* [nnz] global row ids */
  const double* w;         /* [n_cols] objective */
  int64_t node_limit;      /* branch-and-bound nodes per component (0: RGC_ILP_DEFAULT_NODES);
                              components of more than 1024 cliques get node_limit * 16 / W,
                              W = 64-clique words (work-scaled); each reduced-cost-fixing pass
                              (up to 2 below the first) searches with 4x the nodes of the one
                              above.  The node budgets are the only limit of the search, so
                              the result is deterministic */
  uint32_t flags;          /* RGC_F_TIMING */
  double* gap;             /* optional (NULL: not returned), ABI 6: [n_cols] dual bound minus
                            * packing value of column c's component, at the component's first
                            * column (0 elsewhere and for proven-optimal components), so a
                            * caller can certify a whole micrograph the way Gurobi's MIPGap
                            * does (sum of gaps <= 1e-4 x its objective) */
  double time_limit_s;     /* ABI 8, ignored since ABI 9: the search ran under a wall-clock budget,
                            * which made x depend on the device's speed and load; it is bounded
                            * by node budgets only now (kept for the struct layout) */
} rgc_ilp_in;
int rgc_ilp_solve(rgc_ctx* ctx, const rgc_ilp_in* in, uint8_t* x, uint8_t* exact);

/* ABI 10 — `repic consensus`: get_cliques and run_ilp in one device pass.  rgc_consensus does
 * rgc_run's work (both routes, RGC_F_GET_CC, host or device inputs), turns the per-clique
 * outputs into the solver's inputs on the device (rgc_pick.hip k_pick_cols: the rows, weights,
 * confidences and consensus ids never leave HBM), solves the set packing of every micrograph
 * as rgc_ilp_solve does, and emits the picked particles (k_pick_emit) in the order of
 * run_ilp.py:121-131: confidence descending (compared as floats, +0.0 == -0.0), equal
 * confidences in ascending column order, coordinates rounded with np.rint (half to even).
 * Columns are packed micrograph by micrograph, so the result does not depend on the order in
 * which the clique ranges were reserved.  Micrographs with status != RGC_OK have no columns
 * and no picks.  RGC_F_MULTI_OUT is rejected (the reference's run_ilp raises on such inputs);
 * fails like rgc_ilp_solve while a submitted run awaits rgc_wait.  With RGC_F_TIMING (batch
 * or opts flags) rgc_kernel_times lists rgc_run's sections, then "k_pick_cols", the solver's
 * sections and "k_pick_emit". */
typedef struct rgc_consensus_opts {
  int64_t node_limit;      /* as rgc_ilp_in.node_limit (0: RGC_ILP_DEFAULT_NODES) */
  int64_t num_particles;   /* keep the first N picks of each micrograph (run_ilp.py:129); < 0:
                              all; 0: none */
  uint32_t flags;          /* RGC_F_TIMING */
} rgc_consensus_opts;

typedef struct rgc_consensus_out {
  rgc_batch_out run;       /* exactly what rgc_run returns for the batch (per-clique pointers:
                              device, or host with RGC_F_HOST_OUTPUTS; valid until the next
                              run on the context) */
  int64_t n_picked;        /* = pick_off[n_mg] */
  /* host memory, owned by the context like run's per-micrograph arrays */
  int64_t* pick_off;       /* [n_mg+1] picks of micrograph m: [pick_off[m], pick_off[m+1]) */
  double* px;              /* [n_picked] np.rint(consensus x) */
  double* py;
  float* pconf;            /* [n_picked] confidence of the picked clique */
  int32_t* pcol;           /* [n_picked] its column within the micrograph's clique range */
  int32_t* sel_cnt;        /* [n_mg] columns chosen by the packing, before num_particles */
  int32_t* ilp_status;     /* [n_mg] RGC_ILP_*: OPTIMAL when every conflict component was
                              proven; else GAP_OK when the summed component gaps are within
                              1e-4 of the objective; else the weakest component status */
  double* ilp_gap;         /* [n_mg] summed component gaps / objective */
  int64_t h2d_bytes;       /* bytes this call copied host -> device and device -> host */
  int64_t d2h_bytes;
} rgc_consensus_out;
int rgc_consensus(rgc_ctx* ctx, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                  rgc_consensus_out* out);

/* The emit stage alone, on host arrays (uploaded, run, copied back): test hook of
 * k_pick_select / k_pick_emit.  Outputs are owned by the context (valid until its next call). */
typedef struct rgc_pick_in {
  int32_t n_mg;
  const int64_t* col_off;  /* [n_mg+1] columns of micrograph m */
  const uint8_t* x;        /* [n_cols] the packing */
  const float* conf;       /* [n_cols] */
  const double* cx;        /* [n_cols] consensus coordinates of each column */
  const double* cy;
  int64_t num_particles;   /* < 0: all */
} rgc_pick_in;
typedef struct rgc_pick_out {
  int64_t n_picked;
  int64_t* pick_off;       /* [n_mg+1] */
  double* px;
  double* py;
  float* pconf;
  int32_t* pcol;
} rgc_pick_out;
int rgc_pick_select(rgc_ctx* ctx, const rgc_pick_in* in, rgc_pick_out* out);

/* `repic consensus --members`: which box of which picker made up each written pick, and which
 * boxes of each picker are in no written pick.  Additive symbols: no struct changes layout and
 * RGC_ABI_VERSION stays 11; a caller finds out by symbol lookup.
 * rgc_consensus_members does everything rgc_consensus does, on a run with RGC_F_MEMBERS forced
 * on, then emits on the device (rgc_pick.hip k_pick_clique_mark / k_pick_members / k_pick_left)
 * the arrays below: host memory owned by the context like the pick arrays.  Segment
 * s = m * k + p is picker p of micrograph m.  A micrograph with status != RGC_OK has no
 * leftovers.  The picks of a packing have disjoint members, so segment s has
 * boxes(s) - picks(m) leftovers; if chosen columns of one micrograph share a box the call
 * fails and says so.  With RGC_F_TIMING the section "k_pick_members" follows "k_pick_emit";
 * h2d_bytes / d2h_bytes include these arrays (16 k B per pick, 16 B per leftover). */
typedef struct rgc_members_out {
  double* pmx;             /* [n_picked*k] np.rint(x) of pick i's member from picker p at i*k+p */
  double* pmy;
  int64_t* left_off;       /* [n_mg*k+1] leftovers of segment s: [left_off[s], left_off[s+1]) */
  double* left_x;          /* [left_off[n_mg*k]] np.rint(x) of the segment's boxes that are in */
  double* left_y;          /*   no written pick, in file order */
  int32_t* in_clique;      /* [n_mg*k] distinct boxes of the segment in at least one clique */
} rgc_members_out;
int rgc_consensus_members(rgc_ctx* ctx, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                          rgc_consensus_out* out, rgc_members_out* mem);

/* The select / scan / emit / members kernels alone, on host arrays: test hook, the counterpart
 * of rgc_pick_select.  Every micrograph counts as RGC_OK.  Refused before any launch (the
 * context stays usable) for null arrays, offsets that do not start at 0 or decrease, a member
 * or consensus index outside its segment, k outside 1..8 and a run awaiting rgc_wait. */
typedef struct rgc_pick_members_in {
  int32_t n_mg;
  int32_t k;
  const int64_t* col_off;  /* [n_mg+1] columns of micrograph m */
  const uint8_t* x;        /* [n_cols] the packing */
  const float* conf;       /* [n_cols] */
  const int32_t* cons;     /* [n_cols] box of the consensus coordinates (one of the members' range) */
  const int32_t* members;  /* [n_cols*k] batch box indices, picker order */
  const int64_t* box_off;  /* [n_mg*k+1] */
  const double* bx;        /* [n_boxes] */
  const double* by;
  int64_t num_particles;   /* < 0: all */
} rgc_pick_members_in;
int rgc_pick_members(rgc_ctx* ctx, const rgc_pick_members_in* in, rgc_pick_out* out,
                     rgc_members_out* mem);

/* `repic consensus --min_pickers M`: tiered picks agreed by at least M of the k pickers.
 * Additive symbols: no struct changes layout and RGC_ABI_VERSION stays 11; a caller finds out by
 * symbol lookup.  Tiers run t = k, k-1, .., M, per micrograph:
 *   tier k   is rgc_consensus: the same run, packing and picks.
 *   explain  before tier t < k a box b is explained iff a pick c of a higher tier has
 *            JI(b, c) > the run's threshold, c the pick's consensus box at its unrounded
 *            coordinates, JI the reference's f64 quotient (calc_jaccard's operation order, strict
 *            `>`, the test of rgc_nms); a box with a non-finite coordinate is explained by nothing.
 *            box_tier[b] = the tier of the first pick that explained b, else 0 (the picks of tier
 *            M mark their boxes too, so on return box_tier covers every tier).
 *   tier t   for every subset S of t pickers, in ascending order of the picker-index tuple, the
 *            unexplained boxes of S's pickers in file order form a pseudo-micrograph (box ids:
 *            id_base[m] + position).  One with an empty segment is not submitted.  All of a tier's
 *            pseudo-micrographs go through one run (k' = t, the same threshold), so a tier's
 *            cliques, weights, confidences and consensus boxes are what rgc_run gives for those
 *            boxes alone.  One set packing per micrograph over the columns of all its subsets
 *            (subset order, then the run's clique order; rows are full-batch box indices; weights
 *            are the run's w), picks in run_ilp's order.  A tier in which nothing can be submitted
 *            is skipped; the loop ends once no micrograph has M pickers with an unexplained box.
 * `out` is filled as rgc_consensus fills it: out->run is tier k's run (its per-clique pointers are
 * NULL once a lower tier made a run, with or without RGC_F_HOST_OUTPUTS: the lower tiers' runs
 * reuse the context's per-clique arrays), except run.status: RGC_OK iff some tier gave the micrograph a
 * column, else tier k's.  The pick arrays hold every tier: per micrograph tier descending, then the
 * tier's own order; pcol is the column within the micrograph's columns of that tier; sel_cnt the
 * chosen columns summed over tiers; ilp_status the weakest over the tiers that had columns and
 * ilp_gap the largest.  opts->num_particles keeps the first N picks of that order and is applied
 * last, on the host: every pick takes part in explaining.
 * With RGC_F_TIMING the sections "k_vote_explain", "k_vote_gather", the tier's run, "k_vote_cols",
 * the solver's and "k_pick_emit" follow tier k's, per tier.
 * Refused before any launch, the context staying usable: null arguments, a submitted run awaiting
 * rgc_wait, RGC_F_MULTI_OUT or RGC_F_GET_CC, min_pickers outside 2..k. */
typedef struct rgc_tiers_out {
  int32_t n_tiers;         /* k - min_pickers + 1; tier index j is tier k - j */
  /* host memory owned by the context, like the pick arrays */
  int32_t* ptier;          /* [n_picked] tier of each pick */
  int32_t* pmask;          /* [n_picked] bit p set: picker p is in the pick's subset */
  float* pw;               /* [n_picked] the pick's column weight */
  int32_t* pmember;        /* [n_picked*k] batch box index of picker p's member at i*k+p, else -1 */
  int32_t* box_tier;       /* [n_boxes] */
  int64_t* tier_cols;      /* [n_mg*n_tiers] columns of micrograph m in tier index j at m*n_tiers+j */
  int64_t* tier_picks;     /* [n_mg*n_tiers] picks written (after num_particles) */
} rgc_tiers_out;
int rgc_consensus_tiers(rgc_ctx* ctx, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                        int min_pickers, rgc_consensus_out* out, rgc_tiers_out* tiers);

/* The explain / count / gather kernels alone, on host arrays: test hook, the counterpart of
 * rgc_pick_select.  The picks of micrograph m, [pick_off[m], pick_off[m+1]) of pcx / pcy, mark the
 * boxes they explain with pick_tier (box_tier_in, may be NULL: all 0, is the state before); then
 * the pseudo-batch of tier t is built from the boxes still at 0.  Outputs are owned by the context
 * (valid until its next call).  Refused before any launch: null arrays, offsets that do not start
 * at 0 or decrease, k outside 1..8, t outside 1..k, pick_tier < 1, a bad box_size or threshold
 * and a run awaiting rgc_wait. */
typedef struct rgc_vote_gather_in {
  int32_t n_mg;
  int32_t k;
  int32_t t;               /* pickers per subset of the pseudo-batch */
  int32_t pick_tier;       /* what explained boxes are marked with */
  int64_t box_size;
  double ji_threshold;
  const int64_t* box_off;  /* [n_mg*k+1] */
  const double* x;         /* [n_boxes] */
  const double* y;
  const double* score;
  const int64_t* pick_off; /* [n_mg+1] */
  const double* pcx;       /* [pick_off[n_mg]] unrounded consensus coordinates */
  const double* pcy;
  const int32_t* box_tier_in;  /* [n_boxes] or NULL */
} rgc_vote_gather_in;
typedef struct rgc_vote_gather_out {
  int32_t n_sub;           /* submitted pseudo-micrographs, micrograph-major, subsets ascending */
  int32_t* sub_mg;         /* [n_sub] */
  int32_t* sub_mask;       /* [n_sub] picker bitmask of the subset */
  int64_t* box_off;        /* [n_sub*t+1] the pseudo-batch's offsets */
  int32_t* box_tier;       /* [n_boxes] after the explain step */
  int32_t* origin;         /* [box_off[n_sub*t]] batch box index of each pseudo-batch box */
  double* x;               /* the pseudo-batch */
  double* y;
  double* score;
} rgc_vote_gather_out;
int rgc_vote_gather(rgc_ctx* ctx, const rgc_vote_gather_in* in, rgc_vote_gather_out* out);

int rgc_parse_files(const char* const* paths, int64_t n_files, int n_threads, rgc_parsed** out);
void rgc_parsed_free(rgc_parsed* p);

/* Native output writer (ABI 5), reference get_cliques.py:204-229: the pickles are emitted in
 * the opcode layout of CPython's pickler for these objects (protocol 5, no FRAME opcodes);
 * the names below come from the installed numpy / scipy.  repic_amd/writers.py enables it
 * only after rgc_pickle_bytes matched pickle.dumps of the same objects. */
typedef struct rgc_pickle_fmt {
  const char* arr_mod;     /* numpy array reduction: module and function ("_frombuffer") */
  const char* arr_fn;
  const char* dtype_mod;   /* numpy.dtype class */
  const char* dtype_cls;
  const char* coo_mod;     /* scipy.sparse coo_matrix class */
  const char* coo_cls;
  int32_t maxprint;        /* coo_matrix().maxprint */
} rgc_pickle_fmt;

typedef struct rgc_write_in {
  const char* out_dir;
  int32_t n_mg;
  int32_t k;
  const char* const* bases;   /* [n_mg] output base names */
  const int64_t* clique_off;  /* [n_mg+1] ranges into the per-clique arrays */
  const int32_t* n_vert;      /* [n_mg] V (rows of the constraint matrix) */
  const int32_t* cc_max;      /* [n_mg] runtime.tsv columns 2-3 */
  const int32_t* cc_cnt;
  const double* seconds;      /* [n_mg] runtime.tsv column 1 */
  const float* w;             /* [C] */
  const float* conf;          /* [C] */
  const int32_t* rows;        /* [C*k] ascending per clique */
  const double* cx;           /* [C] consensus x, y, global id */
  const double* cy;
  const int64_t* cid;
} rgc_write_in;
/* Writes the 5 files of every micrograph (n_threads threads); on an I/O error returns -errno
 * and the failing micrograph in *failed_mg (the lowest of the failing ones). */
int rgc_write_outputs(const rgc_pickle_fmt* fmt, const rgc_write_in* in, int n_threads,
                      int64_t* failed_mg);
/* Bytes of pickle `which` (0 weight_vector, 1 consensus_coords, 2 consensus_confidences,
 * 3 constraint_matrix) of micrograph mg: *len always, copied when cap >= *len. */
int rgc_pickle_bytes(const rgc_pickle_fmt* fmt, const rgc_write_in* in, int mg, int which,
                     uint8_t* buf, int64_t cap, int64_t* len);
/* CPython str(float) (test hook of the runtime.tsv formatting); returns the length. */
int rgc_py_float_repr(double v, char* buf, int cap);

/* ABI 10 — the consensus BOX writer (reference run_ilp.py:126-133): one <base>.box per
 * micrograph from rgc_consensus' pick arrays, lines "<x>\t<y>\t<box>\t<box>\t<conf>\n" with
 * <x>, <y> as str(int(np.rint(v))) prints them (-0.0 -> "0") and <conf> as str(np.float32(v))
 * (rgc_np_float_str).  A micrograph with count -1 (skipped) or 0 gets an empty file. */
typedef struct rgc_box_write_in {
  const char* out_dir;
  int32_t n_mg;
  int64_t box_size;
  const char* const* bases;   /* [n_mg] output base names */
  const int64_t* pick_off;    /* [n_mg] first pick of each micrograph */
  const int64_t* count;       /* [n_mg] picks, or -1: skipped micrograph */
  const double* px;           /* already rounded (np.rint) */
  const double* py;
  const float* pconf;
} rgc_box_write_in;
/* n_threads threads; on an I/O error returns -errno and the lowest failing micrograph. */
int rgc_write_boxes(const rgc_box_write_in* in, int n_threads, int64_t* failed_mg);

/* `repic consensus --members` writer (an additive symbol): per micrograph the <base>.box of
 * rgc_write_boxes and then, from the same task, <base>_members.tsv - the table the reference's
 * run_ilp.py:110-119 builds for --multi_out inputs, with exact picker columns:
 *   header       the k picker names joined by tabs, "\n"
 *   pick rows    row i describes .box line i: for p = 0..k-1 the member's x, y as
 *                str(int(np.rint(v))), then the confidence as str(np.float32(v)): 2k+1 fields
 *   leftovers    for p = 0..k-1 in turn, the segment's leftover boxes in file order: "N/A\tN/A"
 *                in every other picker's columns, x, y in picker p's, then "0.0"
 * Rows are joined with "\n" and the last has none.  A skipped micrograph (count -1) gets its
 * empty .box and no .tsv. */
typedef struct rgc_members_write_in {
  rgc_box_write_in box;       /* the .box files, as for rgc_write_boxes */
  int32_t k;
  const char* header;         /* the header line without its "\n" */
  const double* pmx;          /* [.. * k] members of pick i (an index into px) at i*k+p, rounded */
  const double* pmy;
  const int64_t* seg;         /* [n_mg] micrograph's first segment in left_off (skipped: unused) */
  const int64_t* left_off;    /* leftovers of segment s: [left_off[s], left_off[s+1]) */
  const double* left_x;       /* rounded */
  const double* left_y;
} rgc_members_write_in;
/* n_threads threads; on an I/O error returns -errno, the lowest failing micrograph and in
 * *failed_file which of its files failed (0: .box, 1: _members.tsv). */
int rgc_write_members(const rgc_members_write_in* in, int n_threads, int64_t* failed_mg,
                      int32_t* failed_file);
/* str(numpy.float32(v)) (test hook of the .box confidence column): shortest round-trip float32
 * digits, positional for 1e-4 <= |v| < 1e16 (and 0), else scientific with an exponent of at
 * least two digits; returns the length. */
int rgc_np_float_str(float v, char* buf, int cap);

/* Host test hook (ABI 11): what the launches pass for box_size and threshold t.  An edge is
 * I > *int_cut on the integer layout (I the integer overlap area) and I > *f64_hi on the f64
 * layout; *f64_lo == *f64_hi, the largest f64 I whose reference quotient I / (2 B^2 - I) does
 * not exceed t (no band of undecided areas is left between them).  Returns 0, or a negative
 * code for box_size outside 1..2^26 or t outside [0, 1). */
int rgc_test_ji_cutoff(int64_t box_size, double t, int64_t* int_cut, double* f64_lo,
                       double* f64_hi);
/* Host test hooks for the CPython set-order emulation (pyset.h). */
uint64_t rgc_py_hash_node(double x, double y, int64_t id);
int rgc_py_set_order(const uint64_t* hashes, int n, int8_t* out);
/* Host test hook: the device ILP epilogue of ONE clique (rgc_device.h epilogue<K>), run on
 * the CPU.  Members in picker order; ji[i*k+j] for i < j; ins only used when !set_order.
 * Outputs: consensus member index, node-iteration order (k entries), w, conf.
 * Reference: get_cliques.py:169-190 (median conf / w, weighted-degree consensus). */
int rgc_test_epilogue(int k, const double* x, const double* y, const double* score,
                      const int64_t* ids, const double* ji, int set_order, const uint64_t* ins,
                      int* arg, int8_t* ord, float* w, float* conf);

#ifdef __cplusplus
}
#endif
#endif
