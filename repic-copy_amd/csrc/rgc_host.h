// rgc_host.h — private to the host orchestration files (not installed): the context, its
// grow-only arena and timing events, and the few functions that cross files.  The host files
// are compiled with -fvisibility=hidden, so nothing declared here is exported from
// librepic_gc.so; the C ABI and the kernel launchers keep default visibility.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/repic_gc.h"
#include "rgc_kernels.h"
#pragma GCC visibility pop

// sets the calling thread's error message (rgc_last_error) and returns -1
int fail(const std::string& msg);
#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e_));                   \
  } while (0)
#define TRY(expr)           \
  do {                      \
    int r_ = (expr);        \
    if (r_ != 0) return r_; \
  } while (0)

enum DevBufId {
  // fused path / whole batch
  D_FBOXOFF, D_FIDBASE, D_MGLIST, D_MGOUT, D_X, D_Y, D_S,
  // outputs
  D_ROWS, D_W, D_CONF, D_CONS, D_MEMBERS, D_ORDER,
  // multi-kernel path (sub-batch)
  D_SUBMG, D_SUBX, D_SUBY, D_SUBS, D_ORIG, D_STAMPS,
  D_BOXOFF, D_GRID, D_CELLSTART, D_SX, D_SY, D_SBOX, D_SPICK, D_SMG, D_BMG,
  D_BPICK, D_FWDCNT, D_FWDOFF, D_TILES, D_TOTAL, D_EDST, D_EJI, D_PARENT, D_HASEDGE, D_CSIZE,
  D_STAT, D_INSKEY, D_COMPMIN, D_CCOUNT, D_COFF, D_INCL, D_VLIST, D_VSORT, D_VROW, D_BOFF, D_RLO, D_ADJG, D_RBOUND, D_RFLAG, D_DFSMG, D_ROOTBOX, D_EXLIST,
  D_LCNT, D_LOFF, D_LROOT0, D_LROOT1, D_LM0, D_LM1, D_LP0, D_LP1, D_PK,
  // HBM level-tree slots of the 1024-thread fused launches (K >= 4)
  D_QG, D_QGSLOT,
  // tie entries of the fused launches and their per-micrograph counts (k_fused_ties)
  D_TIES, D_TIECNT,
  // RGC_F_EDGES test hook
  D_EU, D_EV, D_EJIOUT,
  // score_detections raster
  D_SC_BOX, D_SC_GOFF, D_SC_POFF, D_SC_TP, D_SC_TR, D_SC_TW, D_SC_CNT,
  // ... and its threshold sweep's keep table
  D_SC_KEEP,
  // particle-level matching (rgc_match.hip): layout, per-box state, per-pair edges and results
  D_MT_BOX, D_MT_BASE, D_MT_NGT, D_MT_WMAX, D_MT_STATE, D_MT_ETOT, D_MT_EBASE, D_MT_ADJ, D_MT_TP,
  D_MT_STAT,
  // ... and its threshold sweep's keep table and per-threshold sizes
  D_MT_KEEP, D_MT_TPS,
  // run_ilp set packing
  D_IL_CPTR, D_IL_ROW, D_IL_W, D_IL_REP, D_IL_PAR, D_IL_ROOT, D_IL_CSIZE, D_IL_RCNT, D_IL_RCUR,
  D_IL_RPTR, D_IL_RCOLS, D_IL_CID, D_IL_CN, D_IL_COFF, D_IL_CCUR, D_IL_MEM, D_IL_LOC, D_IL_SCR,
  D_IL_BIG, D_IL_NBIG, D_IL_WSCR, D_IL_X, D_IL_EX, D_IL_RLOC, D_IL_CERT, D_IL_KEY, D_IL_ST,
  D_IL_RMAX, D_IL_OWN, D_IL_LAM, D_IL_GRAD, D_IL_CS, D_IL_CNT, D_IL_GAP, D_IL_STSAVE,
  D_IL_FS, D_IL_FSCNT, D_IL_FSKEEP, D_LBUCKET, D_WIDELIST,
  // consensus hand-off (rgc_pick.hip)
  D_PK_META, D_PK_COLMG, D_PK_SEL, D_PK_SELCNT, D_PK_PRIMAL, D_PK_OFF, D_PK_X, D_PK_PX, D_PK_PY,
  D_PK_PCONF, D_PK_PCOL, D_PK_CONF, D_PK_CX, D_PK_CY,
  // ... and its --members stage: segment metadata (box_off, left_off, ok), the two mark arrays,
  // member and leftover coordinates, per-segment counts (+ the bad-member flag), and the hook's
  // uploaded cons / members
  D_PM_META, D_PM_INPICK, D_PM_INCL, D_PM_X, D_PM_Y, D_PM_LX, D_PM_LY, D_PM_SEG, D_PM_CONS,
  D_PM_MEMB,
  // greedy NMS (rgc_nms.hip): layout, coordinates in priority and in x order, per-box state,
  // per-segment edges and results
  D_NM_OFF, D_NM_NS, D_NM_XY, D_NM_SXY, D_NM_SIDX, D_NM_STATE, D_NM_ETOT, D_NM_EBASE, D_NM_ADJ,
  D_NM_KEEP, D_NM_KEPT, D_NM_STAT,
  // consensus --min_pickers (rgc_vote.hip): the full batch's offsets and box tiers, per-segment
  // counts, the pseudo-batch (segment sources and found counts, offsets, x / y / score, origin),
  // its pseudo-micrograph table, the tier's packed per-column arrays, per-micrograph column
  // offsets, the tier's per-pick arrays, the bad-index flag, and the hook's uploaded boxes / picks
  D_VT_BOXOFF, D_VT_TIER, D_VT_SEGCNT, D_VT_PSEG, D_VT_PBOXOFF, D_VT_GX, D_VT_GY, D_VT_GS,
  D_VT_ORIGIN, D_VT_QMETA, D_VT_CW, D_VT_CCONF, D_VT_CCONS, D_VT_CMEMB, D_VT_CMASK, D_VT_COLOFF,
  D_VT_PCX, D_VT_PCY, D_VT_PW, D_VT_PMASK, D_VT_PMEMB, D_VT_BAD, D_VT_HXYS, D_VT_HPOFF,
  // picker agreement (rgc_agree.hip): offsets, finite counts, launch list, coordinates in x
  // order with their indices, then the outputs: masks, partners, their JI, the pair matrices
  D_AG_OFF, D_AG_NS, D_AG_SEG, D_AG_SXY, D_AG_SIDX, D_AG_SUP, D_AG_PART, D_AG_PJI, D_AG_PAIR,
  D_COUNT
};
enum HostBufId {
  H_FSTAGE, H_STAGE, H_TOTAL, H_MGOUT, H_STAT, H_MGOFF, H_ROWS, H_W, H_CONF, H_CONS, H_MEMBERS,
  H_ORDER, H_EU, H_EV, H_EJIOUT,
  // consensus: per-micrograph block (metadata upload staging, then pick_off / sel_cnt /
  // primal / ilp_status / ilp_gap) and the pick arrays
  H_PK_META, H_PK_MG, H_PK_PX, H_PK_PY, H_PK_PCONF, H_PK_PCOL,
  // consensus --members: segment metadata staging (then left_off), member and leftover
  // coordinates, per-segment counts
  H_PM_META, H_PM_X, H_PM_Y, H_PM_LX, H_PM_LY, H_PM_SEG,
  // consensus --min_pickers: the per-micrograph block (tier k's run stats, pick_off, the ILP
  // summary, per-tier counts), the pick block, box_tier, staging of counts and per-pick arrays,
  // and the gather hook's outputs
  H_VT_MG, H_VT_PICK, H_VT_BOXTIER, H_VT_STAGE, H_VT_SUB, H_VT_ORIGIN, H_VT_GXYS,
  // rgc_agreement: one block (pair matrices, partner_ji, partner, support)
  H_AG_OUT, H_COUNT
};

struct Buf {
  void* p = nullptr;
  size_t cap = 0;
};

// device cursors after the per-micrograph block: [0] cliques [1] edges of finished
// micrographs [2] edge-dump reservation (RGC_F_EDGES) [4] deferrals [5] f64-pass micrographs
constexpr size_t CUR_BYTES = 128;

struct rgc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  Buf d[D_COUNT];
  Buf h[H_COUNT];
  std::vector<hipEvent_t> events;
  std::vector<const char*> ev_names;
  int n_ev = 0;
  bool timing = false;
  std::vector<float> times;
  std::vector<const char*> time_names;
  int64_t cap_cliques = 0;   // capacity of the per-clique output arrays
  int64_t cap_edges = 0;     // RGC_F_EDGES: capacity of the edge dump
  int64_t n_edge_dump = 0;   // RGC_F_EDGES: edges of the last run (host copies in H_EU..)
  int cur_slot = 0;          // device cursor slot of the next run (the other one is zeroed)
  void* slots_at = nullptr;  // D_MGOUT address whose cursor slots are known to be zeroed
  size_t slots_off = 0;      // ... at this offset
  int pend_slot = 0;         // cursor slot of the submitted run
  int lazy_n_mg = -1;        // micrographs of the last lazy-stats run not yet fetched
  hipEvent_t ev_tail = nullptr;   // timing: recorded after a fused pass's last enqueued work
  std::vector<uint64_t> stamps;   // diagnostic build only
  // rgc_submit / rgc_wait: one run in flight per context
  bool pend = false;       // a submitted run awaits rgc_wait
  bool pend_fast = false;  // it is the single fused launch (else it already ran: pend_rc/out)
  int pend_rc = 0;
  rgc_batch_in pin{};      // the submitted batch (caller keeps its arrays alive until rgc_wait)
  rgc_batch_out pend_out{};
  hipEvent_t ev_sub = nullptr;   // after the submitted run's stats copy
  int qg_nslots = 0;             // HBM level-tree slots allocated (ensure_qg)
  // rgc_submit: stream of the per-micrograph stats copy (non-lazy runs).  Unless the caller
  // names one (rgc_ctx_set_copy_stream, ABI 9), the process-wide copy stream of the device,
  // shared by every context: streams beyond GPU_MAX_HW_QUEUES (4) share hardware queues
  bool copy_set = false;
  hipStream_t copy_stream = nullptr;
  bool wide_hint = false;   // rgc_submit: the last batch had micrographs for the f64 layout
  hipEvent_t ev_k = nullptr;           // rgc_submit: after the fused launch
  uint64_t tiles_epoch = 0;      // scan_epoch_count() when D_TILES was last zeroed
  // rgc_submit's general path (host syncs per clique level) runs here; rgc_wait joins it
  std::thread worker;
  std::string pend_err;          // the worker's error message (g_err is per thread)
  int64_t fix_fetch_bytes = 0;   // rgc_consensus: CSC bytes fetched for reduced-cost fixing
  int64_t nms_h2d = 0, nms_d2h = 0;   // rgc_nms: bytes the last call copied (rgc_nms_last_bytes)
  int64_t agree_h2d = 0, agree_d2h = 0;   // rgc_agreement: likewise (rgc_agreement_last_bytes)
};

// ---- arena, events (rgc_ctx.cpp)
int ensure_dev(rgc_ctx* c, int id, size_t bytes, size_t keep = 0);
int ensure_host(rgc_ctx* c, int id, size_t bytes);
int tiles_refresh(rgc_ctx* c);
// Grow the per-clique output arrays to `need` cliques, keeping the first `keep` cliques.
int ensure_outputs(rgc_ctx* c, int64_t need, int64_t keep, int k, bool members, bool multi);
// Grow the RGC_F_EDGES dump arrays to `need` edges, keeping the first `keep`.
int ensure_edges(rgc_ctx* c, int64_t need, int64_t keep);
// with RGC_F_TIMING: an event on the stream that opens the section `name`
int mark(rgc_ctx* c, const char* name);
// with RGC_F_TIMING: the marks since n_ev = 0 become c->times / c->time_names, one section per
// interval between consecutive marks.  keep: append to the sections already there (else they
// are replaced); tail: the last mark's section runs to ev_tail (else the last mark only
// closes the one before it).
int collect_times(rgc_ctx* c, bool keep, bool tail);
// RGC_F_TIMING of the entry points that time a few launches of one call (rgc_nms,
// rgc_agreement): events that live as long as the call ...
struct CallEvents {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~CallEvents() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
// ... and the section between two of them appended to c->times as `name`
int section_time(rgc_ctx* c, hipEvent_t e0, hipEvent_t e1, const char* name);

template <typename T>
inline T* D(rgc_ctx* c, int id) { return reinterpret_cast<T*>(c->d[id].p); }
template <typename T>
inline T* H(rgc_ctx* c, int id) { return reinterpret_cast<T*>(c->h[id].p); }

// ---- the routes (rgc_run.cpp, rgc_run_large.cpp, rgc_ilp_host.cpp)
int run_impl(rgc_ctx* c, const rgc_batch_in* in, rgc_batch_out* out);
// A batch descriptor as its own copy.  ji_threshold is appended to the struct (ABI 11) and read
// only under RGC_F_JI_THRESHOLD: a caller built against the earlier layout passes a shorter
// struct, so the copy takes the earlier layout's bytes and the field only with the flag.
rgc_batch_in batch_copy(const rgc_batch_in* in);
// The batch's Jaccard threshold (0.3 without the flag); false: not a finite value in [0, 1)
bool batch_threshold(const rgc_batch_in* in, double* t);
// the multi-kernel pipeline on a (sub-)batch of device arrays (rgc_run_large.cpp)
int run_multi(rgc_ctx* c, int n_mg, int k, double B, double two_b2, const rgc::JiCut& cut,
              int get_cc, int multi,
              bool want_members, bool want_ji, const int64_t* box_off, const int64_t* id_base,
              const double* x, const double* y, const double* sc, int64_t out_base,
              std::vector<rgc::MgStat>& st_out, int64_t* C_out, int64_t* E_out);
// The device set-packing solver with reduced-cost fixing (depth 0 from the callers).  dev_k > 0:
// the CSC arrays are already in D_IL_CPTR / D_IL_ROW / D_IL_W with dev_k rows per column.
int ilp_solve_rec(rgc_ctx* c, const rgc_ilp_in* in, uint8_t* x, uint8_t* exact, double* gap,
                  int depth, int dev_k = 0);

// ---- rgc_consensus and its pick stage (rgc_consensus.cpp), shared with rgc_vote_host.cpp
// rgc_consensus (mem == nullptr) and rgc_consensus_members
int consensus_impl(rgc_ctx* c, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                   rgc_consensus_out* out, rgc_members_out* mem);
// The per-micrograph host block of the pick stage (H_PK_MG): pick_off, primal, gap (8 B
// each), then sel_cnt and the ILP status (4 B each).
struct PickHost {
  int64_t* pick_off;
  double* primal;
  double* gap;
  int32_t* sel_cnt;
  int32_t* status;
};
int pick_host(rgc_ctx* c, int n_mg, PickHost* h);
// Selection, pick_off scan and emit (rgc_pick.hip) of a batch whose inputs A already names;
// the picks and the per-micrograph counts land in the context's host buffers.
int pick_stage(rgc_ctx* c, rgc::PickArgs& A, const PickHost& h, int64_t* n_picked);
// A micrograph's ILP status and relative gap from its columns' [j0, j1) component statuses and
// gaps and its packing value, reduced as repic_amd.ilp.mg_status does.
void ilp_mg_status(const uint8_t* exact, const double* gap, int64_t j0, int64_t j1, double primal,
                   int32_t* status, double* rel_gap);
