// rgc_run.cpp — rgc_run / rgc_submit / rgc_wait: host orchestration of the batched
// get_cliques pipeline.
//
// rgc_run:
//   1. size-class every micrograph by its box count; each class is one launch of the fused
//      per-micrograph kernel (rgc_fused.hip) with an LDS image sized for the class;
//   2. one sync: read per-micrograph stats and the clique reservation cursor; if the output
//      arrays were too small, grow them and re-run the fused launches (first calls only);
//   3. micrographs too large for LDS (or whose edges overflowed the class's LDS edge
//      capacity) are gathered into a compact sub-batch and run through the multi-kernel
//      pipeline (run_multi, rgc_run_large.cpp), writing after the fused outputs.
// rgc_submit / rgc_wait: the same fused launches enqueued without a host sync when the batch
// allows it (submit_fast), else rgc_run on a worker thread.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <tuple>

#include "rgc_host.h"

using namespace rgc;

// LDS is allocated in 1280-byte blocks, 128 per CU (gfx950, measured with
// tools/probe/lds_occ.hip: 3 workgroups per CU up to 53760 B, 2 above it; the HIP occupancy
// API over-reports 3 up to 54613 B, so it is not used).
constexpr int LDS_BLOCK = 1280;
#ifdef RGC_STAMPS
constexpr int LDS_BLOCKS = 127;   // (diagnostic build: the fused kernel's static LDS counters)
#else
constexpr int LDS_BLOCKS = 128;
#endif
// Micrographs above this many boxes go straight to the large-micrograph route.  Above 2048
// boxes the fused layout uses 2 n grid cells and u16 parents (29 B per box + 2 B per edge),
// so a 4096-box micrograph (C3: ~4k boxes, ~15k edges) runs in one workgroup per CU with room
// for 22k edges; at 4608 boxes ~13k edges still fit.
constexpr int64_t FUSED_MAX_BOXES = 4608;
static int lds_blocks(int bytes) { return (bytes + LDS_BLOCK - 1) / LDS_BLOCK; }

// One fused launch configuration: micrographs of <= nmax boxes, forward-edge capacity ecap,
// dynamic LDS bytes, coordinate width, workgroup size.
struct FusedPlan {
  int nmax = 0, ecap = 0, lds = 0, wg = 0;   // wg: workgroups per CU
  int nt = 512;                              // threads per workgroup
  bool wide = false;
};

// Workgroups per CU the VGPRs of the nt-thread kernel allow (nt / 64 waves per workgroup over
// 4 SIMDs of 512 VGPRs, at most 8 waves per SIMD).
static int vgpr_wg_cap(int k, bool wide, int nt) {
  static int cache[2][MAX_K + 1][5] = {};
  const int slot = nt == 256 ? 0 : nt == 384 ? 1 : nt == 512 ? 2 : nt == 768 ? 3 : 4;
  int& v = cache[wide][k][slot];
  if (!v) {
    const int r = fused_vgprs(k, wide, nt);
    const int waves = r > 0 ? std::min(8, 512 / (((r + 7) / 8) * 8)) : 0;
    v = 1 + waves * 4 / (nt / 64);   // stored + 1 (0 = not computed)
  }
  return v - 1;
}

// The most workgroups per CU that LDS (with ecap >= nmax) and VGPRs allow, then the largest
// edge capacity at that occupancy (free LDS up to the next allocation boundary).  Among the
// compiled workgroup sizes the one with the most resident waves per CU wins (ties: the
// smallest): where LDS admits only one or two workgroups per CU, 768 / 1024 threads put the
// idle SIMD slots to work.  max_wg = 1: the whole 160 KiB (largest ecap).
// RGC_DIAG_NT (experiments only) forces one workgroup size when it is compiled for k.
static bool plan_fused(int k, bool wide, int nmax, int max_wg, FusedPlan* p) {
  const int base = fused_lds_bytes(nmax, 0, wide);
  const int need = lds_blocks(fused_lds_bytes(nmax, nmax, wide));
  if (need > LDS_BLOCKS) return false;
  static const int diag_nt = [] {
    const char* e = getenv("RGC_DIAG_NT");
    return e ? atoi(e) : 0;
  }();
  int w = 0, nt = 512, best_waves = 0;
  for (int cand : {256, 384, 512, 768, 1024}) {
    if (!fused_nt_ok(k, cand) || (diag_nt && fused_nt_ok(k, diag_nt) && cand != diag_nt)) continue;
    const int wc = std::min(std::min(max_wg, vgpr_wg_cap(k, wide, cand)), LDS_BLOCKS / need);
    if (wc < 1) continue;
    if (wc * cand / 64 > best_waves) { best_waves = wc * cand / 64; w = wc; nt = cand; }
  }
  if (w < 1) return false;
  const int budget = (LDS_BLOCKS / w) * LDS_BLOCK;
  int ecap = std::min(65535, (budget - base) / 2);
  while (ecap > nmax && fused_lds_bytes(nmax, ecap, wide) > budget) ecap -= 8;
  p->nmax = nmax;
  p->ecap = ecap;
  p->wide = wide;
  p->wg = w;
  p->nt = nt;
  p->lds = fused_lds_bytes(nmax, ecap, wide);
  return p->lds <= budget;
}

// size class of a micrograph of n boxes (64-box steps to 1024, then 128, then 256)
static int fused_class(int64_t n) {
  if (n <= 1024) return (int)std::max<int64_t>(64, (n + 63) / 64 * 64);
  if (n <= 2048) return (int)((n + 127) / 128 * 128);
  return (int)((n + 255) / 256 * 256);
}

// plan_fused memoised per (k, pass, class); nmax = 0 marks "does not fit"
static const FusedPlan& cached_plan(int k, int pass, int nmax) {
  static std::map<std::tuple<int, int, int>, FusedPlan> memo;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  auto it = memo.find({k, pass, nmax});
  if (it != memo.end()) return it->second;
  FusedPlan p;
  // RGC_DIAG_MAX_WG: occupancy experiments only (caps workgroups per CU; outputs unchanged)
  static const int diag_wg = [] {
    const char* e = getenv("RGC_DIAG_MAX_WG");
    return e ? std::max(1, atoi(e)) : LDS_BLOCKS;
  }();
  if (!plan_fused(k, pass > 0, nmax, pass == 2 ? 1 : diag_wg, &p)) p = FusedPlan();
  return memo.emplace(std::make_tuple(k, pass, nmax), p).first->second;
}


// HBM level-tree slots of the 1024-thread fused launches (K = 4, rgc_fused.hip P4): twice as
// many as the CUs (LDS admits one such workgroup per CU), QG_BYTES each; the slot bitmap is
// zeroed once and every workgroup clears its bit again before it ends.
constexpr int QG_BYTES = 1 << 20;
static int ensure_qg(rgc_ctx* c, FusedArgs& A, int k, int nt) {
  const bool on = nt == 1024 && k == 4;
  if (on && !c->qg_nslots) {
    int ncu = 0;
    HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
    const int ns = (2 * std::max(ncu, 1) + 31) / 32 * 32;
    TRY(ensure_dev(c, D_QG, (size_t)ns * QG_BYTES));
    TRY(ensure_dev(c, D_QGSLOT, (size_t)ns / 8));
    HIPCHK(hipMemsetAsync(c->d[D_QGSLOT].p, 0, (size_t)ns / 8, c->stream));
    c->qg_nslots = ns;
  }
  A.qg_base = on ? D<char>(c, D_QG) : nullptr;
  A.qg_slots = on ? D<uint32_t>(c, D_QGSLOT) : nullptr;
  A.qg_nslots = on ? c->qg_nslots : 0;
  A.qg_bytes = on ? QG_BYTES : 0;
  return 0;
}

// D_MGOUT / H_MGOUT = per-micrograph SoA block, then two cursor slots of CUR_BYTES: a run
// uses slot cur_slot and its kernel zeroes the other one for the next run (no memset packet).
// The cursor pointers of a fused run and its per-micrograph stats block:
struct FusedIo {
  unsigned long long *cur, *clear;
  const unsigned long long* h_cur;   // host copy of cur (after the stats copy)
  int slot;
  MgOut o;
};
static int fused_io(rgc_ctx* c, int n_mg, size_t cur_off, FusedIo* io) {
  TRY(ensure_host(c, H_MGOUT, cur_off + 2 * CUR_BYTES));
  TRY(ensure_dev(c, D_MGOUT, cur_off + 2 * CUR_BYTES));
  TRY(ensure_dev(c, D_TIECNT, (size_t)n_mg * 4));   // (zeroed when it is allocated)
  char* d = D<char>(c, D_MGOUT);
  if (c->slots_at != d || c->slots_off != cur_off) {   // new buffer or layout: zero both slots
    HIPCHK(hipMemsetAsync(d + cur_off, 0, 2 * CUR_BYTES, c->stream));
    c->slots_at = d;
    c->slots_off = cur_off;
    c->cur_slot = 0;
  }
  const int sl = c->cur_slot;
  io->slot = sl;
  io->cur = reinterpret_cast<unsigned long long*>(d + cur_off + sl * CUR_BYTES);
  io->clear = reinterpret_cast<unsigned long long*>(d + cur_off + (1 - sl) * CUR_BYTES);
  io->h_cur = reinterpret_cast<const unsigned long long*>(H<char>(c, H_MGOUT) + cur_off +
                                                           sl * CUR_BYTES);
  io->o = mgout_bind(d, n_mg);
  return 0;
}

// one side copy stream per device for the whole process (created on first use, kept for the
// process's lifetime)
static int shared_copy_stream(int device, hipStream_t* out) {
  static std::mutex mu;
  static std::vector<hipStream_t> streams;
  std::lock_guard<std::mutex> lk(mu);
  if ((int)streams.size() <= device) streams.resize(device + 1, nullptr);
  if (!streams[device]) HIPCHK(hipStreamCreateWithFlags(&streams[device], hipStreamNonBlocking));
  *out = streams[device];
  return 0;
}

// ---------------------------------------------------------------------------- shared steps
// What rgc_run and rgc_submit both read off a batch before anything is enqueued.
struct BatchShape {
  int n_mg = 0, k = 0;
  int64_t N = 0;                         // boxes in the batch
  int64_t nmin = INT64_MAX, nmaxb = 0;   // boxes of the smallest / the largest micrograph
  bool get_cc = false, multi = false, want_members = false, want_edges = false;
  JiCut cut{};                           // the batch's edge threshold as the launches take it
};

rgc_batch_in batch_copy(const rgc_batch_in* in) {
  rgc_batch_in c{};
  std::memcpy(&c, in, offsetof(rgc_batch_in, ji_threshold));
  if (in->flags & RGC_F_JI_THRESHOLD) c.ji_threshold = in->ji_threshold;
  return c;
}

bool batch_threshold(const rgc_batch_in* in, double* t) {
  *t = (in->flags & RGC_F_JI_THRESHOLD) ? in->ji_threshold : JI_DEFAULT;
  return *t >= 0.0 && *t < 1.0;   // (false for NaN)
}

static int64_t mg_boxes(const rgc_batch_in* in, int m) {
  return in->box_off[(int64_t)(m + 1) * in->k] - in->box_off[(int64_t)m * in->k];
}

// nullptr when the batch is valid, else what is wrong with it (rgc_run fails with that text;
// for rgc_submit it is "not a fast-path batch", and the general path reports it)
static const char* batch_shape(const rgc_batch_in* in, BatchShape* b) {
  b->n_mg = in->n_mg;
  b->k = in->k;
  if (b->n_mg < 0) return "n_mg < 0";
  if (b->k < 1 || b->k > MAX_K) return "k (number of pickers) must be in 1..8";
  if (in->box_size > (1LL << 26)) return "box_size too large (> 2^26)";
  double t;
  if (!batch_threshold(in, &t)) return "ji_threshold must be finite and in [0, 1)";
  // (ji_cut bisects, ~90 dependent divisions: kept from the last call while the box size and
  // the threshold stay the same, which is every step of a pipelined run)
  struct Memo { int64_t box = -1; double t = 0.0; JiCut cut{}; };
  static thread_local Memo memo;
  if (memo.box != in->box_size || memo.t != t) memo = {in->box_size, t, ji_cut(in->box_size, t)};
  b->cut = memo.cut;
  b->N = b->n_mg ? in->box_off[(int64_t)b->n_mg * b->k] : 0;
  if (b->N >= (1LL << 31) - 1) return "too many boxes in one batch (>= 2^31)";
  b->get_cc = (in->flags & RGC_F_GET_CC) != 0;
  b->multi = (in->flags & RGC_F_MULTI_OUT) != 0;
  b->want_members = (in->flags & (RGC_F_MEMBERS | RGC_F_MULTI_OUT)) != 0;
  b->want_edges = (in->flags & RGC_F_EDGES) != 0;
  for (int m = 0; m < b->n_mg; ++m) {
    const int64_t nm = mg_boxes(in, m);
    b->nmin = std::min(b->nmin, nm);
    b->nmaxb = std::max(b->nmaxb, nm);
  }
  return nullptr;
}

// Offset of the two cursor slots in D_MGOUT / H_MGOUT, right after the per-micrograph block
// (so one copy returns both).
static size_t cur_off(int n_mg) { return (mgout_bytes(n_mg) + 15) & ~(size_t)15; }

// Per-call plan lookup.  cached_plan takes a process-wide mutex and does a std::map lookup; a
// call sees few distinct (pass, class) pairs, so each is fetched once into this linear list
// and found there afterwards: once per pair per call, never once per micrograph.  (Inline
// storage for every pair there is, 34 classes x 3 passes: rgc_submit builds one per step.)
struct PlanCache {
  int k, n = 0;
  int key[128];                  // cl * 4 + pass (left uninitialised: nothing to pay per step)
  const FusedPlan* plan[128];
  const FusedPlan& get(int pass, int cl) {
    const int ky = cl * 4 + pass;
    for (int i = 0; i < n; ++i)
      if (key[i] == ky) return *plan[i];
    const FusedPlan& p = cached_plan(k, pass, cl);
    if (n < 128) {
      key[n] = ky;
      plan[n++] = &p;
    }
    return p;
  }
};

// The FusedArgs of a run, as far as rgc_run and rgc_submit set them alike.  Left zero for the
// caller: the edge dump (eu / ev / eji / ecap_out), esum_n, wide_list, mg_count, the stats
// hand-off (stats_dev / host_stats / stats_bytes), and per launch nmax / ecap / mg_list /
// stamps (launch_plan sets the first two and the qg_* slots).
static FusedArgs fused_args(rgc_ctx* c, const BatchShape& b, const rgc_batch_in* in,
                            const int32_t* d_bo, const int64_t* d_id, const double* x,
                            const double* y, const double* sc, const FusedIo& io) {
  FusedArgs A{};
  A.k = b.k;
  A.flags = (b.get_cc ? 1 : 0) | (b.multi ? 2 : 0) | (b.want_members ? 32 : 0);
  A.B = (double)in->box_size;
  A.two_b2 = (double)(2 * in->box_size * in->box_size);
  A.cut = b.cut;
  A.box_off = d_bo; A.id_base = d_id;
  A.x = x; A.y = y; A.score = sc; A.o = io.o;
  A.cursor = io.cur; A.cap = c->cap_cliques;
  A.cursor_clear = io.clear;
  A.rows = D<int32_t>(c, D_ROWS); A.w = D<float>(c, D_W); A.conf = D<float>(c, D_CONF);
  A.consensus = D<int32_t>(c, D_CONS);
  A.members = b.want_members ? D<int32_t>(c, D_MEMBERS) : nullptr;
  A.order = b.multi ? D<uint8_t>(c, D_ORDER) : nullptr;
  A.tie_list = D<int32_t>(c, D_TIES);
  A.tie_cap = c->cap_cliques;
  A.tie_cnt = D<int32_t>(c, D_TIECNT);
  A.tie_n = b.n_mg;
  return A;
}

// One fused launch of n_blocks workgroups with plan pl (A.mg_list names their micrographs).
static int launch_plan(rgc_ctx* c, FusedArgs& A, const FusedPlan& pl, int n_blocks) {
  A.nmax = pl.nmax;
  A.ecap = pl.ecap;
  TRY(ensure_qg(c, A, A.k, pl.nt));
  TRY(mark(c, "k_fused"));
  const int le = launch_fused(c->stream, n_blocks, pl.lds, A, pl.wide, pl.nt);
  if (le != 0)
    return fail(std::string("fused kernel launch failed (k=") + std::to_string(A.k) +
                (pl.wide ? ", f64" : ", f32") + " layout, nmax " + std::to_string(pl.nmax) +
                ", lds " + std::to_string(pl.lds) + ", " + std::to_string(pl.nt) +
                " threads): " + (le > 0 ? hipGetErrorString((hipError_t)le) : "unsupported k"));
  return 0;
}

// with RGC_F_TIMING: the event that closes the last section of a fused pass
static int record_tail(rgc_ctx* c) {
  if (!c->timing) return 0;
  if (!c->ev_tail) HIPCHK(hipEventCreate(&c->ev_tail));
  HIPCHK(hipEventRecord(c->ev_tail, c->stream));
  return 0;
}

// *out = zero but for the per-micrograph arrays (the pinned SoA block ho) and the box count
static void bind_stats(rgc_batch_out* out, const MgOut& ho, int64_t n_boxes) {
  std::memset(out, 0, sizeof(*out));
  out->status = ho.status;
  out->cc_max = ho.cc_max;
  out->cc_cnt = ho.cc_cnt;
  out->n_nodes = ho.n_nodes;
  out->n_vert = ho.n_vert;
  out->n_edges_mg = ho.n_edges;
  out->clique_base = ho.clique_base;
  out->clique_cnt = ho.clique_cnt;
  out->n_boxes = n_boxes;
}

// the per-clique arrays: the device outputs, or their pinned host copies
static void bind_cliques(rgc_ctx* c, rgc_batch_out* out, bool host, bool want_members,
                         bool multi) {
  out->rows = host ? H<int32_t>(c, H_ROWS) : D<int32_t>(c, D_ROWS);
  out->w = host ? H<float>(c, H_W) : D<float>(c, D_W);
  out->conf = host ? H<float>(c, H_CONF) : D<float>(c, D_CONF);
  out->consensus = host ? H<int32_t>(c, H_CONS) : D<int32_t>(c, D_CONS);
  out->members = nullptr;
  out->order = nullptr;
  if (want_members) out->members = host ? H<int32_t>(c, H_MEMBERS) : D<int32_t>(c, D_MEMBERS);
  if (multi) out->order = host ? H<uint8_t>(c, H_ORDER) : D<uint8_t>(c, D_ORDER);
}

// ---------------------------------------------------------------------------- rgc_run
// What the steps of one run_impl call share.
struct Run {
  rgc_ctx* c;
  const rgc_batch_in* in;
  rgc_batch_out* out;
  hipStream_t s;
  BatchShape b;
  PlanCache plans;
  size_t cur_off = 0;
  MgOut ho{};                           // the per-micrograph stats, host copy (H_MGOUT)
  const int32_t* d_bo;                  // the inputs on the device: the caller's HBM-resident
  const int64_t* d_id;                  // arrays, or the uploads (upload_inputs)
  const double *x, *y, *sc;
  int32_t* f_ml = nullptr;              // pinned staging of the micrograph lists (3 passes)
  bool all0 = false;                    // one pass-0 launch over the whole batch
  std::vector<int32_t> todo0;           // else: the micrographs pass 0 starts from
  std::vector<int32_t> deferred;        // micrographs for the large-micrograph route
  int64_t fused_total = 0;              // cliques of the fused passes
  int64_t fused_edges = 0;              // RGC_F_EDGES: edges dumped so far
  Run(rgc_ctx* c_, const rgc_batch_in* in_, rgc_batch_out* out_, const BatchShape& b_)
      : c(c_), in(in_), out(out_), s(c_->stream), b(b_), plans{b_.k}, d_bo(in_->dev_box_off),
        d_id(in_->dev_id_base), x(in_->x), y(in_->y), sc(in_->score) {}
  // the steps, in run_impl's order
  int upload_inputs();
  void route_fused();
  int fused_passes();
  int fused_attempt(int attempt, std::vector<int32_t>& todo, bool* overflow);
  int deferred_route();
  int hand_off();
  bool fused_ran() const { return all0 || !todo0.empty(); }
  // size class of micrograph m (0: too large for the fused kernel)
  int mg_class(int m) const {
    const int64_t nm = mg_boxes(in, m);
    return nm <= FUSED_MAX_BOXES ? fused_class(nm) : 0;
  }
};

// Inputs on the device: the caller's HBM-resident arrays, or uploads.
int Run::upload_inputs() {
  const int n_mg = b.n_mg;
  const size_t nbo = (size_t)n_mg * b.k + 1;
  const size_t fstage = nbo * 4 + n_mg * 8 + 3 * (size_t)n_mg * 4 + 64;   // 3 passes of lists
  TRY(ensure_host(c, H_FSTAGE, fstage));
  int32_t* f_bo = H<int32_t>(c, H_FSTAGE);
  int64_t* f_id = reinterpret_cast<int64_t*>(
      (reinterpret_cast<uintptr_t>(f_bo + nbo) + 7) & ~(uintptr_t)7);
  f_ml = reinterpret_cast<int32_t*>(f_id + n_mg);
  // per-micrograph offsets on the device: the caller's HBM-resident copies, or an upload
  const bool dev_meta = (in->flags & RGC_F_DEVICE_META) != 0;
  if (dev_meta && (!in->dev_box_off || !in->dev_id_base))
    return fail("RGC_F_DEVICE_META needs dev_box_off and dev_id_base");
  TRY(ensure_dev(c, D_MGLIST, 3 * (size_t)n_mg * 4 + 4));
  if (!dev_meta) {
    for (size_t i = 0; i < nbo; ++i) f_bo[i] = (int32_t)in->box_off[i];
    std::memcpy(f_id, in->id_base, n_mg * 8);
    TRY(ensure_dev(c, D_FBOXOFF, nbo * 4));
    TRY(ensure_dev(c, D_FIDBASE, n_mg * 8));
    TRY(mark(c, "h2d_meta"));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_FBOXOFF), f_bo, nbo * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_FIDBASE), f_id, n_mg * 8, hipMemcpyHostToDevice, s));
    d_bo = D<int32_t>(c, D_FBOXOFF);
    d_id = D<int64_t>(c, D_FIDBASE);
  }
  if (!(in->flags & RGC_F_DEVICE_INPUTS)) {
    TRY(ensure_dev(c, D_X, b.N * 8));
    TRY(ensure_dev(c, D_Y, b.N * 8));
    TRY(ensure_dev(c, D_S, b.N * 8));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_X), in->x, b.N * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_Y), in->y, b.N * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_S), in->score, b.N * 8, hipMemcpyHostToDevice, s));
    x = D<double>(c, D_X);
    y = D<double>(c, D_Y);
    sc = D<double>(c, D_S);
  }
  return 0;
}

// Which micrographs the fused passes start from.  Fast path (all0): every micrograph fits
// pass 0 and the largest class runs at the occupancy of the smallest (feasibility and
// occupancy are monotone in n) -> one launch over all of them.
void Run::route_fused() {
  const bool no_fused = (in->flags & RGC_F_NO_FUSED) != 0;
  const int n_mg = b.n_mg;
  const int cmin = fused_class(b.nmin), cmax = fused_class(b.nmaxb);
  all0 = !no_fused && n_mg > 0 && b.nmaxb <= FUSED_MAX_BOXES && plans.get(0, cmax).nmax &&
         plans.get(0, cmin).wg == plans.get(0, cmax).wg &&
         plans.get(0, cmin).nt == plans.get(0, cmax).nt;
  if (all0) return;
  todo0.reserve(n_mg);
  for (int m = 0; m < n_mg; ++m) {
    const int cl = mg_class(m);
    if (!no_fused && cl && plans.get(0, cl).nmax) todo0.push_back(m);
    else deferred.push_back(m);
  }
}

// One attempt at the fused passes with the output arrays as they are.  Pass 0: f32-coordinate
// layout at the best occupancy; pass 1: the micrographs it deferred (coordinates not exact in
// f32, or more edges than its ecap) with f64 coordinates; pass 2: the edge-capacity overflows
// of pass 1 with the whole LDS.  Each pass launches once per size class (once in all, all0)
// and ends in one host sync.  todo: what is still deferred; overflow: an output array was too
// small for some micrograph.
int Run::fused_attempt(int attempt, std::vector<int32_t>& todo, bool* overflow) {
  const int n_mg = b.n_mg;
  TRY(ensure_outputs(c, c->cap_cliques, 0, b.k, b.want_members, b.multi));
  if (b.want_edges) TRY(ensure_edges(c, c->cap_edges, 0));
  // this run's cursor slot was zeroed by the previous run's kernel (or at allocation);
  // a regrow attempt re-zeroes it
  FusedIo io;
  TRY(fused_io(c, n_mg, cur_off, &io));
  if (attempt > 0) HIPCHK(hipMemsetAsync(io.cur, 0, CUR_BYTES, s));
  // (esum_n = 0: the host sums the finished micrographs' edges from the stats copy;
  // wide_list = nullptr: the passes are host-driven here)
  FusedArgs A = fused_args(c, b, in, d_bo, d_id, x, y, sc, io);
  A.eu = b.want_edges ? D<int32_t>(c, D_EU) : nullptr;
  A.ev = b.want_edges ? D<int32_t>(c, D_EV) : nullptr;
  A.eji = b.want_edges ? D<double>(c, D_EJIOUT) : nullptr;
  A.ecap_out = c->cap_edges;
#ifdef RGC_STAMPS
  TRY(ensure_dev(c, D_STAMPS, 3 * (size_t)n_mg * rgc::STAMP_SLOTS * 8));
  HIPCHK(hipMemsetAsync(D<void>(c, D_STAMPS), 0, 3 * (size_t)n_mg * rgc::STAMP_SLOTS * 8, s));
#endif
  todo = todo0;
  std::vector<int32_t> left;
  int ml_off = 0;   // mg-list slots used (earlier passes' lists stay intact)
  *overflow = false;
  for (int pass = 0; pass < 3 && (!todo.empty() || (pass == 0 && all0)); ++pass) {
    const bool single = pass == 0 && all0;   // identity list: block b = micrograph b
    // bucket by size class (few classes: linear search of the bucket keys)
    std::vector<int> keys;
    std::vector<std::vector<int32_t>> lists;
    left.clear();
    if (single) {   // (todo is empty: one key, its list stays empty)
      keys.push_back(fused_class(b.nmaxb));
      lists.emplace_back();
    }
    int last = -1;
    for (int32_t m : todo) {
      const int cl = mg_class(m);
      if (!cl || !plans.get(pass, cl).nmax) { left.push_back(m); continue; }
      if (last < 0 || keys[last] != cl) {
        last = (int)(std::find(keys.begin(), keys.end(), cl) - keys.begin());
        if (last == (int)keys.size()) { keys.push_back(cl); lists.emplace_back(); }
      }
      lists[last].push_back(m);
    }
    std::vector<int32_t> by;
    std::vector<size_t> starts;
    for (size_t q = 0; q < keys.size(); ++q) {
      starts.push_back(by.size());
      by.insert(by.end(), lists[q].begin(), lists[q].end());
    }
    if (!by.empty()) {
      std::memcpy(f_ml + ml_off, by.data(), by.size() * 4);
      HIPCHK(hipMemcpyAsync(D<int32_t>(c, D_MGLIST) + ml_off, f_ml + ml_off, by.size() * 4,
                            hipMemcpyHostToDevice, s));
    }
    for (size_t q = 0; q < keys.size(); ++q) {
      A.mg_list = single ? nullptr : D<int32_t>(c, D_MGLIST) + ml_off + starts[q];
#ifdef RGC_STAMPS
      A.stamps = D<unsigned long long>(c, D_STAMPS) + (size_t)(ml_off + starts[q]) * rgc::STAMP_SLOTS;
#endif
      TRY(launch_plan(c, A, plans.get(pass, keys[q]), single ? n_mg : (int)lists[q].size()));
    }
    TRY(mark(c, "k_fused_ties"));
    if (launch_fused_ties(s, A) != 0) return fail("tie kernel launch failed");
    TRY(mark(c, "d2h_stats"));
    HIPCHK(hipMemcpyAsync(H<void>(c, H_MGOUT), D<void>(c, D_MGOUT), cur_off + 2 * CUR_BYTES,
                          hipMemcpyDeviceToHost, s));
    TRY(record_tail(c));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    ml_off += (int)by.size();
    todo.clear();
    for (int32_t i = 0, n = single ? n_mg : (int32_t)by.size(); i < n; ++i) {
      const int32_t m = single ? i : by[i];
      const int stt = ho.status[m];
      if (stt == RGC_ST_OVERFLOW) *overflow = true;
      else if (stt == RGC_ST_DEFER_WIDE || stt == RGC_ST_DEFER) todo.push_back(m);
    }
    for (int32_t m : left) todo.push_back(m);
  }
  fused_total = (int64_t)io.h_cur[0];
  fused_edges = (int64_t)io.h_cur[2];
  // this attempt's launches zeroed the other cursor slot: the next run (or regrow) uses it
  c->cur_slot = 1 - c->cur_slot;
#ifdef RGC_STAMPS
  const size_t n0w = all0 ? (size_t)n_mg : todo0.size();   // pass 0's workgroups
  c->stamps.resize(n0w * rgc::STAMP_SLOTS);
  HIPCHK(hipMemcpy(c->stamps.data(), D<void>(c, D_STAMPS), n0w * rgc::STAMP_SLOTS * 8,
                   hipMemcpyDeviceToHost));
#endif
  return 0;
}

// The fused passes; when an output array was too small, grown arrays and one more attempt
// (first calls only).  What is still deferred joins deferred.
int Run::fused_passes() {
  if (c->cap_cliques < 4096) c->cap_cliques = std::max<int64_t>(4096, b.N);
  if (b.want_edges && c->cap_edges < 4 * b.N + 4096) c->cap_edges = 4 * b.N + 4096;
  for (int attempt = 0; attempt < 2; ++attempt) {
    std::vector<int32_t> todo;
    bool overflow = false;
    TRY(fused_attempt(attempt, todo, &overflow));
    const bool edge_over = b.want_edges && fused_edges > c->cap_edges;
    if (!overflow && fused_total <= c->cap_cliques && !edge_over) {
      for (int32_t m : todo) deferred.push_back(m);
      break;
    }
    if (attempt == 1) return fail("internal: output overflow after regrow");
    if (edge_over) c->cap_edges = fused_edges + fused_edges / 8 + 1024;
    if (overflow || fused_total > c->cap_cliques)   // grow and re-run once
      c->cap_cliques = fused_total + fused_total / 8 + 1024;
    c->n_ev = 0;
  }
  // edges of the micrographs the fused passes finished (the stats were copied after each
  // pass; micrographs never launched hold a previous run's stats, so only launched ones)
  for (int32_t i = 0, n = all0 ? b.n_mg : (int32_t)todo0.size(); i < n; ++i) {
    const int32_t m = all0 ? i : todo0[i];
    if (ho.status[m] < RGC_ST_DEFER) out->n_edges += ho.n_edges[m];
  }
  return 0;
}

// The deferred micrographs as a compact sub-batch through the multi-kernel pipeline: gather,
// run_multi (writing after the fused outputs), index remap, edge dump, stats merge.
int Run::deferred_route() {
  const int k = b.k;
  std::sort(deferred.begin(), deferred.end());
  const int ns = (int)deferred.size();
  std::vector<int64_t> sbo((size_t)ns * k + 1), sid(ns);
  std::vector<int32_t> sbo32((size_t)ns * k + 1);
  int64_t acc = 0;
  for (int i = 0; i < ns; ++i) {
    const int m = deferred[i];
    for (int p = 0; p < k; ++p) {
      sbo[(size_t)i * k + p] = acc;
      acc += in->box_off[(int64_t)m * k + p + 1] - in->box_off[(int64_t)m * k + p];
    }
    sid[i] = in->id_base[m];
  }
  sbo[(size_t)ns * k] = acc;
  for (size_t i = 0; i < sbo.size(); ++i) sbo32[i] = (int32_t)sbo[i];
  // every micrograph deferred (a batch of large micrographs): the sub-batch IS the batch,
  // no gather and no index remap
  const bool ident = ns == b.n_mg;
  const int32_t* orig = nullptr;
  if (!ident) {
    TRY(ensure_dev(c, D_SUBMG, ns * 4));
    TRY(ensure_dev(c, D_SUBX, acc * 8));
    TRY(ensure_dev(c, D_SUBY, acc * 8));
    TRY(ensure_dev(c, D_SUBS, acc * 8));
    TRY(ensure_dev(c, D_ORIG, acc * 4));
    TRY(ensure_dev(c, D_BOXOFF, sbo32.size() * 4));
    HIPCHK(hipMemcpy(D<void>(c, D_SUBMG), deferred.data(), ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D<void>(c, D_BOXOFF), sbo32.data(), sbo32.size() * 4,
                     hipMemcpyHostToDevice));
    TRY(mark(c, "k_gather"));
    launch_gather(s, ns, k, D<int32_t>(c, D_SUBMG), d_bo, D<int32_t>(c, D_BOXOFF),
                  x, y, sc, D<double>(c, D_SUBX), D<double>(c, D_SUBY),
                  D<double>(c, D_SUBS), D<int32_t>(c, D_ORIG));
    HIPCHK(hipStreamSynchronize(s));
    x = D<double>(c, D_SUBX);   // (from here on the sub-batch's)
    y = D<double>(c, D_SUBY);
    sc = D<double>(c, D_SUBS);
    orig = D<int32_t>(c, D_ORIG);
  }
  std::vector<MgStat> sst;
  int64_t Cm = 0, Em = 0;
  TRY(run_multi(c, ns, k, (double)in->box_size, (double)(2 * in->box_size * in->box_size),
                b.cut, b.get_cc, b.multi, b.want_members, b.want_edges, sbo.data(), sid.data(),
                x, y, sc, fused_total, sst, &Cm, &Em));
  if (!ident) {
    TRY(mark(c, "k_remap"));
    launch_remap(s, Cm, k, orig, D<int32_t>(c, D_CONS) + fused_total,
                 b.want_members ? D<int32_t>(c, D_MEMBERS) + fused_total * k : nullptr);
  }
  if (b.want_edges) {
    TRY(ensure_edges(c, fused_edges + Em, fused_edges));
    launch_dump_edges(s, (int)acc, D<int64_t>(c, D_FWDOFF), D<int32_t>(c, D_EDST),
                      D<double>(c, D_EJI), orig, D<int32_t>(c, D_EU) + fused_edges,
                      D<int32_t>(c, D_EV) + fused_edges, D<double>(c, D_EJIOUT) + fused_edges);
    fused_edges += Em;
  }
  for (int i = 0; i < ns; ++i) {
    const int m = deferred[i];
    const MgStat& t = sst[i];
    int stt = t.status;
    if (stt == RGC_OK && t.clique_cnt == 0) stt = RGC_NO_CLIQUES;
    ho.status[m] = stt;
    ho.cc_max[m] = t.cc_max;
    ho.cc_cnt[m] = t.cc_cnt;
    ho.n_nodes[m] = t.n_nodes;
    ho.n_vert[m] = t.n_vert;
    ho.n_edges[m] = t.n_edges;
    ho.clique_base[m] = t.clique_base;
    ho.clique_cnt[m] = stt == RGC_OK ? t.clique_cnt : 0;
  }
  out->n_cliques += Cm;
  out->n_edges += Em;
  return 0;
}

// Pinned host copies of the first n elements of device arrays: the host buffers grown first,
// then the copies enqueued.
struct HostCopy {
  int h, d;       // H_ / D_ buffer ids
  size_t bytes;   // per element
  bool on;
};
static int host_copies(rgc_ctx* c, std::initializer_list<HostCopy> arrays, int64_t n) {
  for (const auto& a : arrays)
    if (a.on) TRY(ensure_host(c, a.h, n * a.bytes));
  for (const auto& a : arrays)
    if (a.on && n)
      HIPCHK(hipMemcpyAsync(c->h[a.h].p, c->d[a.d].p, n * a.bytes, hipMemcpyDeviceToHost, c->stream));
  return 0;
}

// The per-clique arrays into *out; host copies of the edge dump (RGC_F_EDGES) and of the
// per-clique arrays (RGC_F_HOST_OUTPUTS) when asked for.
int Run::hand_off() {
  const size_t k = b.k;
  if (b.want_edges) {
    TRY(host_copies(c, {{H_EU, D_EU, 4, true}, {H_EV, D_EV, 4, true}, {H_EJIOUT, D_EJIOUT, 8, true}},
                    fused_edges));
    HIPCHK(hipStreamSynchronize(s));
    c->n_edge_dump = fused_edges;
  }
  const bool host = (in->flags & RGC_F_HOST_OUTPUTS) != 0;
  if (host) {
    TRY(mark(c, "d2h"));
    TRY(host_copies(c, {{H_ROWS, D_ROWS, k * 4, true}, {H_W, D_W, 4, true}, {H_CONF, D_CONF, 4, true},
                        {H_CONS, D_CONS, 4, true}, {H_MEMBERS, D_MEMBERS, k * 4, b.want_members},
                        {H_ORDER, D_ORDER, k, b.multi}}, out->n_cliques));
  }
  bind_cliques(c, out, host, b.want_members, b.multi);
  return 0;
}

int run_impl(rgc_ctx* c, const rgc_batch_in* in, rgc_batch_out* out) {
  BatchShape b;
  if (const char* bad = batch_shape(in, &b)) return fail(bad);
  const int n_mg = b.n_mg;
  c->n_edge_dump = 0;
  TRY(tiles_refresh(c));
  c->timing = (in->flags & RGC_F_TIMING) != 0;
  c->n_ev = 0;

  // per-micrograph outputs: pinned SoA block, filled by one copy of the device mirror
  Run r(c, in, out, b);
  r.cur_off = cur_off(n_mg);
  TRY(ensure_host(c, H_MGOUT, r.cur_off + 2 * CUR_BYTES));
  r.ho = mgout_bind(H<void>(c, H_MGOUT), n_mg);
  bind_stats(out, r.ho, b.N);
  if (n_mg == 0) return 0;
  if (b.k == 1) {  // no picker pairs -> no edges -> reference ValueError on every micrograph
    std::memset(H<void>(c, H_MGOUT), 0, mgout_bytes(n_mg));
    std::fill(r.ho.status, r.ho.status + n_mg, RGC_NO_EDGES);
    return 0;
  }

  TRY(r.upload_inputs());
  r.route_fused();
  if (r.fused_ran()) TRY(r.fused_passes());
  // what is still deferred (or too large for LDS) runs through the multi-kernel path
  out->n_cliques = r.fused_total;
  if (!r.deferred.empty()) TRY(r.deferred_route());
  TRY(r.hand_off());

  // nothing enqueued since the fused passes' last sync -> no second round trip; their tail
  // event closes the timeline
  const bool tail_work = !r.fused_ran() || !r.deferred.empty() || (in->flags & RGC_F_HOST_OUTPUTS);
  HIPCHK(hipGetLastError());
  if (tail_work) {
    TRY(mark(c, "end"));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return collect_times(c, false, !tail_work);
}

// ---------------------------------------------------------------------------- rgc_submit
// rgc_submit's fast path: a batch whose micrographs all take pass 0 of the fused kernel with
// HBM-resident inputs and offsets and device outputs is enqueued (kernels + stats copy +
// event) without waiting.  Returns 1 when enqueued, 0 when the batch needs the general path
// (run synchronously by the caller), < 0 on error.
//
// Two launch-grouping policies, on purpose.  rgc_run (fused_attempt) launches once per size
// class, or once for the whole batch when all0 holds: each launch gets the LDS image and edge
// capacity of its own class, and the host sync after each pass lets it send what overflowed
// to the next pass.  rgc_submit launches once per occupancy group (below): fewer launches per
// step and no host sync, at the group's largest class's edge capacity; what that defers falls
// back to rgc_run at rgc_wait.  Merging them would change launch geometry and which
// micrographs defer.
static int submit_fast(rgc_ctx* c, const rgc_batch_in* in) {
  const uint32_t flags = in->flags;
  const uint32_t need = RGC_F_DEVICE_INPUTS | RGC_F_DEVICE_META;
  const uint32_t deny = RGC_F_HOST_OUTPUTS | RGC_F_EDGES | RGC_F_NO_FUSED;
  if ((flags & need) != need || (flags & deny) || in->n_mg <= 0 || in->k < 2) return 0;
  if (!in->dev_box_off || !in->dev_id_base) return 0;
  BatchShape b;
  if (batch_shape(in, &b) || b.nmaxb > FUSED_MAX_BOXES) return 0;
  const int n_mg = b.n_mg, k = b.k;
  PlanCache plans{k};
  // launch groups: micrographs whose size classes share a plan's occupancy and workgroup
  // size run as one launch at the group's largest class; several groups (C3 / C4 classes
  // straddle an occupancy step) launch back to back over HBM micrograph lists, still without
  // a host sync (deferrals show up in rgc_wait, which falls back to the general path)
  struct Grp {
    int wg, nt, cl;
    std::vector<int32_t> mg;
  };
  std::vector<Grp> grp;
  {
    const FusedPlan& pl = plans.get(0, fused_class(b.nmaxb));
    const FusedPlan& p0 = plans.get(0, fused_class(b.nmin));
    if (!pl.nmax || !p0.nmax) return 0;
    if (p0.wg == pl.wg && p0.nt == pl.nt) {
      grp.push_back({pl.wg, pl.nt, fused_class(b.nmaxb), {}});
    } else {
      for (int m = 0; m < n_mg; ++m) {
        const int cl = fused_class(mg_boxes(in, m));
        const FusedPlan* p = &plans.get(0, cl);
        if (!p->nmax) return 0;
        Grp* g = nullptr;
        for (auto& e : grp)
          if (e.wg == p->wg && e.nt == p->nt) g = &e;
        if (!g) {
          grp.push_back({p->wg, p->nt, cl, {}});
          g = &grp.back();
        }
        g->cl = std::max(g->cl, cl);
        g->mg.push_back(m);
      }
      for (const auto& g : grp)   // the group's largest class must keep its occupancy
        if (plans.get(0, g.cl).wg != g.wg || plans.get(0, g.cl).nt != g.nt) return 0;
    }
  }
  hipStream_t s = c->stream;
  c->timing = (flags & RGC_F_TIMING) != 0;
  c->n_ev = 0;
  c->n_edge_dump = 0;
  const size_t co = cur_off(n_mg);
  if (c->cap_cliques < 4096) c->cap_cliques = std::max<int64_t>(4096, b.N);
  TRY(ensure_outputs(c, c->cap_cliques, 0, k, b.want_members, b.multi));
  FusedIo io;
  TRY(fused_io(c, n_mg, co, &io));
  FusedArgs A = fused_args(c, b, in, in->dev_box_off, in->dev_id_base, in->x, in->y, in->score, io);
  A.esum_n = n_mg;   // k_fused_ties sums the edges of the finished micrographs (cursor[1])
  // the last run on this context deferred micrographs to the f64 layout: this one appends its
  // DEFER_WIDE micrographs to a device list and runs their f64 pass right after, on the
  // stream (no host round trip, no rerun of the batch through the general path)
  const FusedPlan* pw = c->wide_hint ? &plans.get(1, fused_class(b.nmaxb)) : nullptr;
  if (pw && !pw->nmax) pw = nullptr;
  if (pw) {
    TRY(ensure_dev(c, D_WIDELIST, (size_t)n_mg * 4));
    A.wide_list = D<int32_t>(c, D_WIDELIST);
  }
#ifdef RGC_STAMPS
  return 0;   // the diagnostic build times through rgc_run only
#endif
  int32_t* d_ml = nullptr;
  if (grp.size() > 1) {   // micrograph lists, group after group, through the pinned stage
    TRY(ensure_host(c, H_FSTAGE, (size_t)n_mg * 4));
    TRY(ensure_dev(c, D_MGLIST, (size_t)n_mg * 4));
    int32_t* h_ml = H<int32_t>(c, H_FSTAGE);
    size_t o = 0;
    for (const auto& g : grp) {
      std::memcpy(h_ml + o, g.mg.data(), g.mg.size() * 4);
      o += g.mg.size();
    }
    d_ml = D<int32_t>(c, D_MGLIST);
    HIPCHK(hipMemcpyAsync(d_ml, h_ml, (size_t)n_mg * 4, hipMemcpyHostToDevice, s));
  }
  size_t o = 0;
  for (const auto& g : grp) {
    A.mg_list = grp.size() > 1 ? d_ml + o : nullptr;
    o += g.mg.size();
    TRY(launch_plan(c, A, plans.get(0, g.cl), grp.size() > 1 ? (int)g.mg.size() : n_mg));
  }
  if (pw) {
    FusedArgs Aw = A;
    Aw.mg_list = A.wide_list;
    Aw.mg_count = io.cur + 5;
    Aw.wide_list = nullptr;
    TRY(launch_plan(c, Aw, *pw, n_mg));
  }
  // every micrograph's stats to the host from the ties kernel (the run's last kernel) when
  // the caller wants them with every run
  const bool stats_in_ties = !(flags & RGC_F_LAZY_STATS) && A.tie_list && A.tie_cap > 0;
  if (stats_in_ties) {
    A.stats_dev = D<char>(c, D_MGOUT);
    A.host_stats = H<char>(c, H_MGOUT);
    A.stats_bytes = (int64_t)co;
  }
  TRY(mark(c, "k_fused_ties"));
  if (launch_fused_ties(s, A) != 0) return fail("tie kernel launch failed (submit)");
  c->pend_slot = io.slot;
  c->cur_slot = 1 - c->cur_slot;   // the launch zeroes the other slot: the next run's
  TRY(record_tail(c));
  // The stats copy.  A lazy run's (its 128-B totals) on the launch stream: the next run on
  // THIS context is submitted after rgc_wait, and other contexts launch on streams of their
  // own (bench.py: one stream per context), whose hardware queues a side copy stream per
  // context would share (3-4 % with two or three contexts in flight,
  // profiles/r05w_ab_copy_on_stream.txt).  Every micrograph's stats (48 B each): written to
  // the pinned host block by the ties kernel itself (stats_in_ties).  As a copy they were a
  // blit kernel: on the launch stream it waited for CUs behind the other contexts'
  // workgroups (C2: 0.39 -> 0.56 ms per step), on a side stream after an event its wait
  // packet sat in a hardware queue that, depending on how a process's streams mapped onto
  // the 4 queues, a launch stream could share (14.3-14.8 M against 25 M micrographs/s on
  // half the processes measured, profiles/r06az_*).
  if (!c->ev_sub) HIPCHK(hipEventCreateWithFlags(&c->ev_sub, hipEventDisableTiming));
  if (stats_in_ties || (flags & RGC_F_LAZY_STATS)) {
    // the run's totals (a lazy run's other stats: rgc_fetch_stats; a non-lazy run's: the
    // ties kernel wrote them)
    const size_t so = co + (size_t)io.slot * CUR_BYTES;
    HIPCHK(hipMemcpyAsync(H<char>(c, H_MGOUT) + so, D<char>(c, D_MGOUT) + so, CUR_BYTES,
                          hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(c->ev_sub, s));
  } else {
    if (!c->copy_set) {
      TRY(shared_copy_stream(c->device, &c->copy_stream));
      c->copy_set = true;
    }
    if (!c->ev_k) HIPCHK(hipEventCreateWithFlags(&c->ev_k, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_k, s));
    HIPCHK(hipStreamWaitEvent(c->copy_stream, c->ev_k, 0));
    HIPCHK(hipMemcpyAsync(H<void>(c, H_MGOUT), D<void>(c, D_MGOUT), co + 2 * CUR_BYTES,
                          hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(hipEventRecord(c->ev_sub, c->copy_stream));
  }
  HIPCHK(hipGetLastError());
  return 1;
}

// completes a submit_fast run: 1 = outputs in *out; 0 = some micrograph needs another pass or
// the outputs overflowed (the caller re-runs the batch with rgc_run's general path)
static int wait_fast(rgc_ctx* c, rgc_batch_out* out) {
  const rgc_batch_in* in = &c->pin;
  const int n_mg = in->n_mg;
  HIPCHK(hipEventSynchronize(c->ev_sub));
  const MgOut ho = mgout_bind(H<void>(c, H_MGOUT), n_mg);
  const unsigned long long* h_cur = reinterpret_cast<const unsigned long long*>(
      H<char>(c, H_MGOUT) + cur_off(n_mg) + c->pend_slot * CUR_BYTES);
  bool again = (int64_t)h_cur[0] > c->cap_cliques || h_cur[4] != 0;
  // the next submit on this context runs the f64 pass on the device when this batch had
  // micrographs for it
  c->wide_hint = h_cur[5] != 0;
  const bool lazy = (in->flags & RGC_F_LAZY_STATS) != 0;
  for (int m = 0; m < n_mg && !again && !lazy; ++m) again = ho.status[m] >= RGC_ST_DEFER;
  if (again) return 0;
  c->lazy_n_mg = lazy ? n_mg : -1;   // rgc_fetch_stats copies them on demand
  bind_stats(out, ho, in->box_off[(int64_t)n_mg * in->k]);
  out->n_cliques = (int64_t)h_cur[0];
  out->n_edges = (int64_t)h_cur[1];
  bind_cliques(c, out, false, (in->flags & (RGC_F_MEMBERS | RGC_F_MULTI_OUT)) != 0,
               (in->flags & RGC_F_MULTI_OUT) != 0);
  TRY(collect_times(c, false, true));
  return 1;
}

extern "C" {

int rgc_run(rgc_ctx* c, const rgc_batch_in* in, rgc_batch_out* out) {
  if (!c || !in || !out) return fail("null argument");
  if (c->pend) return fail("rgc_run: a submitted run awaits rgc_wait on this context");
  HIPCHK(hipSetDevice(c->device));
  c->lazy_n_mg = -1;
  return run_impl(c, in, out);
}

int rgc_submit(rgc_ctx* c, const rgc_batch_in* in) {
  if (!c || !in) return fail("null argument");
  if (c->pend) return fail("rgc_submit: a submitted run awaits rgc_wait on this context");
  HIPCHK(hipSetDevice(c->device));
  c->lazy_n_mg = -1;
  double t;
  if (!batch_threshold(in, &t)) return fail("ji_threshold must be finite and in [0, 1)");
  c->pin = batch_copy(in);
  const int r = submit_fast(c, in);
  if (r < 0) return r;
  c->pend = true;
  c->pend_fast = r == 1;
  if (!c->pend_fast) {
    // the general path syncs on the host once per clique level: on a worker thread, so the
    // caller's next submit (another context, another stream) overlaps this run's device work
    // and its host round trips; rgc_wait joins it.  (No thread: the run happens here.)
    auto general = [c] {
      c->pend_rc = run_impl(c, &c->pin, &c->pend_out);
      if (c->pend_rc != 0) c->pend_err = rgc_last_error();   // (the message is per thread)
    };
    try {
      c->worker = std::thread([c, general] {
        if (hipSetDevice(c->device) == hipSuccess) return general();
        c->pend_rc = fail("hipSetDevice failed on the submit worker");
        c->pend_err = rgc_last_error();
      });
    } catch (...) {
      general();
    }
  }
  return 0;
}

int rgc_wait(rgc_ctx* c, rgc_batch_out* out) {
  if (!c || !out) return fail("null argument");
  if (!c->pend) return fail("rgc_wait: nothing submitted on this context");
  HIPCHK(hipSetDevice(c->device));
  c->pend = false;
  if (!c->pend_fast) {
    if (c->worker.joinable()) c->worker.join();
    *out = c->pend_out;
    if (c->pend_rc != 0) (void)fail(c->pend_err);   // (the message is per thread)
    return c->pend_rc;
  }
  const int r = wait_fast(c, out);
  if (r < 0) return r;
  if (r == 0) return run_impl(c, &c->pin, out);   // deferrals / overflow: the general path
  return 0;
}

int rgc_fetch_stats(rgc_ctx* c) {
  if (!c) return fail("null ctx");
  if (c->lazy_n_mg < 0) return 0;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(H<void>(c, H_MGOUT), D<void>(c, D_MGOUT), mgout_bytes(c->lazy_n_mg),
                   hipMemcpyDeviceToHost));
  c->lazy_n_mg = -1;
  return 0;
}

}  // extern "C"
