// rgc_consensus.cpp — rgc_consensus (ABI 10): rgc_run, then the set-packing solver on the
// run's device outputs (rgc_pick.hip k_pick_cols fills the solver's inputs in HBM) and the
// ordered picks (k_pick_select / k_pick_emit): get_cliques + run_ilp without the files in
// between.  rgc_pick_select is the pick stage alone.  rgc_consensus_members adds the members of
// every written pick and each picker's leftovers (members_stage); rgc_pick_members is the pick
// and members stages alone.
#include <cmath>
#include <cstring>

#include "rgc_host.h"

using namespace rgc;

// The per-micrograph host block of the pick stage (PickHost, rgc_host.h)
int pick_host(rgc_ctx* c, int n_mg, PickHost* h) {
  TRY(ensure_host(c, H_PK_MG, ((size_t)n_mg + 1) * 8 + (size_t)n_mg * 24 + 16));
  h->pick_off = H<int64_t>(c, H_PK_MG);
  h->primal = reinterpret_cast<double*>(h->pick_off + n_mg + 1);
  h->gap = h->primal + n_mg;
  h->sel_cnt = reinterpret_cast<int32_t*>(h->gap + n_mg);
  h->status = h->sel_cnt + n_mg;
  h->pick_off[0] = 0;   // (the device scan overwrites it: an empty batch's stays)
  return 0;
}

// Selection, pick_off scan and emit (rgc_pick.hip) of a batch whose inputs A already names;
// the picks and the per-micrograph counts land in the context's host buffers.
int pick_stage(rgc_ctx* c, rgc::PickArgs& A, const PickHost& h, int64_t* n_picked) {
  hipStream_t s = c->stream;
  const int n_mg = A.n_mg;
  *n_picked = 0;
  if (n_mg == 0) return 0;
  TRY(ensure_dev(c, D_PK_SEL, A.n_cols * 4));
  TRY(ensure_dev(c, D_PK_SELCNT, (size_t)n_mg * 4));
  TRY(ensure_dev(c, D_PK_PRIMAL, (size_t)n_mg * 8));
  TRY(ensure_dev(c, D_PK_OFF, ((size_t)n_mg + 1) * 8));
  A.sel = D<int32_t>(c, D_PK_SEL);
  A.sel_cnt = D<int32_t>(c, D_PK_SELCNT);
  A.primal = D<double>(c, D_PK_PRIMAL);
  A.pick_off = D<int64_t>(c, D_PK_OFF);
  rgc::launch_pick_select(s, A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h.pick_off, A.pick_off, ((size_t)n_mg + 1) * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h.sel_cnt, A.sel_cnt, (size_t)n_mg * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h.primal, A.primal, (size_t)n_mg * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int64_t np = h.pick_off[n_mg];
  if (np < 0 || np > A.n_cols) return fail("pick_off scan out of range");
  TRY(ensure_dev(c, D_PK_PX, np * 8));
  TRY(ensure_dev(c, D_PK_PY, np * 8));
  TRY(ensure_dev(c, D_PK_PCONF, np * 4));
  TRY(ensure_dev(c, D_PK_PCOL, np * 4));
  TRY(ensure_host(c, H_PK_PX, np * 8));
  TRY(ensure_host(c, H_PK_PY, np * 8));
  TRY(ensure_host(c, H_PK_PCONF, np * 4));
  TRY(ensure_host(c, H_PK_PCOL, np * 4));
  *n_picked = np;
  if (np == 0) return 0;
  A.px = D<double>(c, D_PK_PX);
  A.py = D<double>(c, D_PK_PY);
  A.pconf = D<float>(c, D_PK_PCONF);
  A.pcol = D<int32_t>(c, D_PK_PCOL);
  rgc::launch_pick_emit(s, A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(H<void>(c, H_PK_PX), A.px, np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(H<void>(c, H_PK_PY), A.py, np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(H<void>(c, H_PK_PCONF), A.pconf, np * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(H<void>(c, H_PK_PCOL), A.pcol, np * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

// the pick arrays of the last pick_stage (host), into either entry point's output struct
template <typename Out>
static void bind_picks(rgc_ctx* c, Out* out) {
  out->px = H<double>(c, H_PK_PX);
  out->py = H<double>(c, H_PK_PY);
  out->pconf = H<float>(c, H_PK_PCONF);
  out->pcol = H<int32_t>(c, H_PK_PCOL);
}

// The --members stage after pick_stage (whose device outputs A still names): the members of
// every written pick and each segment's leftovers (rgc_pick.hip k_pick_clique_mark /
// k_pick_members / k_pick_left), into the context's host buffers.  box_off: host, [n_mg k + 1];
// status: rgc_run's per-micrograph status, or nullptr (every micrograph ok); dev_members: the
// cliques' members in HBM.  *up / *down: what crossed the bus here.
static int members_stage(rgc_ctx* c, const rgc::PickArgs& A, const PickHost& h, int64_t np,
                         const int64_t* box_off, const int32_t* status,
                         const int32_t* dev_members, rgc_members_out* mem, int64_t* up,
                         int64_t* down) {
  hipStream_t s = c->stream;
  const int n_mg = A.n_mg, k = A.k;
  const int64_t S = (int64_t)n_mg * k;
  *up = *down = 0;
  std::memset(mem, 0, sizeof(*mem));
  // segment metadata: box_off, left_off (8 B each), then the ok bytes
  const size_t meta_bytes = ((size_t)S + 1) * 16 + (size_t)n_mg;
  TRY(ensure_host(c, H_PM_META, meta_bytes));
  int64_t* hbo = H<int64_t>(c, H_PM_META);
  int64_t* hlo = hbo + S + 1;
  uint8_t* hok = reinterpret_cast<uint8_t*>(hlo + S + 1);
  mem->left_off = hlo;
  hlo[0] = 0;
  if (n_mg == 0) return 0;
  std::memcpy(hbo, box_off, ((size_t)S + 1) * 8);
  for (int m = 0; m < n_mg; ++m) {
    hok[m] = !status || status[m] == RGC_OK;
    const int64_t keep = h.pick_off[m + 1] - h.pick_off[m];
    for (int p = 0; p < k; ++p) {
      const int64_t seg = (int64_t)m * k + p, boxes = hbo[seg + 1] - hbo[seg];
      // (the picks of a packing have disjoint members: one box of every picker each)
      if (hok[m] && boxes < keep)
        return fail("consensus members: chosen columns of micrograph " + std::to_string(m) +
                    " share a box (" + std::to_string(keep) + " picks, " + std::to_string(boxes) +
                    " boxes of picker " + std::to_string(p) + ")");
      hlo[seg + 1] = hlo[seg] + (hok[m] ? boxes - keep : 0);
    }
  }
  const int64_t N = hbo[S], L = hlo[S];
  const size_t seg_bytes = (2 * (size_t)S + 1) * 4;
  TRY(ensure_dev(c, D_PM_META, meta_bytes));
  TRY(ensure_dev(c, D_PM_INPICK, N));
  TRY(ensure_dev(c, D_PM_INCL, N));
  TRY(ensure_dev(c, D_PM_X, np * k * 8));
  TRY(ensure_dev(c, D_PM_Y, np * k * 8));
  TRY(ensure_dev(c, D_PM_LX, L * 8));
  TRY(ensure_dev(c, D_PM_LY, L * 8));
  TRY(ensure_dev(c, D_PM_SEG, seg_bytes));
  TRY(ensure_host(c, H_PM_X, np * k * 8));
  TRY(ensure_host(c, H_PM_Y, np * k * 8));
  TRY(ensure_host(c, H_PM_LX, L * 8));
  TRY(ensure_host(c, H_PM_LY, L * 8));
  TRY(ensure_host(c, H_PM_SEG, seg_bytes));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_PM_META), hbo, meta_bytes, hipMemcpyHostToDevice, s));
  if (N) {
    HIPCHK(hipMemsetAsync(D<void>(c, D_PM_INPICK), 0, N, s));
    HIPCHK(hipMemsetAsync(D<void>(c, D_PM_INCL), 0, N, s));
  }
  HIPCHK(hipMemsetAsync(D<void>(c, D_PM_SEG), 0, seg_bytes, s));
  rgc::PickMemArgs M{};
  M.n_mg = n_mg;
  M.k = k;
  M.n_cols = A.n_cols;
  M.n_picked = np;
  M.col_off = A.col_off;
  M.src_base = A.src_base;
  M.pick_off = A.pick_off;
  M.pcol = A.pcol;
  M.members = dev_members;
  M.box_off = D<int64_t>(c, D_PM_META);
  M.left_off = M.box_off + S + 1;
  M.ok = reinterpret_cast<const uint8_t*>(M.left_off + S + 1);
  M.bx = A.bx;
  M.by = A.by;
  M.in_pick = D<uint8_t>(c, D_PM_INPICK);
  M.in_clique = D<uint8_t>(c, D_PM_INCL);
  M.pmx = D<double>(c, D_PM_X);
  M.pmy = D<double>(c, D_PM_Y);
  M.left_x = D<double>(c, D_PM_LX);
  M.left_y = D<double>(c, D_PM_LY);
  M.left_cnt = D<int32_t>(c, D_PM_SEG);
  M.clique_cnt = M.left_cnt + S;
  M.bad = M.clique_cnt + S;
  rgc::launch_pick_members(s, M);
  HIPCHK(hipGetLastError());
  rgc::launch_pick_left(s, M);
  HIPCHK(hipGetLastError());
  if (np) {
    HIPCHK(hipMemcpyAsync(H<void>(c, H_PM_X), M.pmx, np * k * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(H<void>(c, H_PM_Y), M.pmy, np * k * 8, hipMemcpyDeviceToHost, s));
  }
  if (L) {
    HIPCHK(hipMemcpyAsync(H<void>(c, H_PM_LX), M.left_x, L * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(H<void>(c, H_PM_LY), M.left_y, L * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipMemcpyAsync(H<void>(c, H_PM_SEG), M.left_cnt, seg_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *up = (int64_t)meta_bytes;
  *down = np * k * 16 + L * 16 + (int64_t)seg_bytes;
  const int32_t* hseg = H<int32_t>(c, H_PM_SEG);
  if (hseg[2 * S]) return fail("consensus members: a clique member lies outside its picker's boxes");
  for (int64_t seg = 0; seg < S; ++seg)
    if (hseg[seg] != hlo[seg + 1] - hlo[seg])
      return fail("consensus members: chosen columns of micrograph " + std::to_string(seg / k) +
                  " share a box (picker " + std::to_string(seg % k) + ": " +
                  std::to_string(hseg[seg]) + " boxes in no pick, " +
                  std::to_string(hlo[seg + 1] - hlo[seg]) + " expected)");
  mem->pmx = H<double>(c, H_PM_X);
  mem->pmy = H<double>(c, H_PM_Y);
  mem->left_x = H<double>(c, H_PM_LX);
  mem->left_y = H<double>(c, H_PM_LY);
  mem->in_clique = H<int32_t>(c, H_PM_SEG) + S;
  return 0;
}

void ilp_mg_status(const uint8_t* exact, const double* gap, int64_t j0, int64_t j1, double primal,
                   int32_t* status, double* rel_gap) {
  bool all_opt = true, heur = false, nodel = false;
  double g = 0.0;
  for (int64_t j = j0; j < j1; ++j) {
    all_opt = all_opt && exact[j] == RGC_ILP_OPTIMAL;
    heur = heur || exact[j] == RGC_ILP_HEURISTIC;
    nodel = nodel || exact[j] == RGC_ILP_NODE_LIMIT;
    g += gap[j];
  }
  int st = RGC_ILP_GAP_OK;
  if (all_opt) st = RGC_ILP_OPTIMAL;
  else if (g <= 1e-4 * std::fabs(primal)) st = RGC_ILP_GAP_OK;
  else if (heur) st = RGC_ILP_HEURISTIC;
  else if (nodel) st = RGC_ILP_NODE_LIMIT;
  *status = st;
  *rel_gap = primal > 0 ? g / primal : (g == 0 ? 0.0 : HUGE_VAL);
}

// rgc_consensus (mem == nullptr) and rgc_consensus_members
int consensus_impl(rgc_ctx* c, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                          rgc_consensus_out* out, rgc_members_out* mem) {
  if (!c || !in || !opts || !out) return fail("null argument");
  if (c->pend) return fail("rgc_consensus: a submitted run awaits rgc_wait on this context");
  if (in->flags & RGC_F_MULTI_OUT)
    return fail("rgc_consensus: RGC_F_MULTI_OUT is not supported (run_ilp raises on --multi_out "
                "inputs)");
  HIPCHK(hipSetDevice(c->device));
  c->lazy_n_mg = -1;
  std::memset(out, 0, sizeof(*out));
  rgc_batch_in bi = batch_copy(in);
  bi.flags |= opts->flags & RGC_F_TIMING;
  bi.flags &= ~(uint32_t)RGC_F_LAZY_STATS;
  if (mem) bi.flags |= RGC_F_MEMBERS;
  if (!(bi.flags & RGC_F_TIMING)) {
    c->times.clear();
    c->time_names.clear();
  }
  TRY(run_impl(c, &bi, &out->run));
  c->n_ev = 0;   // (run_impl has turned its events into c->times; the stages below follow them)
  const int n_mg = bi.n_mg, k = bi.k;
  const rgc_batch_out& R = out->run;
  hipStream_t s = c->stream;
  PickHost h;
  TRY(pick_host(c, n_mg, &h));
  out->pick_off = h.pick_off;
  out->sel_cnt = h.sel_cnt;
  out->ilp_status = h.status;
  out->ilp_gap = h.gap;
  int64_t mem_up = 0, mem_down = 0;
  if (n_mg == 0) {
    rgc::PickArgs A0{};
    A0.k = k;
    return mem ? members_stage(c, A0, h, 0, nullptr, nullptr, nullptr, mem, &mem_up, &mem_down)
               : 0;
  }

  // per-micrograph metadata, prepared here and uploaded: columns packed in micrograph order
  TRY(ensure_host(c, H_PK_META, (3 * (size_t)n_mg + 1) * 8));
  int64_t* col_off = H<int64_t>(c, H_PK_META);
  int64_t* src_base = col_off + n_mg + 1;
  int64_t* row_base = src_base + n_mg;
  int64_t nc = 0, nr = 0;
  for (int m = 0; m < n_mg; ++m) {
    const bool ok = R.status[m] == RGC_OK && R.clique_cnt[m] > 0;
    col_off[m] = nc;
    src_base[m] = ok ? R.clique_base[m] : 0;
    row_base[m] = nr;
    if (ok) {
      if (R.clique_base[m] < 0 || R.clique_base[m] + R.clique_cnt[m] > R.n_cliques)
        return fail("rgc_consensus: clique range out of bounds");
      nc += R.clique_cnt[m];
      nr += R.n_vert[m];
    }
  }
  col_off[n_mg] = nc;
  if (nc >= INT32_MAX || nr >= INT32_MAX) return fail("n_cols / n_rows out of range");
  const size_t meta_bytes = (3 * (size_t)n_mg + 1) * 8;
  TRY(ensure_dev(c, D_PK_META, meta_bytes));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_META), col_off, meta_bytes, hipMemcpyHostToDevice, s));

  rgc::PickArgs A{};
  A.n_mg = n_mg;
  A.k = k;
  A.n_cols = nc;
  A.num_particles = opts->num_particles;
  A.col_off = D<int64_t>(c, D_PK_META);
  A.src_base = A.col_off + n_mg + 1;
  A.row_base = A.src_base + n_mg;
  // (device copies of the run's outputs, whether or not host copies were asked for; the
  // D_IL_* / D_PK_* workspace is disjoint from them and from the input x / y: ensure_dev
  // grows one id at a time)
  A.rows = D<int32_t>(c, D_ROWS);
  A.w = D<float>(c, D_W);
  A.conf = D<float>(c, D_CONF);
  A.cons = D<int32_t>(c, D_CONS);
  A.bx = (bi.flags & RGC_F_DEVICE_INPUTS) ? bi.x : D<double>(c, D_X);
  A.by = (bi.flags & RGC_F_DEVICE_INPUTS) ? bi.y : D<double>(c, D_Y);

  std::vector<uint8_t> hx((size_t)nc), hex((size_t)nc);
  std::vector<double> hgap((size_t)nc, 0.0);
  c->fix_fetch_bytes = 0;
  if (nc > 0) {
    TRY(ensure_dev(c, D_IL_CPTR, (nc + 1) * 8));
    TRY(ensure_dev(c, D_IL_ROW, nc * k * 4));
    TRY(ensure_dev(c, D_IL_W, nc * 8));
    TRY(ensure_dev(c, D_PK_COLMG, nc * 4));
    TRY(ensure_dev(c, D_PK_X, nc));
    A.col_ptr = D<int64_t>(c, D_IL_CPTR);
    A.row_idx = D<int32_t>(c, D_IL_ROW);
    A.w64 = D<double>(c, D_IL_W);
    A.col_mg = D<int32_t>(c, D_PK_COLMG);
    TRY(mark(c, "k_pick_cols"));
    rgc::launch_pick_cols(s, A);
    HIPCHK(hipGetLastError());
    rgc_ilp_in si{};
    si.n_cols = nc;
    si.n_rows = nr;
    si.node_limit = opts->node_limit;
    TRY(ilp_solve_rec(c, &si, hx.data(), hex.data(), hgap.data(), 0, k));
    // the final packing, uploaded once for the emit stage
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_X), hx.data(), nc, hipMemcpyHostToDevice, s));
  }
  A.x = D<uint8_t>(c, D_PK_X);
  TRY(mark(c, "k_pick_emit"));
  TRY(pick_stage(c, A, h, &out->n_picked));
  bind_picks(c, out);
  if (mem) {
    TRY(mark(c, "k_pick_members"));
    TRY(members_stage(c, A, h, out->n_picked, bi.box_off, R.status, D<int32_t>(c, D_MEMBERS), mem,
                      &mem_up, &mem_down));
  }
  TRY(mark(c, "end"));
  HIPCHK(hipStreamSynchronize(s));

  // per-micrograph status and relative gap, reduced as repic_amd.ilp.mg_status does
  for (int m = 0; m < n_mg; ++m)
    ilp_mg_status(hex.data(), hgap.data(), col_off[m], col_off[m + 1], h.primal[m], &h.status[m],
                  &h.gap[m]);

  // what crossed the bus in this call (the solver's per-column x / status / gap included)
  const int64_t N = R.n_boxes;
  int64_t up = (int64_t)meta_bytes + nc;
  if (!(bi.flags & RGC_F_DEVICE_INPUTS)) up += 3 * N * 8;
  if (!(bi.flags & RGC_F_DEVICE_META)) up += ((int64_t)n_mg * k + 1) * 4 + (int64_t)n_mg * 8;
  int64_t down = (int64_t)mgout_bytes(n_mg) + nc * 10 + ((int64_t)n_mg + 1) * 8 +
                 (int64_t)n_mg * 12 + out->n_picked * 24 + c->fix_fetch_bytes;
  if (bi.flags & RGC_F_HOST_OUTPUTS) {
    down += R.n_cliques * ((int64_t)k * 4 + 12);
    if (bi.flags & RGC_F_MEMBERS) down += R.n_cliques * (int64_t)k * 4;
  }
  out->h2d_bytes = up + mem_up;
  out->d2h_bytes = down + mem_down;

  return collect_times(c, true, false);   // (after run_impl's sections)
}

extern "C" {

int rgc_pick_select(rgc_ctx* c, const rgc_pick_in* in, rgc_pick_out* out) {
  if (!c || !in || !out) return fail("null argument");
  if (c->pend) return fail("rgc_pick_select: a submitted run awaits rgc_wait on this context");
  if (in->n_mg < 0 || (in->n_mg > 0 && !in->col_off)) return fail("bad n_mg / col_off");
  HIPCHK(hipSetDevice(c->device));
  std::memset(out, 0, sizeof(*out));
  const int n_mg = in->n_mg;
  PickHost h;
  TRY(pick_host(c, n_mg, &h));
  out->pick_off = h.pick_off;
  if (n_mg == 0) return 0;
  if (in->col_off[0] != 0) return fail("col_off must start at 0");
  for (int m = 0; m < n_mg; ++m)
    if (in->col_off[m + 1] < in->col_off[m]) return fail("col_off must not decrease");
  const int64_t nc = in->col_off[n_mg];
  if (nc >= INT32_MAX) return fail("too many columns");
  if (nc > 0 && (!in->x || !in->conf || !in->cx || !in->cy)) return fail("null column array");
  hipStream_t s = c->stream;
  TRY(ensure_dev(c, D_PK_META, ((size_t)n_mg + 1) * 8));
  TRY(ensure_dev(c, D_PK_X, nc));
  TRY(ensure_dev(c, D_PK_CONF, nc * 4));
  TRY(ensure_dev(c, D_PK_CX, nc * 8));
  TRY(ensure_dev(c, D_PK_CY, nc * 8));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_META), in->col_off, ((size_t)n_mg + 1) * 8,
                        hipMemcpyHostToDevice, s));
  if (nc) {
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_X), in->x, nc, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_CONF), in->conf, nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_CX), in->cx, nc * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_CY), in->cy, nc * 8, hipMemcpyHostToDevice, s));
  }
  rgc::PickArgs A{};
  A.n_mg = n_mg;
  A.k = 1;
  A.n_cols = nc;
  A.num_particles = in->num_particles;
  A.col_off = D<int64_t>(c, D_PK_META);
  A.conf = D<float>(c, D_PK_CONF);
  A.bx = D<double>(c, D_PK_CX);
  A.by = D<double>(c, D_PK_CY);
  A.x = D<uint8_t>(c, D_PK_X);
  TRY(pick_stage(c, A, h, &out->n_picked));
  bind_picks(c, out);
  return 0;
}

int rgc_consensus(rgc_ctx* c, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                  rgc_consensus_out* out) {
  return consensus_impl(c, in, opts, out, nullptr);
}

int rgc_consensus_members(rgc_ctx* c, const rgc_batch_in* in, const rgc_consensus_opts* opts,
                          rgc_consensus_out* out, rgc_members_out* mem) {
  if (!mem) return fail("null argument");
  return consensus_impl(c, in, opts, out, mem);
}

int rgc_pick_members(rgc_ctx* c, const rgc_pick_members_in* in, rgc_pick_out* out,
                     rgc_members_out* mem) {
  if (!c || !in || !out || !mem) return fail("null argument");
  if (c->pend) return fail("rgc_pick_members: a submitted run awaits rgc_wait on this context");
  const int n_mg = in->n_mg, k = in->k;
  if (k < 1 || k > rgc::MAX_K) return fail("k must be in 1..8");
  if (n_mg < 0 || !in->col_off || !in->box_off) return fail("bad n_mg / null offsets");
  const int64_t S = (int64_t)n_mg * k;
  if (in->col_off[0] != 0 || in->box_off[0] != 0) return fail("offsets must start at 0");
  for (int m = 0; m < n_mg; ++m)
    if (in->col_off[m + 1] < in->col_off[m]) return fail("col_off must not decrease");
  for (int64_t i = 0; i < S; ++i)
    if (in->box_off[i + 1] < in->box_off[i]) return fail("box_off must not decrease");
  const int64_t nc = in->col_off[n_mg], N = in->box_off[S];
  if (nc >= INT32_MAX || N >= INT32_MAX) return fail("too many columns / boxes");
  if (nc > 0 && (!in->x || !in->conf || !in->cons || !in->members)) return fail("null column array");
  if (N > 0 && (!in->bx || !in->by)) return fail("null box array");
  for (int m = 0; m < n_mg; ++m)
    for (int64_t j = in->col_off[m]; j < in->col_off[m + 1]; ++j) {
      if (in->cons[j] < in->box_off[(int64_t)m * k] || in->cons[j] >= in->box_off[(int64_t)(m + 1) * k])
        return fail("cons index outside its micrograph");
      for (int p = 0; p < k; ++p) {
        const int64_t b = in->members[j * k + p], seg = (int64_t)m * k + p;
        if (b < in->box_off[seg] || b >= in->box_off[seg + 1])
          return fail("member index outside its (micrograph, picker) range");
      }
    }
  HIPCHK(hipSetDevice(c->device));
  std::memset(out, 0, sizeof(*out));
  PickHost h;
  TRY(pick_host(c, n_mg, &h));
  out->pick_off = h.pick_off;
  rgc::PickArgs A{};
  A.n_mg = n_mg;
  A.k = k;
  int64_t up = 0, down = 0;
  if (n_mg == 0) return members_stage(c, A, h, 0, nullptr, nullptr, nullptr, mem, &up, &down);
  hipStream_t s = c->stream;
  TRY(ensure_dev(c, D_PK_META, ((size_t)n_mg + 1) * 8));
  TRY(ensure_dev(c, D_PK_X, nc));
  TRY(ensure_dev(c, D_PK_CONF, nc * 4));
  TRY(ensure_dev(c, D_PM_CONS, nc * 4));
  TRY(ensure_dev(c, D_PM_MEMB, nc * k * 4));
  TRY(ensure_dev(c, D_PK_CX, N * 8));
  TRY(ensure_dev(c, D_PK_CY, N * 8));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_META), in->col_off, ((size_t)n_mg + 1) * 8,
                        hipMemcpyHostToDevice, s));
  if (nc) {
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_X), in->x, nc, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_CONF), in->conf, nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PM_CONS), in->cons, nc * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PM_MEMB), in->members, nc * k * 4, hipMemcpyHostToDevice, s));
  }
  if (N) {
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_CX), in->bx, N * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_CY), in->by, N * 8, hipMemcpyHostToDevice, s));
  }
  A.n_cols = nc;
  A.num_particles = in->num_particles;
  A.col_off = D<int64_t>(c, D_PK_META);
  A.conf = D<float>(c, D_PK_CONF);
  A.cons = D<int32_t>(c, D_PM_CONS);
  A.bx = D<double>(c, D_PK_CX);
  A.by = D<double>(c, D_PK_CY);
  A.x = D<uint8_t>(c, D_PK_X);
  TRY(pick_stage(c, A, h, &out->n_picked));
  bind_picks(c, out);
  return members_stage(c, A, h, out->n_picked, in->box_off, nullptr, D<int32_t>(c, D_PM_MEMB), mem,
                       &up, &down);
}

}  // extern "C"
