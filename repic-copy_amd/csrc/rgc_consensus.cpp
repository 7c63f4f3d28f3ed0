// rgc_consensus.cpp — rgc_consensus (ABI 10): rgc_run, then the set-packing solver on the
// run's device outputs (rgc_pick.hip k_pick_cols fills the solver's inputs in HBM) and the
// ordered picks (k_pick_select / k_pick_emit): get_cliques + run_ilp without the files in
// between.  rgc_pick_select is the pick stage alone.
#include <cmath>
#include <cstring>

#include "rgc_host.h"

using namespace rgc;

// The per-micrograph host block of the pick stage (H_PK_MG): pick_off, primal, gap (8 B
// each), then sel_cnt and the ILP status (4 B each).
struct PickHost {
  int64_t* pick_off;
  double* primal;
  double* gap;
  int32_t* sel_cnt;
  int32_t* status;
};
static int pick_host(rgc_ctx* c, int n_mg, PickHost* h) {
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
static int pick_stage(rgc_ctx* c, rgc::PickArgs& A, const PickHost& h, int64_t* n_picked) {
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
  if (n_mg == 0) return 0;

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
  TRY(mark(c, "end"));
  HIPCHK(hipStreamSynchronize(s));

  // per-micrograph status and relative gap, reduced as repic_amd.ilp.mg_status does
  for (int m = 0; m < n_mg; ++m) {
    bool all_opt = true, heur = false, nodel = false;
    double g = 0.0;
    for (int64_t j = col_off[m]; j < col_off[m + 1]; ++j) {
      all_opt = all_opt && hex[j] == RGC_ILP_OPTIMAL;
      heur = heur || hex[j] == RGC_ILP_HEURISTIC;
      nodel = nodel || hex[j] == RGC_ILP_NODE_LIMIT;
      g += hgap[j];
    }
    const double primal = h.primal[m];
    int st = RGC_ILP_GAP_OK;
    if (all_opt) st = RGC_ILP_OPTIMAL;
    else if (g <= 1e-4 * std::fabs(primal)) st = RGC_ILP_GAP_OK;
    else if (heur) st = RGC_ILP_HEURISTIC;
    else if (nodel) st = RGC_ILP_NODE_LIMIT;
    h.status[m] = st;
    h.gap[m] = primal > 0 ? g / primal : (g == 0 ? 0.0 : HUGE_VAL);
  }

  // what crossed the bus in this call (the solver's per-column x / status / gap included)
  const int64_t N = R.n_boxes;
  int64_t up = (int64_t)meta_bytes + nc;
  if (!(bi.flags & RGC_F_DEVICE_INPUTS)) up += 3 * N * 8;
  if (!(bi.flags & RGC_F_DEVICE_META)) up += ((int64_t)n_mg * k + 1) * 4 + (int64_t)n_mg * 8;
  int64_t down = (int64_t)mgout_bytes(n_mg) + nc * 10 + ((int64_t)n_mg + 1) * 8 +
                 (int64_t)n_mg * 12 + out->n_picked * 24 + c->fix_fetch_bytes;
  if (bi.flags & RGC_F_HOST_OUTPUTS) down += R.n_cliques * ((int64_t)k * 4 + 12);
  out->h2d_bytes = up;
  out->d2h_bytes = down;

  return collect_times(c, true, false);   // (after run_impl's sections)
}

}  // extern "C"
