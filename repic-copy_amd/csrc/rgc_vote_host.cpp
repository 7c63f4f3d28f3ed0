// rgc_vote_host.cpp — rgc_consensus_tiers (`repic consensus --min_pickers`) and its test hook
// rgc_vote_gather (kernels: rgc_vote.hip).  Tier k is consensus_impl as it is; every lower tier
// marks the boxes the picks so far explain, gathers the rest into one pseudo-batch (a
// pseudo-micrograph per micrograph and picker subset), runs it through run_impl, packs the
// columns of a micrograph's subsets jointly (ilp_solve_rec on device inputs) and emits the picks
// with the pick stage of rgc_consensus.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "rgc_host.h"

using namespace rgc;

namespace {

constexpr int64_t VOTE_BOX_MAX = (int64_t)1 << 26;

// the subsets of t of k pickers as bitmasks, in ascending order of the picker-index tuple
std::vector<int> picker_subsets(int k, int t) {
  std::vector<int> out, idx((size_t)t);
  for (int i = 0; i < t; ++i) idx[i] = i;
  for (;;) {
    int mask = 0;
    for (int i : idx) mask |= 1 << i;
    out.push_back(mask);
    int i = t - 1;
    while (i >= 0 && idx[i] == k - t + i) --i;
    if (i < 0) break;
    ++idx[i];
    for (int j = i + 1; j < t; ++j) idx[j] = idx[j - 1] + 1;
  }
  return out;
}

// The full batch on the device as the vote kernels see it (D_VT_BOXOFF, D_VT_TIER, D_VT_SEGCNT).
// tier_in: the box tiers to start from (host), or nullptr: all 0.
int vote_setup(rgc_ctx* c, int n_mg, int k, const int64_t* box_off, int64_t box_size, double thr,
               const double* dx, const double* dy, const double* ds, const int32_t* tier_in,
               VoteArgs* V, int64_t* up) {
  hipStream_t s = c->stream;
  const int64_t S = (int64_t)n_mg * k, N = box_off[S];
  TRY(ensure_dev(c, D_VT_BOXOFF, ((size_t)S + 1) * 8));
  TRY(ensure_dev(c, D_VT_TIER, (size_t)N * 4));
  TRY(ensure_dev(c, D_VT_SEGCNT, (size_t)S * 4));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_BOXOFF), box_off, ((size_t)S + 1) * 8,
                        hipMemcpyHostToDevice, s));
  *up += (S + 1) * 8;
  if (N && tier_in) {
    HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_TIER), tier_in, (size_t)N * 4, hipMemcpyHostToDevice, s));
    *up += N * 4;
  } else if (N) {
    HIPCHK(hipMemsetAsync(D<void>(c, D_VT_TIER), 0, (size_t)N * 4, s));
  }
  *V = VoteArgs{};
  V->n_mg = n_mg;
  V->k = k;
  V->B = (double)box_size;
  V->two_b2 = (double)(2 * box_size * box_size);
  V->thr = thr;
  V->box_off = D<int64_t>(c, D_VT_BOXOFF);
  V->bx = dx;
  V->by = dy;
  V->bs = ds;
  V->box_tier = D<int32_t>(c, D_VT_TIER);
  V->seg_cnt = D<int32_t>(c, D_VT_SEGCNT);
  return 0;
}

// The pseudo-batch of a tier: the submitted (micrograph, subset) pairs, micrograph-major, and
// the offsets of their segments.
struct VotePlan {
  int t = 0;
  std::vector<int32_t> q_mg, q_mask, pseg_src;
  std::vector<int64_t> pbox_off;   // [n_q * t + 1]
  int max_live = 0;                // most pickers with an unexplained box in one micrograph
  int n_q() const { return (int)q_mg.size(); }
  int64_t n_pbox() const { return pbox_off.back(); }
};

// k_vote_count, the plan from its counts, and k_vote_gather into D_VT_GX / GY / GS / ORIGIN.
int vote_gather(rgc_ctx* c, VoteArgs& V, int t, VotePlan* P, int64_t* up, int64_t* down) {
  hipStream_t s = c->stream;
  const int n_mg = V.n_mg, k = V.k;
  const int64_t S = (int64_t)n_mg * k;
  *P = VotePlan{};
  P->t = t;
  P->pbox_off.assign(1, 0);
  if (S == 0) return 0;
  launch_vote_count(s, V);
  HIPCHK(hipGetLastError());
  TRY(ensure_host(c, H_VT_STAGE, (size_t)S * 4));
  int32_t* cnt = H<int32_t>(c, H_VT_STAGE);
  HIPCHK(hipMemcpyAsync(cnt, V.seg_cnt, (size_t)S * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *down += S * 4;
  const std::vector<int> subsets = picker_subsets(k, t);
  for (int m = 0; m < n_mg; ++m) {
    int live = 0;
    for (int p = 0; p < k; ++p) {
      if (cnt[(int64_t)m * k + p] < 0) return fail("consensus tiers: negative segment count");
      live += cnt[(int64_t)m * k + p] > 0;
    }
    P->max_live = std::max(P->max_live, live);
    if (live < t) continue;
    for (int mask : subsets) {
      bool full = true;
      for (int p = 0; p < k; ++p)
        if ((mask >> p) & 1) full = full && cnt[(int64_t)m * k + p] > 0;
      if (!full) continue;   // (an empty segment: no cliques, not submitted)
      P->q_mg.push_back(m);
      P->q_mask.push_back(mask);
      for (int p = 0; p < k; ++p)
        if ((mask >> p) & 1) {
          P->pseg_src.push_back((int32_t)(m * k + p));
          P->pbox_off.push_back(P->pbox_off.back() + cnt[(int64_t)m * k + p]);
        }
    }
  }
  const int64_t nps = (int64_t)P->pseg_src.size(), NP = P->n_pbox();
  if (nps == 0) return 0;
  if (nps > INT32_MAX / 2 || NP >= INT32_MAX)
    return fail("consensus tiers: the pseudo-batch of tier " + std::to_string(t) + " has too many boxes");
  TRY(ensure_dev(c, D_VT_PSEG, (size_t)nps * 8));
  TRY(ensure_dev(c, D_VT_PBOXOFF, ((size_t)nps + 1) * 8));
  TRY(ensure_dev(c, D_VT_GX, (size_t)NP * 8));
  TRY(ensure_dev(c, D_VT_GY, (size_t)NP * 8));
  TRY(ensure_dev(c, D_VT_GS, (size_t)NP * 8));
  TRY(ensure_dev(c, D_VT_ORIGIN, (size_t)NP * 4));
  int32_t* dseg = D<int32_t>(c, D_VT_PSEG);
  HIPCHK(hipMemcpyAsync(dseg, P->pseg_src.data(), (size_t)nps * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_PBOXOFF), P->pbox_off.data(), ((size_t)nps + 1) * 8,
                        hipMemcpyHostToDevice, s));
  *up += nps * 4 + (nps + 1) * 8;
  V.n_pseg = (int)nps;
  V.pseg_src = dseg;
  V.pseg_cnt = dseg + nps;
  V.pbox_off = D<int64_t>(c, D_VT_PBOXOFF);
  V.gx = D<double>(c, D_VT_GX);
  V.gy = D<double>(c, D_VT_GY);
  V.gs = D<double>(c, D_VT_GS);
  V.origin = D<int32_t>(c, D_VT_ORIGIN);
  launch_vote_gather(s, V);
  HIPCHK(hipGetLastError());
  TRY(ensure_host(c, H_VT_STAGE, (size_t)std::max(S, nps) * 4));
  int32_t* found = H<int32_t>(c, H_VT_STAGE);
  HIPCHK(hipMemcpyAsync(found, V.pseg_cnt, (size_t)nps * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *down += nps * 4;
  for (int64_t u = 0; u < nps; ++u)
    if (found[u] != P->pbox_off[u + 1] - P->pbox_off[u])
      return fail("consensus tiers: segment " + std::to_string(P->pseg_src[u]) + " changed between "
                  "the count and the gather pass");
  return 0;
}

// What one tier gave, copied out of the context's buffers before the next tier reuses them.
struct TierRes {
  int t = 0;
  std::vector<int64_t> pick_off, cols;   // [n_mg + 1], [n_mg]
  std::vector<double> px, py, gap;
  std::vector<float> pconf, pw;
  std::vector<int32_t> pcol, pmask, pmember, sel_cnt, status;
};

// with RGC_F_TIMING: close the sections opened since n_ev = 0 and append them to c->times
int end_sections(rgc_ctx* c) {
  TRY(mark(c, "end"));
  HIPCHK(hipStreamSynchronize(c->stream));
  return collect_times(c, true, false);
}

// After a tier's pick stage: copy its picks out of the context's host buffers, then k_vote_picks
// (weights, masks, members, unrounded consensus coordinates) and k_vote_explain with them.
// P names the tier's column arrays and the pick stage's device pick_off / pcol.
int collect_tier(rgc_ctx* c, VoteArgs& V, int64_t N, VotePickArgs P, const int64_t* pick_off,
                 const int32_t* sel_cnt, const int32_t* status, const double* gap,
                 std::vector<int64_t> cols, TierRes* r, int64_t* down) {
  hipStream_t s = c->stream;
  const int n_mg = V.n_mg, k = V.k;
  const int64_t np = pick_off[n_mg];
  r->t = P.t;
  r->cols = std::move(cols);
  r->pick_off.assign(pick_off, pick_off + n_mg + 1);
  r->sel_cnt.assign(sel_cnt, sel_cnt + n_mg);
  r->status.assign(status, status + n_mg);
  r->gap.assign(gap, gap + n_mg);
  r->px.assign(H<double>(c, H_PK_PX), H<double>(c, H_PK_PX) + np);
  r->py.assign(H<double>(c, H_PK_PY), H<double>(c, H_PK_PY) + np);
  r->pconf.assign(H<float>(c, H_PK_PCONF), H<float>(c, H_PK_PCONF) + np);
  r->pcol.assign(H<int32_t>(c, H_PK_PCOL), H<int32_t>(c, H_PK_PCOL) + np);
  r->pw.resize((size_t)np);
  r->pmask.resize((size_t)np);
  r->pmember.resize((size_t)np * k);
  if (np == 0) return 0;
  TRY(ensure_dev(c, D_VT_PCX, (size_t)np * 8));
  TRY(ensure_dev(c, D_VT_PCY, (size_t)np * 8));
  TRY(ensure_dev(c, D_VT_PW, (size_t)np * 4));
  TRY(ensure_dev(c, D_VT_PMASK, (size_t)np * 4));
  TRY(ensure_dev(c, D_VT_PMEMB, (size_t)np * k * 4));
  P.n_mg = n_mg;
  P.k = k;
  P.n_picked = np;
  P.n_box = N;
  P.bx = V.bx;
  P.by = V.by;
  P.pcx = D<double>(c, D_VT_PCX);
  P.pcy = D<double>(c, D_VT_PCY);
  P.pw = D<float>(c, D_VT_PW);
  P.pmask = D<int32_t>(c, D_VT_PMASK);
  P.pmember = D<int32_t>(c, D_VT_PMEMB);
  c->n_ev = 0;
  TRY(mark(c, "k_vote_explain"));
  launch_vote_picks(s, P);
  HIPCHK(hipGetLastError());
  V.tier = P.t;
  V.pick_off = P.pick_off;
  V.pcx = P.pcx;
  V.pcy = P.pcy;
  launch_vote_explain(s, V);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(r->pw.data(), P.pw, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(r->pmask.data(), P.pmask, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(r->pmember.data(), P.pmember, (size_t)np * k * 4, hipMemcpyDeviceToHost, s));
  TRY(end_sections(c));
  *down += np * (8 + 4 * (int64_t)k);
  return 0;
}

// strength of a micrograph's ILP status, strongest first
int ilp_rank(int st) {
  return st == RGC_ILP_OPTIMAL ? 0 : st == RGC_ILP_GAP_OK ? 1 : st == RGC_ILP_NODE_LIMIT ? 2 : 3;
}

// One tier t < k on the boxes still unexplained.  *more: false once no micrograph has min_pickers
// pickers with an unexplained box (no later tier can submit anything); *ran: a run was made.
int lower_tier(rgc_ctx* c, VoteArgs& V, int64_t N, const rgc_batch_in& bi,
               const rgc_consensus_opts* opts, int t, int min_pickers, std::vector<TierRes>& res,
               bool* more, bool* ran, int64_t* up, int64_t* down) {
  hipStream_t s = c->stream;
  const int n_mg = V.n_mg;
  VotePlan P;
  c->n_ev = 0;
  TRY(mark(c, "k_vote_gather"));
  TRY(vote_gather(c, V, t, &P, up, down));
  TRY(end_sections(c));
  *more = P.max_live >= min_pickers;
  const int nq = P.n_q();
  if (nq == 0) return 0;

  // the tier's run: every pseudo-micrograph of every micrograph in one call
  std::vector<int64_t> qid((size_t)nq);
  for (int q = 0; q < nq; ++q) qid[q] = bi.id_base[P.q_mg[q]];
  rgc_batch_in pb{};
  pb.n_mg = nq;
  pb.k = t;
  pb.box_size = bi.box_size;
  pb.flags = RGC_F_DEVICE_INPUTS | RGC_F_MEMBERS |
             (bi.flags & (RGC_F_NO_FUSED | RGC_F_TIMING | RGC_F_JI_THRESHOLD));
  pb.box_off = P.pbox_off.data();
  pb.id_base = qid.data();
  pb.x = V.gx;
  pb.y = V.gy;
  pb.score = V.gs;
  pb.ji_threshold = bi.ji_threshold;
  rgc_batch_out R{};
  std::vector<float> times = c->times;   // (run_impl replaces the sections: they follow these)
  std::vector<const char*> names = c->time_names;
  TRY(run_impl(c, &pb, &R));
  *ran = true;
  if (c->timing) {
    times.insert(times.end(), c->times.begin(), c->times.end());
    names.insert(names.end(), c->time_names.begin(), c->time_names.end());
    c->times.swap(times);
    c->time_names.swap(names);
  }
  *up += ((int64_t)nq * t + 1) * 4 + (int64_t)nq * 8;
  *down += (int64_t)mgout_bytes(nq);

  // columns: micrograph-major over the micrograph's pseudo-micrographs, then the run's order
  const size_t qmeta_bytes = (2 * (size_t)nq + 1) * 8 + 2 * (size_t)nq * 4;
  std::vector<char> qmeta(qmeta_bytes);
  int64_t* qcol_off = reinterpret_cast<int64_t*>(qmeta.data());
  int64_t* q_src = qcol_off + nq + 1;
  int32_t* q_mg = reinterpret_cast<int32_t*>(q_src + nq);
  int32_t* q_mask = q_mg + nq;
  std::vector<int64_t> col_off((size_t)n_mg + 1, 0), cols((size_t)n_mg, 0);
  int64_t nc = 0;
  for (int q = 0; q < nq; ++q) {
    const bool ok = R.status[q] == RGC_OK && R.clique_cnt[q] > 0;
    qcol_off[q] = nc;
    q_src[q] = ok ? R.clique_base[q] : 0;
    q_mg[q] = P.q_mg[q];
    q_mask[q] = P.q_mask[q];
    if (ok) {
      if (R.clique_base[q] < 0 || R.clique_base[q] + R.clique_cnt[q] > R.n_cliques)
        return fail("consensus tiers: clique range out of bounds");
      nc += R.clique_cnt[q];
      cols[P.q_mg[q]] += R.clique_cnt[q];
    }
  }
  qcol_off[nq] = nc;
  for (int m = 0; m < n_mg; ++m) col_off[m + 1] = col_off[m] + cols[m];
  if (nc >= INT32_MAX || N >= INT32_MAX) return fail("n_cols / n_rows out of range");
  if (nc == 0) return 0;   // (no column anywhere: the tier has no picks and explains nothing)

  TRY(ensure_dev(c, D_VT_QMETA, qmeta_bytes));
  TRY(ensure_dev(c, D_VT_COLOFF, ((size_t)n_mg + 1) * 8));
  TRY(ensure_dev(c, D_VT_CW, (size_t)nc * 4));
  TRY(ensure_dev(c, D_VT_CCONF, (size_t)nc * 4));
  TRY(ensure_dev(c, D_VT_CCONS, (size_t)nc * 4));
  TRY(ensure_dev(c, D_VT_CMEMB, (size_t)nc * t * 4));
  TRY(ensure_dev(c, D_VT_CMASK, (size_t)nc * 4));
  TRY(ensure_dev(c, D_VT_BAD, 16));
  TRY(ensure_dev(c, D_IL_CPTR, ((size_t)nc + 1) * 8));
  TRY(ensure_dev(c, D_IL_ROW, (size_t)nc * t * 4));
  TRY(ensure_dev(c, D_IL_W, (size_t)nc * 8));
  TRY(ensure_dev(c, D_PK_COLMG, (size_t)nc * 4));
  TRY(ensure_dev(c, D_PK_X, (size_t)nc));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_QMETA), qmeta.data(), qmeta_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_COLOFF), col_off.data(), ((size_t)n_mg + 1) * 8,
                        hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(D<void>(c, D_VT_BAD), 0, 16, s));
  *up += (int64_t)qmeta_bytes + ((int64_t)n_mg + 1) * 8;
  VoteColArgs Q{};
  Q.n_q = nq;
  Q.t = t;
  Q.n_cols = nc;
  Q.n_pbox = P.n_pbox();
  Q.n_box = N;
  Q.qcol_off = D<int64_t>(c, D_VT_QMETA);
  Q.q_src = Q.qcol_off + nq + 1;
  Q.q_mg = reinterpret_cast<const int32_t*>(Q.q_src + nq);
  Q.q_mask = Q.q_mg + nq;
  Q.origin = V.origin;
  Q.members = D<int32_t>(c, D_MEMBERS);
  Q.w = D<float>(c, D_W);
  Q.conf = D<float>(c, D_CONF);
  Q.cons = D<int32_t>(c, D_CONS);
  Q.col_ptr = D<int64_t>(c, D_IL_CPTR);
  Q.row_idx = D<int32_t>(c, D_IL_ROW);
  Q.w64 = D<double>(c, D_IL_W);
  Q.col_mg = D<int32_t>(c, D_PK_COLMG);
  Q.cw = D<float>(c, D_VT_CW);
  Q.cconf = D<float>(c, D_VT_CCONF);
  Q.ccons = D<int32_t>(c, D_VT_CCONS);
  Q.cmemb = D<int32_t>(c, D_VT_CMEMB);
  Q.cmask = D<int32_t>(c, D_VT_CMASK);
  Q.bad = D<int32_t>(c, D_VT_BAD);
  c->n_ev = 0;
  TRY(mark(c, "k_vote_cols"));
  launch_vote_cols(s, Q);
  HIPCHK(hipGetLastError());
  int32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, Q.bad, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *down += 4;
  if (bad) return fail("consensus tiers: a clique of tier " + std::to_string(t) +
                       " names a box outside its pseudo-batch");

  // one set packing per micrograph over the columns of all its subsets (rows: full-batch boxes)
  std::vector<uint8_t> hx((size_t)nc), hex((size_t)nc);
  std::vector<double> hgap((size_t)nc, 0.0);
  c->fix_fetch_bytes = 0;
  rgc_ilp_in si{};
  si.n_cols = nc;
  si.n_rows = N;
  si.node_limit = opts->node_limit;
  TRY(ilp_solve_rec(c, &si, hx.data(), hex.data(), hgap.data(), 0, t));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_PK_X), hx.data(), (size_t)nc, hipMemcpyHostToDevice, s));

  PickHost h;
  TRY(pick_host(c, n_mg, &h));
  PickArgs A{};
  A.n_mg = n_mg;
  A.k = t;
  A.n_cols = nc;
  A.num_particles = -1;   // (applied last, over all tiers)
  A.col_off = D<int64_t>(c, D_VT_COLOFF);
  A.w = Q.cw;
  A.conf = Q.cconf;
  A.cons = Q.ccons;
  A.bx = V.bx;
  A.by = V.by;
  A.x = D<uint8_t>(c, D_PK_X);
  int64_t np = 0;
  TRY(mark(c, "k_pick_emit"));
  TRY(pick_stage(c, A, h, &np));
  TRY(end_sections(c));
  for (int m = 0; m < n_mg; ++m)
    ilp_mg_status(hex.data(), hgap.data(), col_off[m], col_off[m + 1], h.primal[m], &h.status[m],
                  &h.gap[m]);
  *up += nc;
  *down += nc * 10 + ((int64_t)n_mg + 1) * 8 + (int64_t)n_mg * 12 + np * 24 + c->fix_fetch_bytes;

  VotePickArgs K{};
  K.t = t;
  K.pick_off = A.pick_off;
  K.pcol = A.pcol;
  K.col_off = A.col_off;
  K.cons = Q.ccons;
  K.members = Q.cmemb;
  K.cmask = Q.cmask;
  K.w = Q.cw;
  res.emplace_back();
  return collect_tier(c, V, N, K, h.pick_off, h.sel_cnt, h.status, h.gap, std::move(cols),
                      &res.back(), down);
}

}  // namespace

extern "C" int rgc_consensus_tiers(rgc_ctx* c, const rgc_batch_in* in,
                                   const rgc_consensus_opts* opts, int min_pickers,
                                   rgc_consensus_out* out, rgc_tiers_out* tiers) {
  if (!c || !in || !opts || !out || !tiers) return fail("null argument");
  const std::string who = "rgc_consensus_tiers";
  if (c->pend) return fail(who + ": a submitted run awaits rgc_wait on this context");
  if (in->flags & RGC_F_MULTI_OUT) return fail(who + ": RGC_F_MULTI_OUT is not supported");
  if (in->flags & RGC_F_GET_CC)
    return fail(who + ": RGC_F_GET_CC is not supported (the largest component of a pseudo-"
                "micrograph is not the micrograph's)");
  const int n_mg = in->n_mg, k = in->k;
  if (k < 1 || k > MAX_K) return fail(who + ": k (number of pickers) must be in 1..8");
  if (min_pickers < 2 || min_pickers > k) return fail(who + ": min_pickers must be in 2..k");
  if (n_mg < 0 || (n_mg > 0 && (!in->box_off || !in->id_base))) return fail(who + ": bad n_mg / null offsets");
  if (in->box_size < 1 || in->box_size > VOTE_BOX_MAX) return fail(who + ": box_size must be in 1..2^26");
  rgc_batch_in bi = batch_copy(in);
  double thr = 0.0;
  if (!batch_threshold(&bi, &thr)) return fail(who + ": ji_threshold must be finite and in [0, 1)");
  std::memset(tiers, 0, sizeof(*tiers));
  const int nt = k - min_pickers + 1;
  tiers->n_tiers = nt;

  // tier k: rgc_consensus as it is, on a run that also returns the members; every pick is kept
  // (num_particles cuts the whole list at the end)
  bi.flags |= RGC_F_MEMBERS | (opts->flags & RGC_F_TIMING);
  rgc_consensus_opts o1 = *opts;
  o1.num_particles = -1;
  TRY(consensus_impl(c, &bi, &o1, out, nullptr));
  hipStream_t s = c->stream;
  const int64_t N = out->run.n_boxes;
  int64_t up = out->h2d_bytes, down = out->d2h_bytes;

  // the outputs' host blocks.  H_VT_MG: tier k's per-micrograph run stats (the lower tiers' runs
  // reuse H_MGOUT), then pick_off, gap, tier_cols, tier_picks (8 B), sel_cnt, status (4 B)
  const size_t mgb = (mgout_bytes(n_mg) + 7) & ~(size_t)7;
  TRY(ensure_host(c, H_VT_MG, mgb + ((size_t)n_mg + 1) * 8 + (size_t)n_mg * (8 + 16 * (size_t)nt + 8) + 16));
  char* blk = H<char>(c, H_VT_MG);
  if (n_mg) std::memcpy(blk, out->run.status, mgout_bytes(n_mg));
  const MgOut mo = mgout_bind(blk, n_mg);
  rgc_batch_out& R = out->run;
  R.status = mo.status;
  R.cc_max = mo.cc_max;
  R.cc_cnt = mo.cc_cnt;
  R.n_nodes = mo.n_nodes;
  R.n_vert = mo.n_vert;
  R.n_edges_mg = mo.n_edges;
  R.clique_base = mo.clique_base;
  R.clique_cnt = mo.clique_cnt;
  int64_t* f_pick_off = reinterpret_cast<int64_t*>(blk + mgb);
  double* f_gap = reinterpret_cast<double*>(f_pick_off + n_mg + 1);
  int64_t* f_cols = reinterpret_cast<int64_t*>(f_gap + n_mg);
  int64_t* f_picks = f_cols + (size_t)n_mg * nt;
  int32_t* f_sel = reinterpret_cast<int32_t*>(f_picks + (size_t)n_mg * nt);
  int32_t* f_status = f_sel + n_mg;
  TRY(ensure_host(c, H_VT_BOXTIER, (size_t)N * 4));
  tiers->box_tier = H<int32_t>(c, H_VT_BOXTIER);
  tiers->tier_cols = f_cols;
  tiers->tier_picks = f_picks;
  f_pick_off[0] = 0;
  if (n_mg == 0) {
    out->pick_off = f_pick_off;
    out->sel_cnt = f_sel;
    out->ilp_status = f_status;
    out->ilp_gap = f_gap;
    return 0;
  }

  std::vector<TierRes> res;
  VoteArgs V;
  const double* fx = (bi.flags & RGC_F_DEVICE_INPUTS) ? bi.x : D<double>(c, D_X);
  const double* fy = (bi.flags & RGC_F_DEVICE_INPUTS) ? bi.y : D<double>(c, D_Y);
  const double* fs = (bi.flags & RGC_F_DEVICE_INPUTS) ? bi.score : D<double>(c, D_S);
  TRY(vote_setup(c, n_mg, k, bi.box_off, bi.box_size, thr, fx, fy, fs, nullptr, &V, &up));
  {
    std::vector<int64_t> cols((size_t)n_mg);
    for (int m = 0; m < n_mg; ++m)
      cols[m] = (R.status[m] == RGC_OK && R.clique_cnt[m] > 0) ? R.clique_cnt[m] : 0;
    VotePickArgs K{};
    K.t = k;
    K.pick_off = D<int64_t>(c, D_PK_OFF);
    K.pcol = D<int32_t>(c, D_PK_PCOL);
    K.col_off = D<int64_t>(c, D_PK_META);
    K.src_base = K.col_off + n_mg + 1;
    K.cons = D<int32_t>(c, D_CONS);
    K.members = D<int32_t>(c, D_MEMBERS);
    K.w = D<float>(c, D_W);
    res.emplace_back();
    TRY(collect_tier(c, V, N, K, out->pick_off, out->sel_cnt, out->ilp_status, out->ilp_gap,
                     std::move(cols), &res.back(), &down));
  }
  bool ran = false;
  for (int t = k - 1; t >= min_pickers; --t) {
    bool more = true;
    TRY(lower_tier(c, V, N, bi, opts, t, min_pickers, res, &more, &ran, &up, &down));
    if (!more) break;
  }
  if (N) {
    HIPCHK(hipMemcpyAsync(tiers->box_tier, V.box_tier, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    down += N * 4;
  }
  if (ran)   // (the lower tiers' runs reused the per-clique arrays)
    R.rows = R.consensus = R.members = nullptr, R.w = R.conf = nullptr;

  // the picks of all tiers: per micrograph tier descending, then the tier's order; the first
  // num_particles of that order
  const int64_t lim = opts->num_particles;
  std::fill(f_cols, f_cols + (size_t)n_mg * nt, (int64_t)0);
  std::fill(f_picks, f_picks + (size_t)n_mg * nt, (int64_t)0);
  int64_t total = 0;
  for (int m = 0; m < n_mg; ++m) {
    int64_t room = lim < 0 ? INT64_MAX : lim;
    f_pick_off[m] = total;
    for (const TierRes& r : res) {
      const int64_t n = std::min(room, r.pick_off[m + 1] - r.pick_off[m]);
      f_picks[(size_t)m * nt + (k - r.t)] = n;
      f_cols[(size_t)m * nt + (k - r.t)] = r.cols[m];
      room -= n;
      total += n;
    }
  }
  f_pick_off[n_mg] = total;
  const size_t np = (size_t)total;
  TRY(ensure_host(c, H_VT_PICK, np * (36 + 4 * (size_t)k) + 64));
  double* px = H<double>(c, H_VT_PICK);
  double* py = px + np;
  float* pconf = reinterpret_cast<float*>(py + np);
  int32_t* pcol = reinterpret_cast<int32_t*>(pconf + np);
  int32_t* ptier = pcol + np;
  int32_t* pmask = ptier + np;
  float* pw = reinterpret_cast<float*>(pmask + np);
  int32_t* pmember = reinterpret_cast<int32_t*>(pw + np);
  for (int m = 0; m < n_mg; ++m) {
    int64_t o = f_pick_off[m];
    int sel = 0, st = -1;
    double gap = 0.0;
    for (const TierRes& r : res) {
      const int64_t i0 = r.pick_off[m], n = f_picks[(size_t)m * nt + (k - r.t)];
      std::copy_n(r.px.begin() + i0, n, px + o);
      std::copy_n(r.py.begin() + i0, n, py + o);
      std::copy_n(r.pconf.begin() + i0, n, pconf + o);
      std::copy_n(r.pcol.begin() + i0, n, pcol + o);
      std::copy_n(r.pmask.begin() + i0, n, pmask + o);
      std::copy_n(r.pw.begin() + i0, n, pw + o);
      std::copy_n(r.pmember.begin() + i0 * k, n * k, pmember + o * k);
      std::fill_n(ptier + o, n, r.t);
      o += n;
      sel += r.sel_cnt[m];
      if (r.cols[m] > 0 || r.t == k) {   // (a tier without columns certifies nothing)
        if (st < 0 || ilp_rank(r.status[m]) > ilp_rank(st)) st = r.status[m];
        gap = std::max(gap, r.gap[m]);
      }
    }
    f_sel[m] = sel;
    f_status[m] = st;
    f_gap[m] = gap;
    bool any = false;
    for (int j = 0; j < nt; ++j) any = any || f_cols[(size_t)m * nt + j] > 0;
    if (any) R.status[m] = RGC_OK;   // (else tier k's: NO_EDGES or NO_CLIQUES)
  }
  out->n_picked = total;
  out->pick_off = f_pick_off;
  out->px = px;
  out->py = py;
  out->pconf = pconf;
  out->pcol = pcol;
  out->sel_cnt = f_sel;
  out->ilp_status = f_status;
  out->ilp_gap = f_gap;
  out->h2d_bytes = up;
  out->d2h_bytes = down;
  tiers->ptier = ptier;
  tiers->pmask = pmask;
  tiers->pw = pw;
  tiers->pmember = pmember;
  return 0;
}

extern "C" int rgc_vote_gather(rgc_ctx* c, const rgc_vote_gather_in* in, rgc_vote_gather_out* out) {
  if (!c || !in || !out) return fail("null argument");
  const std::string who = "rgc_vote_gather";
  if (c->pend) return fail(who + ": a submitted run awaits rgc_wait on this context");
  const int n_mg = in->n_mg, k = in->k, t = in->t;
  if (k < 1 || k > MAX_K) return fail(who + ": k must be in 1..8");
  if (t < 1 || t > k) return fail(who + ": t must be in 1..k");
  if (in->pick_tier < 1) return fail(who + ": pick_tier must be positive");
  if (n_mg < 0 || !in->box_off || !in->pick_off) return fail(who + ": bad n_mg / null offsets");
  if (in->box_size < 1 || in->box_size > VOTE_BOX_MAX) return fail(who + ": box_size must be in 1..2^26");
  const double thr = in->ji_threshold;
  if (!(thr >= 0.0 && thr < 1.0)) return fail(who + ": ji_threshold must be finite and in [0, 1)");
  const int64_t S = (int64_t)n_mg * k;
  if (in->box_off[0] != 0 || in->pick_off[0] != 0) return fail(who + ": offsets must start at 0");
  for (int64_t i = 0; i < S; ++i)
    if (in->box_off[i + 1] < in->box_off[i]) return fail(who + ": box_off must not decrease");
  for (int m = 0; m < n_mg; ++m)
    if (in->pick_off[m + 1] < in->pick_off[m]) return fail(who + ": pick_off must not decrease");
  const int64_t N = in->box_off[S], np = in->pick_off[n_mg];
  if (N >= INT32_MAX || np >= INT32_MAX) return fail(who + ": too many boxes / picks");
  if (N > 0 && (!in->x || !in->y || !in->score)) return fail(who + ": null box array");
  if (np > 0 && (!in->pcx || !in->pcy)) return fail(who + ": null pick array");
  HIPCHK(hipSetDevice(c->device));
  std::memset(out, 0, sizeof(*out));
  c->timing = false;
  hipStream_t s = c->stream;
  const size_t nz = (size_t)N;
  TRY(ensure_dev(c, D_VT_HXYS, 3 * nz * 8));
  TRY(ensure_dev(c, D_VT_HPOFF, ((size_t)n_mg + 1) * 8));
  TRY(ensure_dev(c, D_VT_PCX, (size_t)np * 8));
  TRY(ensure_dev(c, D_VT_PCY, (size_t)np * 8));
  double* dx = D<double>(c, D_VT_HXYS);
  if (N) {
    HIPCHK(hipMemcpyAsync(dx, in->x, nz * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dx + nz, in->y, nz * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dx + 2 * nz, in->score, nz * 8, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_HPOFF), in->pick_off, ((size_t)n_mg + 1) * 8,
                        hipMemcpyHostToDevice, s));
  if (np) {
    HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_PCX), in->pcx, (size_t)np * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(D<void>(c, D_VT_PCY), in->pcy, (size_t)np * 8, hipMemcpyHostToDevice, s));
  }
  int64_t up = 0, down = 0;
  VoteArgs V;
  TRY(vote_setup(c, n_mg, k, in->box_off, in->box_size, thr, dx, dx + nz, dx + 2 * nz,
                 in->box_tier_in, &V, &up));
  V.tier = in->pick_tier;
  V.pick_off = D<int64_t>(c, D_VT_HPOFF);
  V.pcx = D<double>(c, D_VT_PCX);
  V.pcy = D<double>(c, D_VT_PCY);
  launch_vote_explain(s, V);
  HIPCHK(hipGetLastError());
  VotePlan P;
  TRY(vote_gather(c, V, t, &P, &up, &down));
  const int nq = P.n_q();
  const int64_t NP = P.n_pbox(), nps = (int64_t)nq * t;
  TRY(ensure_host(c, H_VT_BOXTIER, nz * 4));
  TRY(ensure_host(c, H_VT_SUB, ((size_t)nps + 1) * 8 + 2 * (size_t)nq * 4));
  TRY(ensure_host(c, H_VT_ORIGIN, (size_t)NP * 4));
  TRY(ensure_host(c, H_VT_GXYS, 3 * (size_t)NP * 8));
  out->n_sub = nq;
  out->box_off = H<int64_t>(c, H_VT_SUB);
  out->sub_mg = reinterpret_cast<int32_t*>(out->box_off + nps + 1);
  out->sub_mask = out->sub_mg + nq;
  std::copy(P.pbox_off.begin(), P.pbox_off.end(), out->box_off);
  std::copy(P.q_mg.begin(), P.q_mg.end(), out->sub_mg);
  std::copy(P.q_mask.begin(), P.q_mask.end(), out->sub_mask);
  out->box_tier = H<int32_t>(c, H_VT_BOXTIER);
  out->origin = H<int32_t>(c, H_VT_ORIGIN);
  out->x = H<double>(c, H_VT_GXYS);
  out->y = out->x + NP;
  out->score = out->y + NP;
  if (N) HIPCHK(hipMemcpyAsync(out->box_tier, V.box_tier, nz * 4, hipMemcpyDeviceToHost, s));
  if (NP) {
    HIPCHK(hipMemcpyAsync(out->origin, V.origin, (size_t)NP * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->x, V.gx, (size_t)NP * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->y, V.gy, (size_t)NP * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out->score, V.gs, (size_t)NP * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}
