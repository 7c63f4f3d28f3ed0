// rgc_ilp_host.cpp — host loop of the set-packing solver (rgc_ilp.hip): rgc_ilp_solve, and
// ilp_solve_rec for rgc_consensus.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rgc_host.h"

using namespace rgc;

// One pass of the device solver over a CSC batch (rgc_ilp_solve runs it once, then once more
// on the reduced-cost-fixed columns of the components it left unproven): x, statuses and the
// per-component gaps (gap_out, at one column of each component) on the host.  With fix set,
// the kept columns of the certified components come back too (rgc_ilp.hip k_fs_*).
struct IlpFix {
  std::vector<uint8_t> keep;    // [n_cols] kept by reduced-cost fixing
  std::vector<int32_t> comp;    // [n_cols] component of each column
  std::vector<uint32_t> cnt;    // [n_comp] kept columns per component
  std::vector<uint8_t> cert;    // [n_comp] 0: proven by the search, else certified
};

// dev_k > 0: the CSC arrays are already in D_IL_CPTR / D_IL_ROW / D_IL_W (written by
// k_pick_cols: every column has dev_k rows in range by construction) and in->col_ptr / row_idx /
// w are not read; else they are validated here and uploaded.
static int ilp_core(rgc_ctx* c, const rgc_ilp_in* in, uint8_t* x, uint8_t* exact,
                    double* gap_out, IlpFix* fix, int dev_k = 0) {
  const int64_t nc = in->n_cols, nr = in->n_rows;
  if (nc == 0) return 0;
  int64_t nnz = nc * dev_k;
  int kmax = dev_k;
  if (!dev_k) {
    nnz = in->col_ptr[nc];
    if (in->col_ptr[0] != 0 || nnz < 0) return fail("col_ptr must start at 0");
    kmax = 1;
    for (int64_t j = 0; j < nc; ++j) {
      const int64_t d = in->col_ptr[j + 1] - in->col_ptr[j];
      if (d < 1) return fail("every column needs at least one row");
      kmax = (int)std::max<int64_t>(kmax, d);
    }
    if (kmax > 8) return fail("columns of more than 8 rows (cliques of more than 8 boxes)");
    for (int64_t e = 0; e < nnz; ++e)
      if (in->row_idx[e] < 0 || in->row_idx[e] >= nr) return fail("row index out of range");
  }
  hipStream_t s = c->stream;
  TRY(ensure_dev(c, D_IL_CPTR, (nc + 1) * 8));
  TRY(ensure_dev(c, D_IL_ROW, nnz * 4));
  TRY(ensure_dev(c, D_IL_W, nc * 8));
  TRY(ensure_dev(c, D_IL_REP, nr * 4));
  TRY(ensure_dev(c, D_IL_PAR, nc * 4));
  TRY(ensure_dev(c, D_IL_ROOT, nc * 4));
  TRY(ensure_dev(c, D_IL_CSIZE, nc * 4));
  TRY(ensure_dev(c, D_IL_RCNT, nr * 4));
  TRY(ensure_dev(c, D_IL_RCUR, nr * 4));
  TRY(ensure_dev(c, D_IL_RPTR, (nr + 1) * 8));
  TRY(ensure_dev(c, D_IL_RCOLS, nnz * 4));
  TRY(ensure_dev(c, D_IL_CID, (nc + 1) * 8));
  TRY(ensure_dev(c, D_IL_MEM, nc * 4));
  TRY(ensure_dev(c, D_IL_LOC, nc * 4));
  TRY(ensure_dev(c, D_IL_SCR, (size_t)nc * (2 * kmax + 8) * 8));
  TRY(ensure_dev(c, D_IL_RLOC, nr * 4));
  TRY(ensure_dev(c, D_IL_NBIG, 16));
  TRY(ensure_dev(c, D_IL_X, nc));
  TRY(ensure_dev(c, D_IL_EX, nc));
  TRY(ensure_dev(c, D_TILES, scan_tiles_needed(std::max(nc, nr) + 1) * 8));
  TRY(tiles_refresh(c));
  TRY(ensure_dev(c, D_TOTAL, 32));
  TRY(ensure_host(c, H_TOTAL, 64));
  if (!dev_k) {
    HIPCHK(hipMemcpyAsync(c->d[D_IL_CPTR].p, in->col_ptr, (nc + 1) * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d[D_IL_ROW].p, in->row_idx, nnz * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d[D_IL_W].p, in->w, nc * 8, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemsetAsync(c->d[D_IL_NBIG].p, 0, 16, s));
  rgc::IlpArgs A{};
  A.n_cols = nc;
  A.n_rows = nr;
  A.kmax = kmax;
  A.node_limit = in->node_limit > 0 ? in->node_limit : (int64_t)RGC_ILP_DEFAULT_NODES;
  A.col_ptr = D<int64_t>(c, D_IL_CPTR);
  A.row_idx = D<int32_t>(c, D_IL_ROW);
  A.w = D<double>(c, D_IL_W);
  A.rep = D<int32_t>(c, D_IL_REP);
  A.rloc = D<int32_t>(c, D_IL_RLOC);
  A.parent = D<int32_t>(c, D_IL_PAR);
  A.is_root = D<int32_t>(c, D_IL_ROOT);
  A.csize = D<int32_t>(c, D_IL_CSIZE);
  A.rcnt = D<int32_t>(c, D_IL_RCNT);
  A.rcur = D<int32_t>(c, D_IL_RCUR);
  A.rptr = D<int64_t>(c, D_IL_RPTR);
  A.rcols = D<int32_t>(c, D_IL_RCOLS);
  A.comp_id = D<int64_t>(c, D_IL_CID);
  A.members = D<int32_t>(c, D_IL_MEM);
  A.loc = D<int32_t>(c, D_IL_LOC);
  A.scratch = D<uint64_t>(c, D_IL_SCR);
  A.n_big = D<unsigned int>(c, D_IL_NBIG);
  A.x = D<uint8_t>(c, D_IL_X);
  A.exact = D<uint8_t>(c, D_IL_EX);
  TRY(mark(c, "k_ilp_components"));
  rgc::launch_ilp(s, 0, A, 0, 0);
  launch_scan(s, nc, A.is_root, D<int64_t>(c, D_IL_CID), D<int64_t>(c, D_TILES),
              D<int64_t>(c, D_TOTAL));
  HIPCHK(hipMemcpyAsync(H<int64_t>(c, H_TOTAL), D<int64_t>(c, D_TOTAL), 8, hipMemcpyDeviceToHost, s));
  launch_scan(s, nr, A.rcnt, D<int64_t>(c, D_IL_RPTR), D<int64_t>(c, D_TILES),
              D<int64_t>(c, D_TOTAL) + 1);
  HIPCHK(hipStreamSynchronize(s));
  const int64_t ncomp = H<int64_t>(c, H_TOTAL)[0];
  if (ncomp < 0) return fail("component scan: look-back guard exhausted (stale tile buffer)");
  TRY(ensure_dev(c, D_IL_CN, (ncomp + 1) * 4));
  TRY(ensure_dev(c, D_IL_COFF, (ncomp + 1) * 8));
  TRY(ensure_dev(c, D_IL_CCUR, (ncomp + 1) * 4));
  TRY(ensure_dev(c, D_IL_BIG, (ncomp + 1) * 4));
  A.n_comp = ncomp;
  A.comp_n = D<int32_t>(c, D_IL_CN);
  A.comp_off = D<int64_t>(c, D_IL_COFF);
  A.comp_cur = D<int32_t>(c, D_IL_CCUR);
  A.big = D<int32_t>(c, D_IL_BIG);
  rgc::launch_ilp(s, 1, A, 0, 0);
  launch_scan(s, ncomp, A.comp_n, D<int64_t>(c, D_IL_COFF), D<int64_t>(c, D_TILES),
              D<int64_t>(c, D_TOTAL) + 2);
  HIPCHK(hipMemsetAsync(A.comp_cur, 0, (ncomp + 1) * 4, s));
  rgc::launch_ilp(s, 2, A, 0, 0);
  TRY(mark(c, "k_ilp_small"));
  rgc::launch_ilp(s, 3, A, 0, 0);
  HIPCHK(hipMemcpyAsync(H<int64_t>(c, H_TOTAL) + 1, A.n_big, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const int n_big = (int)*reinterpret_cast<uint32_t*>(H<int64_t>(c, H_TOTAL) + 1);
  // certification arrays (rgc_ilp.hip): also the wave search's pre-search multipliers
  TRY(ensure_dev(c, D_IL_CERT, ncomp + 1));
  TRY(ensure_dev(c, D_IL_KEY, nc * 8));
  TRY(ensure_dev(c, D_IL_ST, nc));
  TRY(ensure_dev(c, D_IL_RMAX, nr * 8 + 8));
  TRY(ensure_dev(c, D_IL_OWN, nr * 4 + 4));
  TRY(ensure_dev(c, D_IL_LAM, nr * 8 + 8));
  TRY(ensure_dev(c, D_IL_GRAD, nr * 8 + 8));
  TRY(ensure_dev(c, D_IL_CS, (ncomp + 1) * 10 * 8));
  TRY(ensure_dev(c, D_IL_STSAVE, nc));
  TRY(ensure_dev(c, D_IL_CNT, 16));
  A.cert = D<uint8_t>(c, D_IL_CERT);
  A.key = D<uint64_t>(c, D_IL_KEY);
  A.st = D<uint8_t>(c, D_IL_ST);
  A.rmax = D<uint64_t>(c, D_IL_RMAX);
  A.owner = D<int32_t>(c, D_IL_OWN);
  A.lam = D<double>(c, D_IL_LAM);
  A.grad = D<double>(c, D_IL_GRAD);
  A.cs = D<double>(c, D_IL_CS);
  A.count = D<unsigned int>(c, D_IL_CNT);
  A.st_save = D<uint8_t>(c, D_IL_STSAVE);
  // per-component gaps: zero for proven components
  TRY(ensure_dev(c, D_IL_GAP, nc * 8));
  A.gap = D<double>(c, D_IL_GAP);
  HIPCHK(hipMemsetAsync(A.gap, 0, nc * 8, s));
  // rounds until a pass changes nothing (each round settles at least the heaviest undecided
  // clique / makes at least one improving swap, so both terminate); counters read every 4
  auto rounds = [&](int phase, int cap) -> int {
    for (int it = 0; it < cap; it += 4) {
      HIPCHK(hipMemsetAsync(A.count, 0, 4, s));
      for (int j = 0; j < 4; ++j) rgc::launch_ilp_cert(s, phase, A);
      HIPCHK(hipMemcpyAsync(H<int64_t>(c, H_TOTAL) + 3, A.count, 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (*reinterpret_cast<uint32_t*>(H<int64_t>(c, H_TOTAL) + 3) == 0) break;
    }
    return 0;
  };
  // Lagrangian repack of the flagged components (rgc_ilp.hip k_rp_*): greedy by reduced cost
  // with the best multipliers, swaps, kept per component when better
  auto repack = [&]() -> int {
    rgc::launch_ilp_cert(s, 8, A);
    TRY(rounds(1, 1 << 20));
    TRY(rounds(2, 1 << 16));
    rgc::launch_ilp_cert(s, 9, A);
    return 0;
  };
  if (n_big > 0) {
    std::vector<int32_t> big(n_big), cn(ncomp);
    HIPCHK(hipMemcpyAsync(big.data(), A.big, n_big * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(cn.data(), A.comp_n, ncomp * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    int nmax = 0;
    for (int b : big) nmax = std::max(nmax, std::min(cn[b], rgc::ilp_big_max()));
    const int64_t W = (nmax + 63) / 64;
    // adjacency n W, stack n (W + 2), weights n, tmpid K n / 2, row info (K + 1) n / 4; then
    // the Lagrangian bound's row multipliers K n and member weights n
    A.wlag_off = (int64_t)nmax * W + (int64_t)nmax * (W + 2) + nmax +
                 ((int64_t)kmax * nmax + 1) / 2 + ((int64_t)(kmax + 1) * nmax + 3) / 4 + 8;
    A.wstride = A.wlag_off + (int64_t)(kmax + 1) * nmax;
    const int n_waves = std::min(n_big, 2048);
    TRY(ensure_dev(c, D_IL_WSCR, (size_t)n_waves * A.wstride * 8));
    A.wscratch = D<uint64_t>(c, D_IL_WSCR);
    // multipliers for the search's Lagrangian bound: the certification's greedy primal,
    // swaps and projected subgradient (rgc_ilp.hip) on the wave components (cert 3)
    TRY(mark(c, "k_ilp_lagrange"));
    HIPCHK(hipMemsetAsync(A.count, 0, 16, s));
    rgc::launch_ilp_cert(s, 6, A);
    TRY(rounds(1, 1 << 20));
    TRY(rounds(2, 1 << 16));
    rgc::launch_ilp_cert(s, 3, A);
    for (int it = 0; it < 400; ++it) rgc::launch_ilp_cert(s, 4, A);
    rgc::launch_ilp_cert(s, 7, A);
    // the packing repacked by reduced cost when better: it seeds the search's incumbent
    TRY(repack());
    TRY(mark(c, "k_ilp_wave"));
    rgc::launch_ilp(s, 4, A, n_big, n_waves);
  }
  TRY(mark(c, "k_ilp_cert"));
  HIPCHK(hipMemsetAsync(A.count, 0, 16, s));
  rgc::launch_ilp_cert(s, 0, A);
  // no component left unproven by the branch and bound (the common case): nothing to certify
  HIPCHK(hipMemcpyAsync(H<int64_t>(c, H_TOTAL) + 3, A.count, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const bool any_flagged = reinterpret_cast<uint32_t*>(H<int64_t>(c, H_TOTAL) + 3)[1] != 0;
  if (any_flagged) {
    TRY(rounds(1, 1 << 20));
    TRY(rounds(2, 1 << 16));
    rgc::launch_ilp_cert(s, 3, A);
    // projected subgradient iterations of the Lagrangian bound (per component Polyak steps
    // towards the primal; after 40 iterations without progress the step shrinks and lam
    // restarts from the best one), a repack by reduced cost from the multipliers, then more
    // iterations with the better primal's steps
    for (int it = 0; it < 1000; ++it) rgc::launch_ilp_cert(s, 4, A);
    TRY(repack());
    for (int it = 0; it < 4000; ++it) rgc::launch_ilp_cert(s, 4, A);
    TRY(repack());
    for (int it = 0; it < 2000; ++it) rgc::launch_ilp_cert(s, 4, A);
    rgc::launch_ilp_cert(s, 5, A);
    if (fix) {   // reduced-cost fixing of the certified components (the second pass's input)
      TRY(ensure_dev(c, D_IL_FS, (ncomp + 1) * 16));
      TRY(ensure_dev(c, D_IL_FSCNT, (ncomp + 1) * 4));
      TRY(ensure_dev(c, D_IL_FSKEEP, nc));
      A.fs = D<double>(c, D_IL_FS);
      A.fs_cnt = D<unsigned int>(c, D_IL_FSCNT);
      A.fs_keep = D<uint8_t>(c, D_IL_FSKEEP);
      rgc::launch_ilp_cert(s, 10, A);
      fix->keep.resize(nc);
      fix->comp.resize(nc);
      fix->cnt.resize(ncomp);
      fix->cert.resize(ncomp);
      HIPCHK(hipMemcpyAsync(fix->keep.data(), A.fs_keep, nc, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(fix->comp.data(), A.loc, nc * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(fix->cnt.data(), A.fs_cnt, ncomp * 4, hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(fix->cert.data(), A.cert, ncomp, hipMemcpyDeviceToHost, s));
    }
  }
  TRY(mark(c, "d2h_x"));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(x, A.x, nc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(exact, A.exact, nc, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(gap_out, A.gap, nc * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}

// The device solver, then (depth < ILP_FIX_DEPTH) reduced-cost fixing of the components it
// left unproven, solved by the same function one level down.
constexpr int ILP_FIX_DEPTH = 4;

int ilp_solve_rec(rgc_ctx* c, const rgc_ilp_in* in, uint8_t* x, uint8_t* exact, double* gap,
                  int depth, int dev_k) {
  const int64_t nc = in->n_cols, nr = in->n_rows;
  if (nc == 0) return 0;
  IlpFix fix;
  TRY(ilp_core(c, in, x, exact, gap, depth + 1 < ILP_FIX_DEPTH ? &fix : nullptr, dev_k));
  // device inputs (rgc_consensus): the fix pass below reads the CSC arrays on the host, so
  // they are fetched, but only when there is something to fix
  rgc_ilp_in host_in;
  std::vector<int64_t> h_ptr;
  std::vector<int32_t> h_row;
  std::vector<double> h_w;
  if (dev_k && !fix.cnt.empty()) {
    h_ptr.resize(nc + 1);
    h_row.resize(nc * dev_k);
    h_w.resize(nc);
    HIPCHK(hipMemcpyAsync(h_ptr.data(), c->d[D_IL_CPTR].p, (nc + 1) * 8, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipMemcpyAsync(h_row.data(), c->d[D_IL_ROW].p, nc * dev_k * 4, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipMemcpyAsync(h_w.data(), c->d[D_IL_W].p, nc * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->fix_fetch_bytes += (nc + 1) * 8 + nc * dev_k * 4 + nc * 8;
    host_in = *in;
    host_in.col_ptr = h_ptr.data();
    host_in.row_idx = h_row.data();
    host_in.w = h_w.data();
    in = &host_in;
  }
  // Next pass: the certified components whose reduced-cost-fixed column set is small enough
  // for the exact search (and smaller than the component), solved as one batch.  A packing of
  // component j that uses a fixed column is worth less than its packing P_j, so its optimum is
  // max(P_j, optimum over the kept columns): proven when the second pass proves its part.
  if (!fix.cnt.empty()) {
    const int64_t ncomp = (int64_t)fix.cnt.size();
    std::vector<int32_t> size(ncomp, 0);
    std::vector<double> pval(ncomp, 0.0), gap1(ncomp, 0.0);
    for (int64_t j = 0; j < nc; ++j) {
      const int32_t q = fix.comp[j];
      ++size[q];
      if (x[j]) pval[q] += in->w[j];
      gap1[q] += gap[j];
    }
    std::vector<uint8_t> elig(ncomp, 0);
    int64_t sub_nc = 0, sub_nnz = 0;
    for (int64_t q = 0; q < ncomp; ++q)
      elig[q] = fix.cert[q] != 0 && gap1[q] > 0.0 && fix.cnt[q] > 0 &&
                (int)fix.cnt[q] <= rgc::ilp_big_max() && (int32_t)fix.cnt[q] < size[q];
    std::vector<int64_t> sub_ptr(1, 0);
    std::vector<int32_t> sub_row;
    std::vector<double> sub_w;
    std::vector<int64_t> sub_col;   // original column of each sub column
    for (int64_t j = 0; j < nc; ++j) {
      if (!elig[fix.comp[j]] || !fix.keep[j]) continue;
      for (int64_t e = in->col_ptr[j]; e < in->col_ptr[j + 1]; ++e) sub_row.push_back(in->row_idx[e]);
      sub_nnz += in->col_ptr[j + 1] - in->col_ptr[j];
      sub_ptr.push_back(sub_nnz);
      sub_w.push_back(in->w[j]);
      sub_col.push_back(j);
      ++sub_nc;
    }
    if (sub_nc > 0) {
      TRY(mark(c, "k_ilp_fixsearch"));
      rgc_ilp_in sub{};
      sub.n_cols = sub_nc;
      sub.n_rows = nr;
      sub.col_ptr = sub_ptr.data();
      sub.row_idx = sub_row.data();
      sub.w = sub_w.data();
      // (4x the nodes one level down, up to 16x the first pass's: its components are the few
      // hard ones, restricted)
      const int64_t nl = in->node_limit > 0 ? in->node_limit : (int64_t)RGC_ILP_DEFAULT_NODES;
      sub.node_limit = depth < 2 ? 4 * nl : nl;
      std::vector<uint8_t> sx(sub_nc), sex(sub_nc);
      std::vector<double> sgap(sub_nc);
      // (with RGC_F_TIMING the second pass's sections follow "k_ilp_fixsearch" in the list)
      TRY(ilp_solve_rec(c, &sub, sx.data(), sex.data(), sgap.data(), depth + 1));
      std::vector<double> rval(ncomp, 0.0), rgap(ncomp, 0.0);
      std::vector<uint8_t> ropt(ncomp, 1);
      for (int64_t i = 0; i < sub_nc; ++i) {
        const int32_t q = fix.comp[sub_col[i]];
        if (sx[i]) rval[q] += sub_w[i];
        rgap[q] += sgap[i];
        if (sex[i] != RGC_ILP_OPTIMAL) ropt[q] = 0;
      }
      // per eligible component: bound min(L, max(P, R + sub gap)); the better packing
      std::vector<uint8_t> take(ncomp, 0), st(ncomp, 0);
      std::vector<double> g(ncomp, 0.0);
      for (int64_t q = 0; q < ncomp; ++q) {
        if (!elig[q]) continue;
        const double P = pval[q], L = P + gap1[q], R = rval[q];
        const double ub = std::min(L, std::max(P, R + (ropt[q] ? 0.0 : rgap[q])));
        take[q] = R > P;
        const double v = take[q] ? R : P;
        g[q] = std::max(0.0, ub - v);
        st[q] = g[q] <= 0.0 ? RGC_ILP_OPTIMAL : g[q] <= 1e-4 * std::fabs(v) ? RGC_ILP_GAP_OK : 0;
      }
      if (std::getenv("RGC_ILP_DEBUG")) {
        int64_t nel = 0, nopt = 0, nok = 0, ntake = 0, nflag = 0, nbig = 0, cmax = 0;
        for (int64_t q = 0; q < ncomp; ++q) {
          nflag += fix.cert[q] != 0;
          if (fix.cert[q] && gap1[q] > 0.0) {
            nbig += (int)fix.cnt[q] > rgc::ilp_big_max();
            cmax = std::max<int64_t>(cmax, fix.cnt[q]);
          }
          if (!elig[q]) continue;
          ++nel;
          nopt += st[q] == RGC_ILP_OPTIMAL;
          nok += st[q] == RGC_ILP_GAP_OK;
          ntake += take[q];
        }
        std::fprintf(stderr, "rgc_ilp fixsearch %d: %lld flagged, %lld eligible, %lld columns; "
                     "%lld optimal, %lld gap-ok, %lld improved; %lld kept > search limit "
                     "(largest kept set %lld)\n", depth, (long long)nflag, (long long)nel,
                     (long long)sub_nc, (long long)nopt, (long long)nok, (long long)ntake,
                     (long long)nbig, (long long)cmax);
      }
      std::vector<uint8_t> seen(ncomp, 0);
      for (int64_t j = 0; j < nc; ++j) {
        const int32_t q = fix.comp[j];
        if (!elig[q]) continue;
        if (take[q]) x[j] = 0;
        if (st[q]) exact[j] = st[q];
        gap[j] = 0.0;
        if (!seen[q]) {   // the component's gap at its first column
          seen[q] = 1;
          gap[j] = g[q];   // (<= the first pass's: the bound is min(L, ...))
        }
      }
      for (int64_t i = 0; i < sub_nc; ++i)
        if (take[fix.comp[sub_col[i]]] && sx[i]) x[sub_col[i]] = 1;
    }
  }
  return 0;
}

extern "C" int rgc_ilp_solve(rgc_ctx* c, const rgc_ilp_in* in, uint8_t* x, uint8_t* exact) {
  if (!c || !in || !x || !exact) return fail("null argument");
  if (c->pend) return fail("rgc_ilp_solve: a submitted run awaits rgc_wait on this context");
  HIPCHK(hipSetDevice(c->device));
  const int64_t nc = in->n_cols, nr = in->n_rows;
  if (nc < 0 || nc >= INT32_MAX || nr < 0 || nr >= INT32_MAX) return fail("n_cols / n_rows out of range");
  c->times.clear();
  c->time_names.clear();
  c->n_ev = 0;
  c->timing = (in->flags & RGC_F_TIMING) != 0;
  if (nc == 0) return 0;
  std::vector<double> gap(nc);
  TRY(ilp_solve_rec(c, in, x, exact, gap.data(), 0));
  if (in->gap) std::memcpy(in->gap, gap.data(), nc * 8);
  TRY(mark(c, "end"));
  HIPCHK(hipStreamSynchronize(c->stream));
  return collect_times(c, true, false);   // (cleared at entry, timing or not)
}
