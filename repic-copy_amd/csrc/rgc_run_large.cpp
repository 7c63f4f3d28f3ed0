// rgc_run_large.cpp — the large-micrograph route: the multi-kernel pipeline (rgc_kernels.hip,
// rgc_cliques.hip) for micrographs the fused kernel cannot take (too large for LDS, or still
// deferred after its three passes).
#include <algorithm>
#include <cstring>

#include "rgc_host.h"

using namespace rgc;

// Runs the multi-kernel pipeline on a (sub-)batch whose x/y/score are device arrays, writing
// per-clique outputs at [out_base, out_base + C).  Fills st_out[n_mg] (clique_base/cnt set).
int run_multi(rgc_ctx* c, int n_mg, int k, double B, double two_b2, const JiCut& cut,
              int get_cc, int multi,
              bool want_members, bool want_ji, const int64_t* box_off, const int64_t* id_base,
              const double* x, const double* y, const double* sc, int64_t out_base,
              std::vector<MgStat>& st_out, int64_t* C_out, int64_t* E_out) {
  const int64_t N = box_off[(int64_t)n_mg * k];
  const size_t nbo = (size_t)n_mg * k + 1;
  std::vector<int32_t> cell_off(n_mg + 1);
  int64_t cells = 0;
  bool bin_wide = false;   // k1_bin's u32 counters: a micrograph of more than 65535 boxes
  int max_n = 0;           // largest micrograph (k1_bin's LDS; LDS union-find when it fits)
  for (int m = 0; m < n_mg; ++m) {
    const int64_t nm = box_off[(int64_t)(m + 1) * k] - box_off[(int64_t)m * k];
    bin_wide |= nm > 65535;
    max_n = std::max<int>(max_n, (int)std::min<int64_t>(nm, INT32_MAX));
  }
  for (int m = 0; m < n_mg; ++m) {
    cell_off[m] = (int32_t)cells;
    const int64_t nm = box_off[(int64_t)(m + 1) * k] - box_off[(int64_t)m * k];
    cells += bin_budget(nm, bin_wide) + 2;
  }
  cell_off[n_mg] = (int32_t)cells;
  if (cells >= (1LL << 31)) return fail("too many grid cells in one batch");
  const size_t stage_bytes = nbo * 4 + 2 * (n_mg + 1) * 4 + n_mg * 8 + 64;
  TRY(ensure_host(c, H_STAGE, stage_bytes));
  int32_t* st_bo = H<int32_t>(c, H_STAGE);
  int32_t* st_co = st_bo + nbo;
  int32_t* st_p0 = st_co + n_mg + 1;   // picker-0 prefix: wavefront -> clique root
  int64_t* st_id = reinterpret_cast<int64_t*>(
      (reinterpret_cast<uintptr_t>(st_p0 + n_mg + 1) + 7) & ~(uintptr_t)7);
  for (size_t i = 0; i < nbo; ++i) st_bo[i] = (int32_t)box_off[i];
  std::memcpy(st_co, cell_off.data(), (n_mg + 1) * 4);
  std::memcpy(st_id, id_base, n_mg * 8);
  int64_t n_roots = 0;
  for (int m = 0; m < n_mg; ++m) {
    st_p0[m] = (int32_t)n_roots;
    n_roots += box_off[(int64_t)m * k + 1] - box_off[(int64_t)m * k];
  }
  st_p0[n_mg] = (int32_t)n_roots;

  // the per-micrograph metadata (box offsets, cell offsets, picker-0 prefix, id bases) go up
  // in ONE copy of the host staging block; the device block has the same layout
  const size_t meta_bytes = (size_t)(reinterpret_cast<char*>(st_id + n_mg) -
                                     reinterpret_cast<char*>(st_bo));
  TRY(ensure_dev(c, D_BOXOFF, meta_bytes));
  TRY(ensure_dev(c, D_GRID, n_mg * sizeof(MgGrid)));
  TRY(ensure_dev(c, D_CELLSTART, cells * 4));
  TRY(ensure_dev(c, D_SX, N * 8));
  TRY(ensure_dev(c, D_SY, N * 8));
  TRY(ensure_dev(c, D_SBOX, N * 4));
  TRY(ensure_dev(c, D_SPICK, N));
  TRY(ensure_dev(c, D_SMG, N * 4));
  TRY(ensure_dev(c, D_BMG, N * 4));
  TRY(ensure_dev(c, D_BPICK, N));
  TRY(ensure_dev(c, D_FWDCNT, N * 4));
  TRY(ensure_dev(c, D_FWDOFF, (N + 1) * 8));
  TRY(ensure_dev(c, D_TILES, scan_tiles_needed(N + 1) * 8));
  TRY(ensure_dev(c, D_TOTAL, 32));
  TRY(ensure_dev(c, D_PARENT, N * 4));
  TRY(ensure_dev(c, D_HASEDGE, N));
  TRY(ensure_dev(c, D_CSIZE, N * 4));
  TRY(ensure_dev(c, D_STAT, n_mg * sizeof(MgStat)));
  TRY(ensure_dev(c, D_INSKEY, N * 8));
  if (get_cc) TRY(ensure_dev(c, D_COMPMIN, N * 8));
  TRY(ensure_dev(c, D_CCOUNT, N * 4));
  TRY(ensure_dev(c, D_COFF, (N + 1) * 8));
  TRY(ensure_dev(c, D_INCL, N));
  TRY(ensure_dev(c, D_VLIST, N * 4));
  TRY(ensure_dev(c, D_VSORT, N * 4));
  TRY(ensure_dev(c, D_VROW, N * 4));
  TRY(ensure_dev(c, D_BOFF, (N + 1) * 8));
  TRY(ensure_dev(c, D_RLO, 2 * (size_t)n_mg * 8 + 8));
  TRY(ensure_host(c, H_TOTAL, 32));
  TRY(ensure_host(c, H_STAT, n_mg * sizeof(MgStat)));
  TRY(ensure_host(c, H_MGOFF, 2 * (size_t)n_mg * 8 + 8));
  TRY(ensure_dev(c, D_RBOUND, N * 8));
  TRY(ensure_dev(c, D_RFLAG, N));
  TRY(ensure_dev(c, D_ROOTBOX, n_roots * 4));
  TRY(ensure_dev(c, D_DFSMG, n_mg));

  hipStream_t s = c->stream;
  TRY(mark(c, "h2d_meta"));
  HIPCHK(hipMemcpyAsync(D<void>(c, D_BOXOFF), st_bo, meta_bytes, hipMemcpyHostToDevice, s));
  const int32_t* d_co = D<int32_t>(c, D_BOXOFF) + (st_co - st_bo);
  const int32_t* d_p0 = D<int32_t>(c, D_BOXOFF) + (st_p0 - st_bo);
  const int64_t* d_id = reinterpret_cast<const int64_t*>(
      D<char>(c, D_BOXOFF) + (reinterpret_cast<char*>(st_id) - reinterpret_cast<char*>(st_bo)));
  TRY(mark(c, "memset"));
  // the level loop's first count array (non-roots stay 0) is zeroed with the others
  TRY(ensure_dev(c, D_LCNT, N * 4));
  {
    rgc::FillSegs F{};
    F.add(D<void>(c, D_HASEDGE), N, 0);
    F.add(D<void>(c, D_CSIZE), N * 4, 0);
    F.add(D<void>(c, D_INCL), N, 0);
    F.add(D<void>(c, D_CCOUNT), N * 4, 0);
    F.add(D<void>(c, D_VLIST), N * 4, 0);   // row-rank bucket counters
    F.add(D<void>(c, D_RFLAG), N, 0);
    F.add(D<void>(c, D_DFSMG), n_mg, 0);
    F.add(D<void>(c, D_INSKEY), N * 8, 0xff);
    F.add(D<void>(c, D_LCNT), N * 4, 0);
    if (get_cc) F.add(D<void>(c, D_COMPMIN), N * 8, 0xff);
    rgc::launch_fill_multi(s, F);
  }

  const int32_t* bo = D<int32_t>(c, D_BOXOFF);
  TRY(mark(c, "k1_bin"));
  launch_bin(s, n_mg, k, B, cut.row_min, bo, d_co, x, y, D<MgGrid>(c, D_GRID),
             D<int32_t>(c, D_CELLSTART), D<double>(c, D_SX), D<double>(c, D_SY),
             D<int32_t>(c, D_SBOX), D<uint8_t>(c, D_SPICK), D<int32_t>(c, D_SMG),
             D<int32_t>(c, D_BMG), D<uint8_t>(c, D_BPICK), bin_wide, max_n);
  TRY(mark(c, "k2_pairs_count"));
  launch_pairs(s, false, (int)N, k, B, two_b2, cut, bo, d_co, D<MgGrid>(c, D_GRID),
               D<int32_t>(c, D_CELLSTART), D<double>(c, D_SX), D<double>(c, D_SY),
               D<int32_t>(c, D_SBOX), D<uint8_t>(c, D_SPICK), D<int32_t>(c, D_SMG),
               D<int32_t>(c, D_FWDCNT), nullptr, nullptr, nullptr);
  TRY(mark(c, "scan_edges"));
  launch_scan(s, N, D<int32_t>(c, D_FWDCNT), D<int64_t>(c, D_FWDOFF), D<int64_t>(c, D_TILES),
              D<int64_t>(c, D_TOTAL));
  HIPCHK(hipMemcpyAsync(H<int64_t>(c, H_TOTAL), D<int64_t>(c, D_TOTAL), 8,
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  const int64_t E = H<int64_t>(c, H_TOTAL)[0];
  if (E < 0) return fail("edge scan: look-back guard exhausted (stale tile buffer)");
  *E_out = E;
  TRY(ensure_dev(c, D_EDST, E * 4));
  TRY(ensure_dev(c, D_ADJG, E * 8));
  if (want_ji) TRY(ensure_dev(c, D_EJI, E * 8));   // (the edge JIs feed the RGC_F_EDGES dump only)
  TRY(mark(c, "k2_pairs_fill"));
  launch_pairs(s, true, (int)N, k, B, two_b2, cut, bo, d_co, D<MgGrid>(c, D_GRID),
               D<int32_t>(c, D_CELLSTART), D<double>(c, D_SX), D<double>(c, D_SY),
               D<int32_t>(c, D_SBOX), D<uint8_t>(c, D_SPICK), D<int32_t>(c, D_SMG),
               D<int32_t>(c, D_FWDCNT), D<int64_t>(c, D_FWDOFF), D<int32_t>(c, D_EDST),
               want_ji ? D<double>(c, D_EJI) : nullptr);

  static const char* cc_names[7] = {"k4_init",     "k4_union",    "k4_compress", "k4_stats",
                                    "k4_ins_keys", "k4_comp_min", "k4_target"};
  for (int phase = 0; phase < 7; ++phase) {
    if ((phase == 5 || phase == 6) && !get_cc) continue;
    TRY(mark(c, cc_names[phase]));
    launch_cc(s, phase, (int)N, n_mg, k, get_cc, bo, D<int32_t>(c, D_BMG), D<uint8_t>(c, D_BPICK),
              D<int64_t>(c, D_FWDOFF), D<int32_t>(c, D_EDST), D<int32_t>(c, D_PARENT),
              D<uint8_t>(c, D_HASEDGE), D<int32_t>(c, D_CSIZE), D<MgStat>(c, D_STAT),
              D<unsigned long long>(c, D_INSKEY), D<unsigned long long>(c, D_COMPMIN), max_n);
  }

  CliqueArgs A;
  A.k = k; A.flags = get_cc | (multi << 1); A.n_mg = n_mg; A.n_roots = n_roots; A.C = 0;
  A.B = B; A.two_b2 = two_b2;
  A.box_off = bo; A.p0off = d_p0; A.id_base = d_id;
  A.x = x; A.y = y; A.score = sc; A.bmg = D<int32_t>(c, D_BMG); A.bpick = D<uint8_t>(c, D_BPICK);
  A.fwd_off = D<int64_t>(c, D_FWDOFF); A.e_dst = D<int32_t>(c, D_EDST);
  A.parent = D<int32_t>(c, D_PARENT); A.st = D<MgStat>(c, D_STAT);
  A.ins_key = D<unsigned long long>(c, D_INSKEY); A.clique_off = D<int64_t>(c, D_COFF);
  A.vrow = D<int32_t>(c, D_VROW);
  A.pk = nullptr;
  A.ccount = D<int32_t>(c, D_CCOUNT); A.in_clique = D<uint8_t>(c, D_INCL);
  A.adjg = D<uint64_t>(c, D_ADJG); A.rbound = D<uint64_t>(c, D_RBOUND);
  A.rflag = D<uint8_t>(c, D_RFLAG); A.dfs_mg = D<uint8_t>(c, D_DFSMG); A.dfs_base = 0;
  A.root_box = D<int32_t>(c, D_ROOTBOX);
  A.exmask = nullptr; A.exlist = nullptr; A.excount = nullptr;
  A.members = nullptr; A.rows = nullptr; A.w = nullptr; A.conf = nullptr; A.consensus = nullptr;
  A.order = nullptr;
  int64_t* d_tot = D<int64_t>(c, D_TOTAL);   // [0] edges, [1] DFS cliques, [2] level, [3] rank
  int64_t* h_tot = H<int64_t>(c, H_TOTAL);
  TRY(mark(c, "k5_setup"));   // DFS routing, neighbourhood bitmaps
  launch_clique_setup(s, (int)N, A);
  TRY(mark(c, "k5_dfs_count"));   // (micrographs with a root of > RB_W neighbours only)
  if (launch_cliques_dfs(s, false, (int)N, A) != 0) return fail("unsupported k");
  launch_scan(s, N, D<int32_t>(c, D_CCOUNT), D<int64_t>(c, D_COFF), D<int64_t>(c, D_TILES),
              d_tot + 1);
  // prefix levels: count -> scan -> (host reads the size) -> fill, ping-pong item buffers
  LevelArgs L;
  L.D = 0; L.n_items = N; L.in_root = nullptr; L.in_M = nullptr; L.in_P = nullptr;
  L.cnt = nullptr; L.off = nullptr; L.out_root = nullptr; L.out_M = nullptr; L.out_P = nullptr;
  L.next_cnt = nullptr;
  int cur = 0;
  int64_t C1 = 0, C2 = 0;
  // k >= 3 without members in the outputs: the leaf level's cliques are generated inside their
  // epilogue (k5_leaf_epi), their members never written (the exact pass's excepted)
  const bool leaf_epi = !want_members && !multi && k >= 3;
  for (int lv = 0; lv <= k - 2; ++lv) {
    const bool first = lv == 0, leaf = lv == k - 2;
    L.D = lv;
    TRY(ensure_dev(c, D_LCNT, L.n_items * 4));
    TRY(ensure_dev(c, D_LOFF, (L.n_items + 1) * 8));
    TRY(ensure_dev(c, D_TILES, scan_tiles_needed(L.n_items + 1) * 8));
    L.cnt = D<int32_t>(c, D_LCNT);
    L.off = D<int64_t>(c, D_LOFF);
    // (the leaf level of k >= 3: its counts and marks came from the last fill, next_cnt)
    if (!(leaf && k >= 3)) {
      TRY(mark(c, leaf ? "k5_leaf_count" : "k5_level_count"));
      // (first level: L.cnt was zeroed with the per-box arrays; non-roots stay 0)
      if (launch_clique_level(s, first, leaf, false, A, L) != 0) return fail("unsupported k");
    }
    // (the leaf level of the fused leaf epilogue: its scan also records the prefix holding
    // each wave's first clique; C1 <= 64 n_items, so at most n_items / 2 + 1 waves)
    int32_t* lbucket = nullptr;
    if (leaf && leaf_epi) {
      TRY(ensure_dev(c, D_LBUCKET, ((size_t)L.n_items / 2 + 2) * 4));
      lbucket = D<int32_t>(c, D_LBUCKET);
    }
    launch_scan(s, L.n_items, L.cnt, D<int64_t>(c, D_LOFF), D<int64_t>(c, D_TILES), d_tot + 2,
                lbucket, LEAF_Q);
    HIPCHK(hipMemcpyAsync(h_tot + 1, d_tot + 1, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    const int64_t nn = h_tot[2];
    C2 = h_tot[1];
    if (nn < 0 || C2 < 0) return fail("clique scan: look-back guard exhausted (stale tile buffer)");
    if (leaf) {
      C1 = nn;
      break;
    }
    const int o = cur ^ 1;
    TRY(ensure_dev(c, D_LROOT0 + o, nn * 4));
    TRY(ensure_dev(c, D_LM0 + o, nn * 8));
    TRY(ensure_dev(c, D_LP0 + o, nn * 8));
    L.out_root = D<int32_t>(c, D_LROOT0 + o);
    L.out_M = D<uint64_t>(c, D_LM0 + o);
    L.out_P = D<uint64_t>(c, D_LP0 + o);
    // the last fill's children are the leaf prefixes: it writes their leaf counts into the
    // count buffer (this level's counts are dead after the scan; sized here so the leaf
    // iteration's ensure_dev keeps it) and marks the clique vertices
    L.next_cnt = nullptr;
    if (lv == k - 3) {
      TRY(ensure_dev(c, D_LCNT, nn * 4));
      L.next_cnt = D<int32_t>(c, D_LCNT);
    }
    TRY(mark(c, "k5_level_fill"));
    launch_clique_level(s, first, false, true, A, L);
    L.next_cnt = nullptr;
    L.in_root = L.out_root; L.in_M = L.out_M; L.in_P = L.out_P;
    L.n_items = nn;
    cur = o;
  }
  // row ranks need only the clique-vertex flags of the count passes (bucket counters in
  // D_VLIST, slots in D_CSIZE: the CC sizes are dead by now; buckets in D_FWDCNT, dead since
  // the edge scan)
  TRY(mark(c, "k7_rank"));
  launch_rank(s, (int)N, n_mg, k, bo, D<int32_t>(c, D_BMG), D<MgGrid>(c, D_GRID), x, y,
              D<uint8_t>(c, D_INCL), D<int32_t>(c, D_VLIST), D<int32_t>(c, D_CSIZE),
              D<int32_t>(c, D_FWDCNT), D<int64_t>(c, D_BOFF), D<int64_t>(c, D_TILES), d_tot + 3,
              D<int32_t>(c, D_VSORT), D<int32_t>(c, D_VROW), D<MgStat>(c, D_STAT));
  const int64_t C = C1 + C2;
  *C_out = C;
  TRY(ensure_outputs(c, out_base + C, out_base, k, true, multi != 0));
  A.C = C;
  A.dfs_base = C1;
  A.members = D<int32_t>(c, D_MEMBERS) + out_base * k;
  A.rows = D<int32_t>(c, D_ROWS) + out_base * k;
  A.w = D<float>(c, D_W) + out_base;
  A.conf = D<float>(c, D_CONF) + out_base;
  A.consensus = D<int32_t>(c, D_CONS) + out_base;
  A.order = multi ? D<uint8_t>(c, D_ORDER) + out_base * k : nullptr;
  if (!leaf_epi) {
    TRY(mark(c, "k5_leaf_fill"));
    launch_clique_level(s, k == 2, true, true, A, L);
  }
  TRY(mark(c, "k5_dfs_fill"));
  launch_cliques_dfs(s, true, (int)N, A);
  // exact list [C], ballot words [ceil(C / 64)], per compaction wave: offsets and counts
  const int64_t exw = (C + 63) / 64, exnw = (exw + 63) / 64;
  TRY(ensure_dev(c, D_EXLIST, (C + exw + exnw + 1) * 8 + exnw * 4 + 16));
  TRY(ensure_dev(c, D_TILES, scan_tiles_needed(exnw + 1) * 8));
  A.exlist = D<int64_t>(c, D_EXLIST);
  A.exmask = reinterpret_cast<uint64_t*>(A.exlist + C);
  A.exwoff = reinterpret_cast<int64_t*>(A.exmask + exw);
  A.exwtot = reinterpret_cast<int32_t*>(A.exwoff + exnw + 1);
  A.tiles = D<int64_t>(c, D_TILES);
  // the exact list's length: the compaction scan's total (the rank scan's total is dead)
  A.excount = reinterpret_cast<unsigned long long*>(d_tot + 3);
  TRY(ensure_dev(c, D_PK, (size_t)N * 16));
  A.pk = D<double>(c, D_PK);
  // the epilogues set one bit per clique for the exact pass in these words
  HIPCHK(hipMemsetAsync(A.exmask, 0, exw * 8, s));
  TRY(mark(c, "k5_pack"));
  launch_clique_pack(s, (int)N, A);
  A.epi_lo = 0;
  if (leaf_epi) {
    TRY(mark(c, "k5_leaf_epi"));
    // (the prefix holding each wave's first clique: written by the leaf level's scan)
    if (launch_clique_leaf_epi(s, A, L, D<int32_t>(c, D_LBUCKET), C1) != 0)
      return fail("unsupported k");
    A.epi_lo = C1;   // k5_epilogue: the DFS route's cliques only
  }
  TRY(mark(c, "k5_epilogue"));
  launch_clique_epilogue(s, false, A);
  TRY(mark(c, "k5_epi_exact"));
  launch_clique_epilogue(s, true, A);
  TRY(mark(c, "k5_ranges"));
  launch_clique_ranges(s, A, C1, D<int64_t>(c, D_RLO), D<int64_t>(c, D_RLO) + n_mg,
                       leaf_epi ? L.in_root : nullptr, leaf_epi ? L.off : nullptr,
                       leaf_epi ? L.n_items : 0);
  HIPCHK(hipMemcpyAsync(H<void>(c, H_STAT), D<void>(c, D_STAT), n_mg * sizeof(MgStat),
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(H<void>(c, H_MGOFF), D<void>(c, D_RLO), 2 * (size_t)n_mg * 8,
                        hipMemcpyDeviceToHost, s));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s));
  const MgStat* st = H<MgStat>(c, H_STAT);
  const int64_t* rlo = H<int64_t>(c, H_MGOFF);
  const int64_t* rhi = rlo + n_mg;
  st_out.assign(st, st + n_mg);
  for (int m = 0; m < n_mg; ++m) {
    st_out[m].clique_base = out_base + rlo[m];
    st_out[m].clique_cnt = rhi[m] - rlo[m];
    if (st_out[m].status == RGC_OK && st_out[m].clique_cnt == 0) st_out[m].status = RGC_NO_CLIQUES;
  }
  return 0;
}
