// rgc_score_host.cpp — rgc_score_pairs and rgc_score_sweep: tiling and launch of the
// score_detections raster kernels (rgc_score.hip); rgc_score_match and rgc_score_match_sweep:
// layout, the two launches and the hand-back of the particle-level matching (rgc_match.hip).
#include <algorithm>

#include "rgc_host.h"

namespace {

// What both entry points share: the checks of the pairs and their boxes, and the tiles.
struct ScorePlan {
  int64_t np = 0, nb = 0;
  int R = 0, TW = 0;
  std::vector<int> tp, tr, tw;   // per tile: pair, first row, first 64-pixel word
};

// Checks `in` and plans the tiles; no device work beyond hipSetDevice.  np == 0 leaves the plan
// empty (the caller returns 0).
int score_plan(rgc_ctx* c, const rgc_score_in* in, const char* who, ScorePlan& P) {
  if (c->pend) return fail(std::string(who) + ": a submitted run awaits rgc_wait on this context");
  HIPCHK(hipSetDevice(c->device));
  const int64_t np = in->n_pairs;
  if (np < 0 || np > INT32_MAX) return fail("n_pairs out of range");
  c->times.clear();
  c->time_names.clear();
  P.np = np;
  if (np == 0) return 0;
  const int64_t nb = std::max(in->pk_off[np], in->gt_off[np]);   // boxes in the array
  if (in->gt_off[0] < 0 || in->pk_off[0] < 0) return fail("negative box offset");
  // tiles: R rows x TW words, R * TW = the kernel's LDS words per mask
  const int words_cap = rgc::score_tile_words();
  int64_t maxw = 1;
  for (int64_t p = 0; p < np; ++p) maxw = std::max<int64_t>(maxw, (in->width[p] + 63) / 64);
  const int TW = (int)std::min<int64_t>(maxw, 32);
  const int R = words_cap / TW;
  for (int64_t p = 0; p < np; ++p) {
    const int64_t H = in->height[p], W = in->width[p];
    if (H < 0 || W < 0 || H > (1 << 30) || W > (1 << 30)) return fail("mask size out of range");
    if (in->gt_off[p + 1] < in->gt_off[p] || in->pk_off[p + 1] < in->pk_off[p] ||
        in->pk_off[p + 1] > nb)
      return fail("box offsets must be non-decreasing and within the box array");
    for (int which = 0; which < 2; ++which) {
      const int64_t* off = which ? in->pk_off : in->gt_off;
      for (int64_t b = off[p]; b < off[p + 1]; ++b) {
        const int32_t* q = in->boxes + 4 * b;
        if (!(0 <= q[0] && q[0] < q[1] && q[1] <= H && 0 <= q[2] && q[2] < q[3] && q[3] <= W))
          return fail("box " + std::to_string(b) + " is not a normalised non-empty slice");
      }
    }
    const int64_t nw = (W + 63) / 64;
    for (int64_t r0 = 0; r0 < H; r0 += R)
      for (int64_t w0 = 0; w0 < nw; w0 += TW) {
        // (lvalues: the push_back instantiation the rest of the library already has)
        const int ip = (int)p, ir = (int)r0, iw = (int)w0;
        P.tp.push_back(ip);
        P.tr.push_back(ir);
        P.tw.push_back(iw);
      }
  }
  if ((int64_t)P.tp.size() > INT32_MAX) return fail("too many tiles");
  P.nb = nb;
  P.R = R;
  P.TW = TW;
  return 0;
}

// Uploads the planned call, zeroes cnt_bytes of counters, runs `launch(stream, n_tiles, args)`
// (timed as `kname` with RGC_F_TIMING) and copies the counters to `counts`.
template <typename Launch>
int score_launch(rgc_ctx* c, const rgc_score_in* in, const ScorePlan& P, size_t cnt_bytes,
                 const char* kname, int64_t* counts, Launch launch) {
  const int64_t np = P.np, nb = P.nb, nt = (int64_t)P.tp.size();
  TRY(ensure_dev(c, D_SC_BOX, (size_t)nb * 16));
  TRY(ensure_dev(c, D_SC_GOFF, (size_t)(np + 1) * 8));
  TRY(ensure_dev(c, D_SC_POFF, (size_t)(np + 1) * 8));
  TRY(ensure_dev(c, D_SC_TP, (size_t)nt * 4));
  TRY(ensure_dev(c, D_SC_TR, (size_t)nt * 4));
  TRY(ensure_dev(c, D_SC_TW, (size_t)nt * 4));
  TRY(ensure_dev(c, D_SC_CNT, cnt_bytes));
  hipStream_t s = c->stream;
  if (nb) HIPCHK(hipMemcpyAsync(c->d[D_SC_BOX].p, in->boxes, (size_t)nb * 16, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_SC_GOFF].p, in->gt_off, (size_t)(np + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_SC_POFF].p, in->pk_off, (size_t)(np + 1) * 8, hipMemcpyHostToDevice, s));
  if (nt) {
    HIPCHK(hipMemcpyAsync(c->d[D_SC_TP].p, P.tp.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d[D_SC_TR].p, P.tr.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d[D_SC_TW].p, P.tw.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemsetAsync(c->d[D_SC_CNT].p, 0, cnt_bytes, s));
  rgc::ScoreArgs A;
  A.boxes = D<int4>(c, D_SC_BOX);
  A.gt_off = D<int64_t>(c, D_SC_GOFF);
  A.pk_off = D<int64_t>(c, D_SC_POFF);
  A.tile_pair = D<int>(c, D_SC_TP);
  A.tile_r0 = D<int>(c, D_SC_TR);
  A.tile_w0 = D<int>(c, D_SC_TW);
  A.R = P.R;
  A.TW = P.TW;
  A.counts = D<unsigned long long>(c, D_SC_CNT);
  const bool timing = (in->flags & RGC_F_TIMING) != 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (timing) {
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, s));
  }
  launch(s, (int)nt, A);
  HIPCHK(hipGetLastError());
  if (timing) HIPCHK(hipEventRecord(e1, s));
  HIPCHK(hipMemcpyAsync(counts, c->d[D_SC_CNT].p, cnt_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (timing) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    c->times.push_back(ms);
    c->time_names.push_back(kname);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return 0;
}

}  // namespace

extern "C" int rgc_score_pairs(rgc_ctx* c, const rgc_score_in* in, int64_t* counts) {
  if (!c || !in || !counts) return fail("null argument");
  ScorePlan P;
  TRY(score_plan(c, in, "rgc_score_pairs", P));
  if (P.np == 0) return 0;
  return score_launch(c, in, P, (size_t)P.np * 24, "k_score_raster", counts,
                      rgc::launch_score_raster);
}

// ---- particle-level matching (rgc_match.hip)
namespace {

constexpr int64_t MT_XY_MAX = (int64_t)1 << 30;     // |x0|, |y0|
constexpr int64_t MT_SIDE_MAX = (int64_t)1 << 25;   // x1 - x0, y1 - y0

// the section between two events as `name` (RGC_F_TIMING)
int match_time(rgc_ctx* c, hipEvent_t e0, hipEvent_t e1, const char* name) {
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  c->times.push_back(ms);
  c->time_names.push_back(name);
  return 0;
}

// What rgc_score_match and rgc_score_match_sweep share: the checked call, its device layout on
// the host, the kernels' arguments and the events of a timed call.
struct MatchPlan {
  int64_t np = 0, nb = 0;
  std::vector<int32_t> box, perm, ngt, wmax;   // perm: the caller's index of each sorted box
  std::vector<int64_t> base, ebase;            // ebase: uploaded by a copy the caller waits for
  rgc::MatchArgs A{};
  bool timing = false;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~MatchPlan() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// Checks `in` and lays the pairs out; no device work.  np == 0 leaves the plan empty (the
// caller returns 0).  Messages name `who`.
int match_layout(rgc_ctx* c, const rgc_score_match_in* in, const std::string& who, MatchPlan& P) {
  if (c->pend) return fail(who + ": a submitted run awaits rgc_wait on this context");
  const int64_t np = in->n_pairs;
  if (np < 0 || np > INT32_MAX) return fail("n_pairs out of range");
  const double t = in->ji_threshold;
  if (!(t >= 0.0 && t < 1.0))   // (false for NaN)
    return fail(who + ": ji_threshold must be finite and in [0, 1)");
  c->times.clear();
  c->time_names.clear();
  P.np = np;
  if (np == 0) return 0;
  if (!in->gt_off || !in->pk_off) return fail("null argument");
  if (in->gt_off[0] < 0 || in->pk_off[0] < 0) return fail("negative box offset");
  int64_t nb = 0;
  for (int64_t p = 0; p < np; ++p) {
    if (in->gt_off[p + 1] < in->gt_off[p] || in->pk_off[p + 1] < in->pk_off[p])
      return fail("box offsets must be non-decreasing");
    const int64_t dg = in->gt_off[p + 1] - in->gt_off[p], dk = in->pk_off[p + 1] - in->pk_off[p];
    if (dg <= INT32_MAX && dk <= INT32_MAX) nb += dg + dk;
    if (dg > INT32_MAX || dk > INT32_MAX || nb > INT32_MAX) return fail(who + ": more than 2^31 - 1 boxes in one call");
  }
  if (nb && !in->boxes) return fail("null argument");
  // the device layout: pair after pair, its ground truth ascending in x0 (ties: the caller's
  // order), then its picks; perm = the caller's index of each sorted ground-truth box
  P.nb = nb;
  P.box.resize((size_t)nb * 4);
  P.perm.resize((size_t)nb);
  P.ngt.resize((size_t)np);
  P.wmax.resize((size_t)np);
  P.base.resize((size_t)np + 1);
  std::vector<int32_t> idx;
  int64_t at = 0;
  for (int64_t p = 0; p < np; ++p) {
    P.base[p] = at;
    const int64_t g0 = in->gt_off[p], ng = in->gt_off[p + 1] - g0;
    const int64_t k0 = in->pk_off[p], nk = in->pk_off[p + 1] - k0;
    for (int which = 0; which < 2; ++which) {
      const int64_t b0 = which ? k0 : g0, n = which ? nk : ng;
      for (int64_t b = b0; b < b0 + n; ++b) {
        const int32_t* q = in->boxes + 4 * b;
        if (q[0] > MT_XY_MAX || q[0] < -MT_XY_MAX || q[2] > MT_XY_MAX || q[2] < -MT_XY_MAX ||
            (int64_t)q[1] - q[0] > MT_SIDE_MAX || (int64_t)q[3] - q[2] > MT_SIDE_MAX)
          return fail(who + ": box " + std::to_string(b) +
                      " is out of range (|x0|, |y0| <= 2^30, sides <= 2^25)");
      }
    }
    idx.resize((size_t)ng);
    for (int64_t i = 0; i < ng; ++i) idx[i] = (int32_t)i;
    const int32_t* gb = in->boxes + 4 * g0;
    std::stable_sort(idx.begin(), idx.end(),
                     [gb](int32_t a, int32_t b) { return gb[4 * a] < gb[4 * b]; });
    int32_t wm = 0;
    for (int64_t i = 0; i < ng; ++i) {
      const int32_t* q = gb + 4 * idx[i];
      std::copy(q, q + 4, P.box.begin() + 4 * (at + i));
      P.perm[at + i] = idx[i];
      if (q[1] > q[0] && q[3] > q[2]) wm = std::max<int32_t>(wm, q[1] - q[0]);
    }
    if (nk) std::copy(in->boxes + 4 * k0, in->boxes + 4 * (k0 + nk), P.box.begin() + 4 * (at + ng));
    P.ngt[p] = (int32_t)ng;
    P.wmax[p] = wm;
    at += ng + nk;
  }
  P.base[np] = at;
  P.A.t = t;
  P.timing = (in->flags & RGC_F_TIMING) != 0;
  return 0;
}

// Uploads the layout, runs the count launch (between ev[0] and ev[1] of a timed call), sizes
// the edge lists from its per-pair totals and uploads their bases: P.A is then complete.
int match_count(rgc_ctx* c, const std::string& who, MatchPlan& P) {
  const int64_t np = P.np, nb = P.nb;
  HIPCHK(hipSetDevice(c->device));
  const size_t nbz = (size_t)nb;
  TRY(ensure_dev(c, D_MT_BOX, nbz * 16));
  TRY(ensure_dev(c, D_MT_BASE, (size_t)(np + 1) * 8));
  TRY(ensure_dev(c, D_MT_NGT, (size_t)np * 4));
  TRY(ensure_dev(c, D_MT_WMAX, (size_t)np * 4));
  TRY(ensure_dev(c, D_MT_STATE, nbz * 4 * 6));   // deg, rowp, mate, par, lvl, found
  TRY(ensure_dev(c, D_MT_ETOT, (size_t)np * 8));
  TRY(ensure_dev(c, D_MT_EBASE, (size_t)np * 8));
  TRY(ensure_dev(c, D_MT_TP, (size_t)np * 8));
  TRY(ensure_dev(c, D_MT_STAT, (size_t)np * 4));
  hipStream_t s = c->stream;
  if (nb) HIPCHK(hipMemcpyAsync(c->d[D_MT_BOX].p, P.box.data(), nbz * 16, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_MT_BASE].p, P.base.data(), (size_t)(np + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_MT_NGT].p, P.ngt.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_MT_WMAX].p, P.wmax.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
  rgc::MatchArgs& A = P.A;
  A.boxes = D<int4>(c, D_MT_BOX);
  A.base = D<int64_t>(c, D_MT_BASE);
  A.n_gt = D<int32_t>(c, D_MT_NGT);
  A.gt_wmax = D<int32_t>(c, D_MT_WMAX);
  int32_t* st = D<int32_t>(c, D_MT_STATE);
  A.deg = st;
  A.rowp = st + nbz;
  A.mate = st + 2 * nbz;
  A.par = st + 3 * nbz;
  A.lvl = st + 4 * nbz;
  A.found = st + 5 * nbz;
  A.etot = D<int64_t>(c, D_MT_ETOT);
  A.ebase = D<int64_t>(c, D_MT_EBASE);
  A.tp = D<int64_t>(c, D_MT_TP);
  A.status = D<int32_t>(c, D_MT_STAT);
  if (P.timing)
    for (hipEvent_t& e : P.ev) HIPCHK(hipEventCreate(&e));
  // the count launch; its per-pair totals size the edge lists
  if (P.timing) HIPCHK(hipEventRecord(P.ev[0], s));
  rgc::launch_match_count(s, (int)np, A);
  HIPCHK(hipGetLastError());
  if (P.timing) HIPCHK(hipEventRecord(P.ev[1], s));
  std::vector<int64_t> etot((size_t)np);
  P.ebase.resize((size_t)np);
  HIPCHK(hipMemcpyAsync(etot.data(), c->d[D_MT_ETOT].p, (size_t)np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int64_t ne = 0;
  for (int64_t p = 0; p < np; ++p) {
    P.ebase[p] = ne;
    ne += etot[p];
    if (etot[p] < 0 || ne > INT32_MAX) return fail(who + ": more than 2^31 - 1 edges in one call");
  }
  TRY(ensure_dev(c, D_MT_ADJ, (size_t)ne * 4));
  A.adj = D<int32_t>(c, D_MT_ADJ);
  HIPCHK(hipMemcpyAsync(c->d[D_MT_EBASE].p, P.ebase.data(), (size_t)np * 8, hipMemcpyHostToDevice, s));
  return 0;
}

// the first pair whose status says it ran into a loop bound
int match_status(const std::string& who, const std::vector<int32_t>& status) {
  for (size_t p = 0; p < status.size(); ++p)
    if (status[p] != 0)
      return fail(who + ": pair " + std::to_string(p) + " ran into a loop bound (status " +
                  std::to_string(status[p]) + ")");
  return 0;
}

}  // namespace

extern "C" int rgc_score_match(rgc_ctx* c, const rgc_score_match_in* in, int64_t* counts,
                               int32_t* match) {
  if (!c || !in || !counts) return fail("null argument");
  const std::string who = "rgc_score_match";
  MatchPlan P;
  TRY(match_layout(c, in, who, P));
  const int64_t np = P.np, nb = P.nb;
  if (np == 0) return 0;
  TRY(match_count(c, who, P));
  const rgc::MatchArgs& A = P.A;
  const size_t nbz = (size_t)nb;
  hipStream_t s = c->stream;
  if (P.timing) HIPCHK(hipEventRecord(P.ev[2], s));
  rgc::launch_match(s, (int)np, A);
  HIPCHK(hipGetLastError());
  if (P.timing) HIPCHK(hipEventRecord(P.ev[3], s));
  std::vector<int64_t> tp((size_t)np);
  std::vector<int32_t> status((size_t)np), mate;
  HIPCHK(hipMemcpyAsync(tp.data(), c->d[D_MT_TP].p, (size_t)np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(status.data(), c->d[D_MT_STAT].p, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  if (match && nb) {
    mate.resize(nbz);
    HIPCHK(hipMemcpyAsync(mate.data(), A.mate, nbz * 4, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  if (P.timing) {
    TRY(match_time(c, P.ev[0], P.ev[1], "k_score_match_count"));
    TRY(match_time(c, P.ev[2], P.ev[3], "k_score_match"));
  }
  TRY(match_status(who, status));
  int64_t out = 0;
  for (int64_t p = 0; p < np; ++p) {
    const int64_t ng = P.ngt[p], nk = P.base[p + 1] - P.base[p] - ng;
    counts[3 * p] = ng;
    counts[3 * p + 1] = nk;
    counts[3 * p + 2] = tp[p];
    if (match)
      for (int64_t u = 0; u < nk; ++u) {
        const int32_t g = mate[P.base[p] + ng + u];
        match[out + u] = g < 0 ? -1 : P.perm[P.base[p] + g];
      }
    out += nk;
  }
  return 0;
}

extern "C" int rgc_score_match_sweep(rgc_ctx* c, const rgc_score_match_sweep_in* in,
                                     int64_t* counts) {
  if (!c || !in || !counts) return fail("null argument");
  const std::string who = "rgc_score_match_sweep";
  const int64_t T = in->n_thr;
  if (T < 1 || T > RGC_MATCH_MAX_THR)
    return fail(who + ": n_thr " + std::to_string(T) + " is outside 1.." +
                std::to_string(RGC_MATCH_MAX_THR));
  const rgc_score_match_in* pi = &in->pairs;
  MatchPlan P;
  TRY(match_layout(c, pi, who, P));
  const int64_t np = P.np;
  if (np == 0) return 0;
  if (!in->keep) return fail("null argument");
  for (int64_t p = 0; p < np; ++p) {
    const int64_t n = pi->pk_off[p + 1] - pi->pk_off[p];
    const int64_t* k = in->keep + p * T;
    for (int64_t j = 0; j < T; ++j) {
      if (k[j] < 0 || k[j] > n)
        return fail(who + ": keep[" + std::to_string(p) + "][" + std::to_string(j) + "] = " +
                    std::to_string(k[j]) + " is outside the pair's " + std::to_string(n) +
                    " picks");
      if (j && k[j] > k[j - 1])
        return fail(who + ": keep[" + std::to_string(p) + "] increases at threshold " +
                    std::to_string(j) + " (thresholds ascend, so keep must not)");
    }
  }
  TRY(match_count(c, who, P));
  const size_t nt = (size_t)np * (size_t)T;
  TRY(ensure_dev(c, D_MT_KEEP, nt * 8));
  TRY(ensure_dev(c, D_MT_TPS, nt * 8));
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(c->d[D_MT_KEEP].p, in->keep, nt * 8, hipMemcpyHostToDevice, s));
  if (P.timing) HIPCHK(hipEventRecord(P.ev[2], s));
  rgc::launch_match_sweep(s, (int)np, P.A, (int)T, D<int64_t>(c, D_MT_KEEP),
                          D<int64_t>(c, D_MT_TPS));
  HIPCHK(hipGetLastError());
  if (P.timing) HIPCHK(hipEventRecord(P.ev[3], s));
  std::vector<int64_t> tp(nt);
  std::vector<int32_t> status((size_t)np);
  HIPCHK(hipMemcpyAsync(tp.data(), c->d[D_MT_TPS].p, nt * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(status.data(), c->d[D_MT_STAT].p, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (P.timing) {
    TRY(match_time(c, P.ev[0], P.ev[1], "k_score_match_count"));
    TRY(match_time(c, P.ev[2], P.ev[3], "k_score_match_sweep"));
  }
  TRY(match_status(who, status));
  for (int64_t p = 0; p < np; ++p)
    for (int64_t j = 0; j < T; ++j) {
      int64_t* q = counts + (p * T + j) * 3;
      q[0] = P.ngt[p];
      q[1] = in->keep[p * T + j];
      q[2] = tp[(size_t)(p * T + j)];
    }
  return 0;
}

extern "C" int rgc_score_sweep(rgc_ctx* c, const rgc_score_sweep_in* in, int64_t* counts) {
  if (!c || !in || !counts) return fail("null argument");
  const int64_t T = in->n_thr;
  if (T < 1 || T > RGC_SCORE_MAX_THR)
    return fail("rgc_score_sweep: n_thr " + std::to_string(T) + " is outside 1.." +
                std::to_string(RGC_SCORE_MAX_THR));
  const rgc_score_in* pi = &in->pairs;
  ScorePlan P;
  TRY(score_plan(c, pi, "rgc_score_sweep", P));
  const int64_t np = P.np;
  if (np == 0) return 0;
  if (!in->keep) return fail("null argument");
  for (int64_t p = 0; p < np; ++p) {
    const int64_t n = pi->pk_off[p + 1] - pi->pk_off[p];
    const int64_t* k = in->keep + p * T;
    for (int64_t j = 0; j < T; ++j) {
      if (k[j] < 0 || k[j] > n)
        return fail("rgc_score_sweep: keep[" + std::to_string(p) + "][" + std::to_string(j) +
                    "] = " + std::to_string(k[j]) + " is outside the pair's " +
                    std::to_string(n) + " picks");
      if (j && k[j] > k[j - 1])
        return fail("rgc_score_sweep: keep[" + std::to_string(p) + "] increases at threshold " +
                    std::to_string(j) + " (thresholds ascend, so keep must not)");
    }
  }
  const size_t kb = (size_t)np * T * 8;
  TRY(ensure_dev(c, D_SC_KEEP, kb));
  HIPCHK(hipMemcpyAsync(c->d[D_SC_KEEP].p, in->keep, kb, hipMemcpyHostToDevice, c->stream));
  const int64_t* dkeep = D<int64_t>(c, D_SC_KEEP);
  TRY(score_launch(c, pi, P, (size_t)np * T * 24, "k_score_sweep", counts,
                   [&](hipStream_t s, int nt, const rgc::ScoreArgs& A) {
                     rgc::launch_score_sweep(s, nt, A, (int)T, dkeep);
                   }));
  // the kernel counted the pixels that first appear at each threshold (walking down from the
  // highest) and sum(gt) once per pair: suffix sums give the counts at each threshold
  for (int64_t p = 0; p < np; ++p) {
    int64_t* q = counts + p * T * 3;
    const int64_t g = q[0];
    int64_t k = 0, tp = 0;
    for (int64_t j = T - 1; j >= 0; --j) {
      k += q[3 * j + 1];
      tp += q[3 * j + 2];
      q[3 * j] = g;
      q[3 * j + 1] = k;
      q[3 * j + 2] = tp;
    }
  }
  return 0;
}
