// rgc_score_host.cpp — rgc_score_pairs and rgc_score_sweep: tiling and launch of the
// score_detections raster kernels (rgc_score.hip).
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
