// rgc_agree_host.cpp — host orchestration of rgc_agreement (kernels: rgc_agree.hip): the checked
// call, each segment's finite boxes sorted by x, the preset outputs, the partner launch, the
// mutual launch, and the results in the context's host block.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "rgc_host.h"

namespace {

constexpr int64_t AGREE_BOX_MAX = (int64_t)1 << 26;

}  // namespace

extern "C" int rgc_agreement(rgc_ctx* c, const rgc_agree_in* in, rgc_agree_out* out) {
  if (!c || !in || !out) return fail("null argument");
  const std::string who = "rgc_agreement";
  if (c->pend) return fail(who + ": a submitted run awaits rgc_wait on this context");
  const int64_t k = in->k;
  if (k < 1 || k > rgc::MAX_K) return fail(who + ": k must be in 1..8");
  if (in->n_mg < 0 || (int64_t)in->n_mg * k > INT32_MAX) return fail(who + ": n_mg out of range");
  if (in->box_size < 1 || in->box_size > AGREE_BOX_MAX)
    return fail(who + ": box_size must be in 1..2^26");
  const double t = in->ji_threshold;
  if (!(t >= 0.0 && t < 1.0))   // (false for NaN)
    return fail(who + ": ji_threshold must be finite and in [0, 1)");
  const int64_t n_seg = (int64_t)in->n_mg * k;
  if (n_seg > 0) {
    if (!in->box_off) return fail("null argument");
    if (in->box_off[0] != 0) return fail(who + ": box_off must start at 0");
    for (int64_t s = 0; s < n_seg; ++s) {
      if (in->box_off[s + 1] < in->box_off[s])
        return fail(who + ": box_off must be non-decreasing");
      if (in->box_off[s + 1] > INT32_MAX)
        return fail(who + ": more than 2^31 - 1 boxes in one call");
    }
  }
  const int64_t n = n_seg ? in->box_off[n_seg] : 0;
  if (n && (!in->x || !in->y)) return fail("null argument");
  c->times.clear();
  c->time_names.clear();
  c->agree_h2d = c->agree_d2h = 0;
  std::memset(out, 0, sizeof(*out));
  if (n_seg == 0) return 0;

  const bool partners = (in->flags & RGC_F_PARTNERS) != 0;
  const size_t nz = (size_t)n, np = (size_t)(n_seg * k), nk = nz * (size_t)k;
  // the host block: the three pair matrices, then partner_ji, partner, support
  const size_t o_ji = 3 * np * 8, o_part = o_ji + (partners ? nk * 8 : 0),
               o_sup = o_part + (partners ? nk * 4 : 0);
  HIPCHK(hipSetDevice(c->device));
  TRY(ensure_host(c, H_AG_OUT, o_sup + nz));
  char* hb = H<char>(c, H_AG_OUT);
  out->pair_edges = reinterpret_cast<int64_t*>(hb);
  out->pair_supported = out->pair_edges + np;
  out->pair_mutual = out->pair_supported + np;
  out->support = reinterpret_cast<uint8_t*>(hb + o_sup);
  if (partners) {
    out->partner_ji = reinterpret_cast<double*>(hb + o_ji);
    out->partner = reinterpret_cast<int32_t*>(hb + o_part);
  }
  std::memset(hb, 0, 3 * np * 8);
  if (n == 0) return 0;

  // the device layout: per segment its boxes with finite coordinates in ascending x (ties: file
  // order); the launch list holds the segments that have one (k = 1: no other picker, nothing
  // to launch)
  std::vector<double> sxy(2 * nz, 0.0);
  std::vector<int32_t> sidx(nz, 0), ns((size_t)n_seg, 0), seg, idx;
  double* sx = sxy.data();
  double* sy = sx + nz;
  if (k > 1)
    for (int64_t s = 0; s < n_seg; ++s) {
      const int64_t b0 = in->box_off[s], m = in->box_off[s + 1] - b0;
      const double* x = in->x + b0;
      const double* y = in->y + b0;
      idx.clear();
      for (int64_t i = 0; i < m; ++i)
        if (std::isfinite(x[i]) && std::isfinite(y[i])) idx.push_back((int32_t)i);
      std::stable_sort(idx.begin(), idx.end(), [x](int32_t a, int32_t b) { return x[a] < x[b]; });
      for (size_t j = 0; j < idx.size(); ++j) {
        sx[b0 + j] = x[idx[j]];
        sy[b0 + j] = y[idx[j]];
        sidx[b0 + j] = idx[j];
      }
      ns[s] = (int32_t)idx.size();
      if (!idx.empty()) seg.push_back((int32_t)s);
    }
  const int64_t nl = (int64_t)seg.size();
  if (nl == 0) {   // every mask 0, every partner -1
    std::memset(out->support, 0, nz);
    if (partners) {
      std::memset(out->partner, 0xFF, nk * 4);
      std::memset(out->partner_ji, 0, nk * 8);
    }
    return 0;
  }

  TRY(ensure_dev(c, D_AG_OFF, (size_t)(n_seg + 1) * 8));
  TRY(ensure_dev(c, D_AG_NS, (size_t)n_seg * 4));
  TRY(ensure_dev(c, D_AG_SEG, (size_t)nl * 4));
  TRY(ensure_dev(c, D_AG_SXY, nz * 16));
  TRY(ensure_dev(c, D_AG_SIDX, nz * 4));
  TRY(ensure_dev(c, D_AG_SUP, nz));
  TRY(ensure_dev(c, D_AG_PART, nk * 4));
  if (partners) TRY(ensure_dev(c, D_AG_PJI, nk * 8));
  TRY(ensure_dev(c, D_AG_PAIR, 3 * np * 8));
  hipStream_t st = c->stream;
  HIPCHK(hipMemcpyAsync(c->d[D_AG_OFF].p, in->box_off, (size_t)(n_seg + 1) * 8, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d[D_AG_NS].p, ns.data(), (size_t)n_seg * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d[D_AG_SEG].p, seg.data(), (size_t)nl * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d[D_AG_SXY].p, sxy.data(), nz * 16, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(c->d[D_AG_SIDX].p, sidx.data(), nz * 4, hipMemcpyHostToDevice, st));
  c->agree_h2d = (n_seg + 1) * 8 + n_seg * 4 + nl * 4 + n * 20;
  HIPCHK(hipMemsetAsync(c->d[D_AG_SUP].p, 0, nz, st));
  HIPCHK(hipMemsetAsync(c->d[D_AG_PART].p, 0xFF, nk * 4, st));
  if (partners) HIPCHK(hipMemsetAsync(c->d[D_AG_PJI].p, 0, nk * 8, st));
  HIPCHK(hipMemsetAsync(c->d[D_AG_PAIR].p, 0, 3 * np * 8, st));
  rgc::AgreeArgs A{};
  A.k = (int)k;
  A.n_box = n;
  A.off = D<int64_t>(c, D_AG_OFF);
  A.ns = D<int32_t>(c, D_AG_NS);
  A.seg = D<int32_t>(c, D_AG_SEG);
  A.sx = D<double>(c, D_AG_SXY);
  A.sy = A.sx + nz;
  A.sidx = D<int32_t>(c, D_AG_SIDX);
  A.B = (double)in->box_size;
  A.two_b2 = (double)(2 * in->box_size * in->box_size);
  A.t = t;
  A.support = D<uint8_t>(c, D_AG_SUP);
  A.partner = D<int32_t>(c, D_AG_PART);
  A.partner_ji = partners ? D<double>(c, D_AG_PJI) : nullptr;
  A.pair_edges = D<int64_t>(c, D_AG_PAIR);
  A.pair_supported = A.pair_edges + np;
  A.pair_mutual = A.pair_supported + np;
  const bool timing = (in->flags & RGC_F_TIMING) != 0;
  CallEvents E;   // before, between and after the two launches
  if (timing)
    for (int i = 0; i < 3; ++i) HIPCHK(hipEventCreate(&E.ev[i]));

  if (timing) HIPCHK(hipEventRecord(E.ev[0], st));
  rgc::launch_agree_partner(st, (int)nl, A);
  HIPCHK(hipGetLastError());
  if (timing) HIPCHK(hipEventRecord(E.ev[1], st));
  // the partners of every segment are complete at the launch boundary
  rgc::launch_agree_mutual(st, (int)nl, A);
  HIPCHK(hipGetLastError());
  if (timing) HIPCHK(hipEventRecord(E.ev[2], st));
  HIPCHK(hipMemcpyAsync(out->support, A.support, nz, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(out->pair_edges, A.pair_edges, 3 * np * 8, hipMemcpyDeviceToHost, st));
  c->agree_d2h = n + (int64_t)(3 * np * 8);
  if (partners) {
    HIPCHK(hipMemcpyAsync(out->partner, A.partner, nk * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out->partner_ji, A.partner_ji, nk * 8, hipMemcpyDeviceToHost, st));
    c->agree_d2h += (int64_t)(nk * 12);
  }
  HIPCHK(hipStreamSynchronize(st));
  if (timing) {
    TRY(section_time(c, E.ev[0], E.ev[1], "k_agree_partner"));
    TRY(section_time(c, E.ev[1], E.ev[2], "k_agree_mutual"));
  }
  return 0;
}

extern "C" int rgc_agreement_last_bytes(rgc_ctx* c, int64_t* h2d, int64_t* d2h) {
  if (!c || !h2d || !d2h) return fail("null argument");
  *h2d = c->agree_h2d;
  *d2h = c->agree_d2h;
  return 0;
}
