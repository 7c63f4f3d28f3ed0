// rgc_nms_host.cpp — host orchestration of rgc_nms (kernels: rgc_nms.hip): the checked call,
// each segment's finite boxes sorted by x, the count launch that sizes the conflict lists, the
// rounds launch, and the results back in the caller's layout.
#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>

#include "rgc_host.h"

namespace {

constexpr int64_t NMS_BOX_MAX = (int64_t)1 << 26;

}  // namespace

extern "C" int rgc_nms(rgc_ctx* c, const rgc_nms_in* in, uint8_t* keep, int64_t* kept) {
  if (!c || !in) return fail("null argument");
  const std::string who = "rgc_nms";
  if (c->pend) return fail(who + ": a submitted run awaits rgc_wait on this context");
  const int64_t n_seg = in->n_seg;
  if (n_seg < 0 || n_seg > INT32_MAX) return fail(who + ": n_seg out of range");
  if (in->box_size < 1 || in->box_size > NMS_BOX_MAX)
    return fail(who + ": box_size must be in 1..2^26");
  const double t = in->ji_threshold;
  if (!(t >= 0.0 && t < 1.0))   // (false for NaN)
    return fail(who + ": ji_threshold must be finite and in [0, 1)");
  c->times.clear();
  c->time_names.clear();
  c->nms_h2d = c->nms_d2h = 0;
  if (n_seg == 0) return 0;
  if (!in->seg_off || !kept) return fail("null argument");
  if (in->seg_off[0] != 0) return fail(who + ": seg_off must start at 0");
  for (int64_t p = 0; p < n_seg; ++p) {
    if (in->seg_off[p + 1] < in->seg_off[p])
      return fail(who + ": seg_off must be non-decreasing");
    if (in->seg_off[p + 1] > INT32_MAX)
      return fail(who + ": more than 2^31 - 1 boxes in one call");
  }
  const int64_t n = in->seg_off[n_seg];
  if (n && (!in->x || !in->y || !keep)) return fail("null argument");
  std::fill(kept, kept + n_seg, (int64_t)0);
  if (n == 0) return 0;

  // the device layout: the non-empty segments only (an empty one launches nothing); per segment
  // its boxes with finite coordinates in ascending x (ties: priority order)
  std::vector<int32_t> seg;   // the caller's index of each launched segment
  std::vector<int64_t> off;
  for (int64_t p = 0; p < n_seg; ++p)
    if (in->seg_off[p + 1] > in->seg_off[p]) {
      seg.push_back((int32_t)p);
      off.push_back(in->seg_off[p]);
    }
  off.push_back(n);   // (the launched segments tile [0, n): the boxes keep their positions)
  const int64_t np = (int64_t)seg.size();
  const size_t nz = (size_t)n;
  std::vector<double> sxy(2 * nz, 0.0);
  std::vector<int32_t> sidx(nz, 0), ns((size_t)np), idx;
  double* sx = sxy.data();
  double* sy = sx + nz;
  for (int64_t q = 0; q < np; ++q) {
    const int64_t b0 = off[q], m = off[q + 1] - b0;
    const double* x = in->x + b0;
    const double* y = in->y + b0;
    idx.clear();
    for (int64_t i = 0; i < m; ++i)
      if (std::isfinite(x[i]) && std::isfinite(y[i])) idx.push_back((int32_t)i);
    std::stable_sort(idx.begin(), idx.end(), [x](int32_t a, int32_t b) { return x[a] < x[b]; });
    for (size_t s = 0; s < idx.size(); ++s) {
      sx[b0 + s] = x[idx[s]];
      sy[b0 + s] = y[idx[s]];
      sidx[b0 + s] = idx[s];
    }
    ns[q] = (int32_t)idx.size();
  }

  HIPCHK(hipSetDevice(c->device));
  TRY(ensure_dev(c, D_NM_OFF, (size_t)(np + 1) * 8));
  TRY(ensure_dev(c, D_NM_NS, (size_t)np * 4));
  TRY(ensure_dev(c, D_NM_XY, nz * 16));
  TRY(ensure_dev(c, D_NM_SXY, nz * 16));
  TRY(ensure_dev(c, D_NM_SIDX, nz * 4));
  TRY(ensure_dev(c, D_NM_STATE, nz * 4 * 3));   // cnt, rowp, state
  TRY(ensure_dev(c, D_NM_ETOT, (size_t)np * 8));
  TRY(ensure_dev(c, D_NM_EBASE, (size_t)np * 8));
  TRY(ensure_dev(c, D_NM_KEEP, nz));
  TRY(ensure_dev(c, D_NM_KEPT, (size_t)np * 8));
  TRY(ensure_dev(c, D_NM_STAT, (size_t)np * 4));
  hipStream_t s = c->stream;
  double* dxy = D<double>(c, D_NM_XY);
  HIPCHK(hipMemcpyAsync(c->d[D_NM_OFF].p, off.data(), (size_t)(np + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_NM_NS].p, ns.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dxy, in->x, nz * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(dxy + nz, in->y, nz * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_NM_SXY].p, sxy.data(), nz * 16, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(c->d[D_NM_SIDX].p, sidx.data(), nz * 4, hipMemcpyHostToDevice, s));
  c->nms_h2d = (np + 1) * 8 + np * 4 + n * 36;
  rgc::NmsArgs A{};
  A.off = D<int64_t>(c, D_NM_OFF);
  A.ns = D<int32_t>(c, D_NM_NS);
  A.x = dxy;
  A.y = dxy + nz;
  A.sx = D<double>(c, D_NM_SXY);
  A.sy = A.sx + nz;
  A.sidx = D<int32_t>(c, D_NM_SIDX);
  A.B = (double)in->box_size;
  A.two_b2 = (double)(2 * in->box_size * in->box_size);
  A.t = t;
  int32_t* st = D<int32_t>(c, D_NM_STATE);
  A.cnt = st;
  A.rowp = st + nz;
  A.state = st + 2 * nz;
  A.etot = D<int64_t>(c, D_NM_ETOT);
  A.ebase = D<int64_t>(c, D_NM_EBASE);
  A.keep = D<uint8_t>(c, D_NM_KEEP);
  A.kept = D<int64_t>(c, D_NM_KEPT);
  A.status = D<int32_t>(c, D_NM_STAT);
  const bool timing = (in->flags & RGC_F_TIMING) != 0;
  CallEvents E;
  if (timing)
    for (hipEvent_t& e : E.ev) HIPCHK(hipEventCreate(&e));

  // the count launch; its per-segment totals size the conflict lists
  if (timing) HIPCHK(hipEventRecord(E.ev[0], s));
  rgc::launch_nms_count(s, (int)np, A);
  HIPCHK(hipGetLastError());
  if (timing) HIPCHK(hipEventRecord(E.ev[1], s));
  std::vector<int64_t> etot((size_t)np), ebase((size_t)np);
  HIPCHK(hipMemcpyAsync(etot.data(), c->d[D_NM_ETOT].p, (size_t)np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->nms_d2h = np * 8;
  int64_t ne = 0;
  for (int64_t q = 0; q < np; ++q) {
    ebase[q] = ne;
    if (etot[q] < 0 || etot[q] > INT32_MAX || (ne += etot[q]) > INT32_MAX)
      return fail(who + ": more than 2^31 - 1 conflict edges in one call");
  }
  TRY(ensure_dev(c, D_NM_ADJ, (size_t)ne * 4));
  A.adj = D<int32_t>(c, D_NM_ADJ);
  HIPCHK(hipMemcpyAsync(c->d[D_NM_EBASE].p, ebase.data(), (size_t)np * 8, hipMemcpyHostToDevice, s));
  c->nms_h2d += np * 8;

  if (timing) HIPCHK(hipEventRecord(E.ev[2], s));
  rgc::launch_nms(s, (int)np, A);
  HIPCHK(hipGetLastError());
  if (timing) HIPCHK(hipEventRecord(E.ev[3], s));
  std::vector<int64_t> kq((size_t)np);
  std::vector<int32_t> status((size_t)np);
  HIPCHK(hipMemcpyAsync(keep, A.keep, nz, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(kq.data(), A.kept, (size_t)np * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(status.data(), A.status, (size_t)np * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  c->nms_d2h += n + np * 12;
  if (timing) {
    TRY(section_time(c, E.ev[0], E.ev[1], "k_nms_count"));
    TRY(section_time(c, E.ev[2], E.ev[3], "k_nms"));
  }
  for (int64_t q = 0; q < np; ++q)
    if (status[q] != 0)
      return fail(who + ": segment " + std::to_string(seg[q]) +
                  (status[q] == rgc::NMS_ST_ROUNDS ? " ran out of rounds" : " has a broken conflict list") +
                  " (status " + std::to_string(status[q]) + ")");
  for (int64_t q = 0; q < np; ++q) kept[seg[q]] = kq[q];
  return 0;
}

extern "C" int rgc_nms_last_bytes(rgc_ctx* c, int64_t* h2d, int64_t* d2h) {
  if (!c || !h2d || !d2h) return fail("null argument");
  *h2d = c->nms_h2d;
  *d2h = c->nms_d2h;
  return 0;
}
