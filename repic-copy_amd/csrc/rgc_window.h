// rgc_window.h — the x-window of a sorted segment, shared by rgc_nms.hip and rgc_agree.hip.
#pragma once
#include "rgc_device.h"

namespace rgc {

// The window [lo, hi) of the segment's sorted boxes whose x lies in (xi - B, xi + B), widened by
// a few ulps of |xi| + B: an x overlap needs fl(min + B) > max, which the roundings of that sum
// and of the bounds here can move by at most two ulps of |xi| + B each.  The window only has to
// hold every conflicting box; the exact test decides.
__device__ __forceinline__ void nms_window(const double* sx, int ns, double xi, double B, int& lo,
                                           int& hi) {
  const double m = (fabs(xi) + B) * 0x1p-50;
  const double xl = (xi - B) - m, xh = (xi + B) + m;
  int l = 0, h = ns;
  while (l < h) {               // first x > xl
    const int mid = (l + h) >> 1;
    if (sx[mid] > xl) h = mid; else l = mid + 1;
  }
  lo = l;
  h = ns;
  while (l < h) {               // first x >= xh
    const int mid = (l + h) >> 1;
    if (sx[mid] >= xh) h = mid; else l = mid + 1;
  }
  hi = l;
}

}  // namespace rgc
