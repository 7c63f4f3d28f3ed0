// rgc_agree.hip — per-box picker support and pairwise picker agreement (rgc_agreement).
//
// Segment s = m * k + p holds the boxes of picker p of micrograph m.  Two boxes of the same
// micrograph and different pickers are joined iff is_edge() of rgc_device.h holds: |dx| <= B and
// the reference quotient (get_cliques.py:40-46,59-69, its f64 operation order) strictly above the
// threshold - the edge set of the consensus graph.  The quotient is symmetric in its two boxes
// bit for bit (min / max of the same pairs), so "joined" is symmetric.
//
//   k_agree_partner  one workgroup per segment with a finite box: per box and other picker q the
//                    number of joined boxes of (m, q) and the one with the largest JI (ties: the
//                    lowest batch index); the support mask, the partners, and per q the segment's
//                    joined pairs and supported boxes
//   k_agree_mutual   a second launch (the launch boundary makes the other segments' partners
//                    visible): per q the boxes whose partner's partner they are
//
// The host hands over each segment's finite boxes sorted by x (rgc_nms.hip's layout), so a box
// tests only the window of each other segment whose x can overlap its own; a box with a
// non-finite coordinate is in no list: it owns no thread and is in no window.  The host presets
// the outputs (0, partner -1), so what launches nothing reads as that.  Every output is a
// function of the inputs alone: counts are integer sums, and a best partner is a maximum under a
// total order.  No workgroup waits for another, and no segment size is compiled in.
#include "rgc_device.h"
#include "rgc_kernels.h"
#include "rgc_window.h"

namespace rgc {

constexpr int AGREE_WG = 256;

__global__ __launch_bounds__(AGREE_WG) void k_agree_partner(AgreeArgs A) {
  __shared__ int64_t red[AGREE_WG / 64][2 * MAX_K];
  const int tid = threadIdx.x, k = A.k;
  const int s = A.seg[blockIdx.x];
  const int m = s / k, p = s - m * k;
  const int64_t b0 = A.off[s];
  const int n = A.ns[s];
  // per other picker: joined pairs and supported boxes of this thread's boxes (the q loops are
  // unrolled over MAX_K, so the arrays are indexed by constants and stay in registers)
  int64_t ne[MAX_K];
  int nsup[MAX_K];
#pragma unroll
  for (int q = 0; q < MAX_K; ++q) { ne[q] = 0; nsup[q] = 0; }
  for (int i = tid; i < n; i += AGREE_WG) {
    const double xi = A.sx[b0 + i], yi = A.sy[b0 + i];
    const int64_t b = b0 + A.sidx[b0 + i];
    unsigned mask = 0;
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) {
      if (q >= k || q == p) continue;
      const int64_t c0 = A.off[m * k + q];
      const int nq = A.ns[m * k + q];
      int lo, hi;
      nms_window(A.sx + c0, nq, xi, A.B, lo, hi);
      int cnt = 0, best_c = -1;
      double best = 0.0;
      for (int j = lo; j < hi; ++j) {
        double ji;
        if (!is_edge(xi, yi, A.sx[c0 + j], A.sy[c0 + j], A.B, A.two_b2, A.t, &ji)) continue;
        const int c = (int)(c0 + A.sidx[c0 + j]);   // (the tie rule is on batch indices)
        ++cnt;
        if (best_c < 0 || ji > best || (ji == best && c < best_c)) { best = ji; best_c = c; }
      }
      ne[q] += cnt;
      if (cnt > 0) { ++nsup[q]; mask |= 1u << q; }
      A.partner[b * k + q] = best_c;
      if (A.partner_ji) A.partner_ji[b * k + q] = best;
    }
    A.support[b] = (uint8_t)mask;
  }
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < MAX_K; ++q) {
    int64_t e = ne[q], u = nsup[q];
    for (int o = 32; o > 0; o >>= 1) {
      e += __shfl_xor(e, o, 64);
      u += __shfl_xor(u, o, 64);
    }
    if (lane == 0) { red[w][q] = e; red[w][MAX_K + q] = u; }
  }
  __syncthreads();
  if (tid < 2 * MAX_K) {
    const int q = tid & (MAX_K - 1);
    int64_t r = 0;
    for (int i = 0; i < AGREE_WG / 64; ++i) r += red[i][tid];
    if (q < k) (tid < MAX_K ? A.pair_edges : A.pair_supported)[(int64_t)s * k + q] = r;
  }
}

__global__ __launch_bounds__(AGREE_WG) void k_agree_mutual(AgreeArgs A) {
  __shared__ int64_t red[AGREE_WG / 64][MAX_K];
  const int tid = threadIdx.x, k = A.k;
  const int s = A.seg[blockIdx.x];
  const int m = s / k, p = s - m * k;
  const int64_t b0 = A.off[s];
  const int n = (int)(A.off[s + 1] - b0);
  int cnt[MAX_K];
#pragma unroll
  for (int q = 0; q < MAX_K; ++q) cnt[q] = 0;
  for (int i = tid; i < n; i += AGREE_WG) {
    const int64_t b = b0 + i;
#pragma unroll
    for (int q = 0; q < MAX_K; ++q) {
      if (q >= k || q == p) continue;
      const int64_t c = A.partner[b * k + q];
      // (a partner is a batch index or -1; nothing outside the arrays is ever read)
      if (c >= 0 && c < A.n_box && A.partner[c * k + p] == b) ++cnt[q];
    }
  }
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int q = 0; q < MAX_K; ++q) {
    int64_t v = cnt[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[w][q] = v;
  }
  __syncthreads();
  if (tid < k) {
    int64_t r = 0;
    for (int i = 0; i < AGREE_WG / 64; ++i) r += red[i][tid];
    A.pair_mutual[(int64_t)s * k + tid] = r;
  }
}

void launch_agree_partner(hipStream_t stream, int n_launch, const AgreeArgs& A) {
  if (n_launch > 0)
    hipLaunchKernelGGL(k_agree_partner, dim3(n_launch), dim3(AGREE_WG), 0, stream, A);
}

void launch_agree_mutual(hipStream_t stream, int n_launch, const AgreeArgs& A) {
  if (n_launch > 0)
    hipLaunchKernelGGL(k_agree_mutual, dim3(n_launch), dim3(AGREE_WG), 0, stream, A);
}

}  // namespace rgc
