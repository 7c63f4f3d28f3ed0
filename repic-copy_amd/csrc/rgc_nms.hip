// rgc_nms.hip — greedy non-maximum suppression of square boxes (rgc_nms).
//
// A segment is a list of boxes of side B in priority order (index 0 first).  Two boxes conflict
// iff the reference quotient exceeds the threshold: jaccard() of rgc_device.h, the f64 operation
// order of get_cliques.py:40-46, strict `> t`.  keep[i] = 1 iff no j < i of the segment is kept
// and conflicts with i: the greedy result, and the only set with that property.  One workgroup
// per segment, many segments per launch; all per-box state lives in HBM scratch indexed like
// the boxes (L2 resident at data-set sizes), so no segment size is compiled in.
//
//   k_nms_count   per box its conflicting neighbours of higher priority, and the segment's total
//                 (the host sizes the CSR from it)
//   k_nms         scan of the counts, CSR fill, then rounds: an undecided box becomes suppressed
//                 when a listed neighbour is kept, kept when all of them are suppressed
//
// The host hands over each segment's finite boxes sorted by x, so a box tests only the window of
// boxes whose x can overlap its own; a box with a non-finite coordinate is in no window and has
// no neighbours (the reference formula gives 0 or NaN there, never > t).
//
// The rounds need no claim protocol: a box is decided only from final neighbour states, final
// states are the greedy answer by induction on priority, and a state word changes once
// (0 -> kept or 0 -> suppressed), so a stale read only leaves a box undecided for another round.
// Every round decides at least the lowest undecided box (all its neighbours have lower
// indices), so n + 1 rounds suffice; a chain along the priority order needs n.  A segment that
// runs out of rounds sets its status and the host reports it.  No workgroup waits for another.
#include "rgc_device.h"
#include "rgc_kernels.h"
#include "rgc_window.h"   // nms_window: the x-window of a sorted segment

namespace rgc {

constexpr int NMS_WG = 256;
constexpr int NMS_UNDECIDED = 0, NMS_KEPT = 1, NMS_SUPPRESSED = 2;

// one segment's part of the launch's arrays
struct NmsSeg {
  int n, ns;
  const double *x, *y, *sx, *sy;
  const int32_t* sidx;
  int32_t *cnt, *rowp, *state;
};

__device__ __forceinline__ NmsSeg nms_seg(const NmsArgs& A, int p) {
  NmsSeg S;
  const int64_t b0 = A.off[p];
  S.n = (int)(A.off[p + 1] - b0);
  S.ns = A.ns[p];
  S.x = A.x + b0;    S.y = A.y + b0;
  S.sx = A.sx + b0;  S.sy = A.sy + b0;  S.sidx = A.sidx + b0;
  S.cnt = A.cnt + b0;  S.rowp = A.rowp + b0;  S.state = A.state + b0;
  return S;
}

// Box i's conflicting neighbours of higher priority, in ascending sorted position: counted, and
// written to out[0 .. cap) when out is given (never past cap).
__device__ __forceinline__ int nms_neighbours(const NmsSeg& S, const NmsArgs& A, int i,
                                              int32_t* out, int cap) {
  const double xi = S.x[i], yi = S.y[i];
  if (!(isfinite(xi) && isfinite(yi))) return 0;
  int lo, hi, d = 0;
  nms_window(S.sx, S.ns, xi, A.B, lo, hi);
  for (int s = lo; s < hi; ++s) {
    const int j = S.sidx[s];
    if (j >= i) continue;
    if (jaccard(S.sx[s], S.sy[s], xi, yi, A.B, A.two_b2) > A.t) {
      if (out && d < cap) out[d] = j;
      ++d;
    }
  }
  return d;
}

// a state word other lanes finalise in the same round
__device__ __forceinline__ int state_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void state_store(int32_t* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NMS_WG) void k_nms_count(NmsArgs A) {
  __shared__ int64_t red[NMS_WG / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const NmsSeg S = nms_seg(A, p);
  int64_t mine = 0;
  for (int i = tid; i < S.n; i += NMS_WG) {
    const int d = nms_neighbours(S, A, i, nullptr, 0);
    S.cnt[i] = d;
    mine += d;
  }
  const int64_t tot = block_sum64<NMS_WG>(mine, red);
  if (tid == 0) A.etot[p] = tot;
}

__global__ __launch_bounds__(NMS_WG) void k_nms(NmsArgs A) {
  __shared__ int s_scan[NMS_WG / 64];
  __shared__ int64_t red[NMS_WG / 64];
  __shared__ int s_any, s_bad;
  const int p = blockIdx.x, tid = threadIdx.x;
  const NmsSeg S = nms_seg(A, p);
  const int n = S.n;
  if (tid == 0) s_bad = 0;
  int32_t* adj = A.adj + A.ebase[p];
  // exclusive scan of the counts (the segment's edges fit 31 bits: the host checked)
  int carry = 0;
  for (int c0 = 0; c0 < n; c0 += NMS_WG) {
    const int i = c0 + tid;
    const int d = i < n ? S.cnt[i] : 0;
    int tot;
    const int ex = block_excl_scan_add32<NMS_WG>(d, s_scan, &tot);
    if (i < n) S.rowp[i] = carry + ex;
    carry += tot;
    __syncthreads();
  }
  // CSR fill: the count pass's test again, so each box writes exactly its count
  for (int i = tid; i < n; i += NMS_WG) {
    state_store(&S.state[i], NMS_UNDECIDED);
    const int d = S.cnt[i];
    if (d > 0) nms_neighbours(S, A, i, adj + S.rowp[i], d);
  }
  __syncthreads();
  // rounds, at most n + 1
  const int64_t cap = (int64_t)n + 1;
  bool open = true;
  for (int64_t round = 0; round < cap && open; ++round) {
    if (tid == 0) s_any = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NMS_WG) {
      if (state_load(&S.state[i]) != NMS_UNDECIDED) continue;
      const int e0 = S.rowp[i], e1 = e0 + S.cnt[i];
      bool hit = false, all = true;
      for (int e = e0; e < e1; ++e) {
        const int j = adj[e];
        // (a listed neighbour has a lower index; anything else ends the call with a status)
        if ((unsigned)j >= (unsigned)i) { s_bad = NMS_ST_LIST; continue; }
        const int v = state_load(&S.state[j]);
        if (v == NMS_KEPT) { hit = true; break; }
        all = all && v == NMS_SUPPRESSED;
      }
      if (hit) state_store(&S.state[i], NMS_SUPPRESSED);
      else if (all) state_store(&S.state[i], NMS_KEPT);
      else s_any = 1;
    }
    __syncthreads();
    open = s_any != 0;   // (uniform; s_any is next written after the barrier below)
    __syncthreads();
  }
  int64_t mine = 0;
  for (int i = tid; i < n; i += NMS_WG) {
    const int k = state_load(&S.state[i]) == NMS_KEPT ? 1 : 0;
    A.keep[A.off[p] + i] = (uint8_t)k;
    mine += k;
  }
  const int64_t tot = block_sum64<NMS_WG>(mine, red);
  if (tid == 0) {
    A.kept[p] = tot;
    A.status[p] = s_bad ? s_bad : open ? NMS_ST_ROUNDS : 0;
  }
}

void launch_nms_count(hipStream_t stream, int n_seg, const NmsArgs& A) {
  if (n_seg > 0) hipLaunchKernelGGL(k_nms_count, dim3(n_seg), dim3(NMS_WG), 0, stream, A);
}

void launch_nms(hipStream_t stream, int n_seg, const NmsArgs& A) {
  if (n_seg > 0) hipLaunchKernelGGL(k_nms, dim3(n_seg), dim3(NMS_WG), 0, stream, A);
}

}  // namespace rgc
