// rgc_match.hip — particle-level scoring: a maximum-cardinality one-to-one matching between
// the ground-truth boxes and the picks of every pair (rgc_score_match).
//
// Two boxes are joined iff their exact intersection over union exceeds the threshold
// (iou_edge, rgc_device.h).  One workgroup per pair, many pairs per launch; all per-pair state
// lives in HBM scratch indexed like the boxes (L2 resident at data-set sizes), so no pair size
// is compiled in: every step is a loop over the pair's boxes in chunks of MT_WG.
//
//   k_score_match_count   edges of every pick and of the pair (the host sizes the CSR from it)
//   k_score_match         scan of the degrees, CSR fill, greedy maximal matching by rounds,
//                         then phases of multi-source alternating BFS from all free picks
//
// The host sorts each pair's ground truth by x0, so a pick tests only the window of boxes whose
// x-range can overlap it: x0 in (pick.x0 - widest ground-truth box, pick.x1).
//
// Every contested claim is an atomicMin followed by a workgroup barrier, and the winner is read
// after it: the lowest index wins, never the first to arrive, so the matching returned is a
// function of the inputs.  Every loop on device state has a bound; a pair that reaches one sets
// its status and the host reports it.
#include <climits>

#include "rgc_device.h"
#include "rgc_kernels.h"

namespace rgc {

constexpr int MT_WG = 256;

// the window [lo, hi) of the pair's ground truth (ascending x0) that can overlap pick b in x
__device__ __forceinline__ void match_window(const int4* G, int ng, int wmax, int4 b, int& lo,
                                             int& hi) {
  const int xlo = b.x - wmax;   // a box with x0 <= xlo ends at or before b.x (no overflow: host limits)
  int l = 0, h = ng;
  while (l < h) {               // first x0 > xlo
    const int m = (l + h) >> 1;
    if (G[m].x > xlo) h = m; else l = m + 1;
  }
  lo = l;
  h = ng;
  while (l < h) {               // first x0 >= b.x1
    const int m = (l + h) >> 1;
    if (G[m].x >= b.y) h = m; else l = m + 1;
  }
  hi = l;
}

// a word other lanes claim with atomicMin, read after the barrier that ends the claims
__device__ __forceinline__ int claim_load(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(MT_WG) void k_score_match_count(MatchArgs A) {
  __shared__ int64_t red[MT_WG / 64];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = A.base[p];
  const int ng = A.n_gt[p];
  const int npk = (int)(A.base[p + 1] - b0) - ng;
  const int wmax = A.gt_wmax[p];
  const int4* G = A.boxes + b0;
  const int4* P = G + ng;
  int32_t* deg = A.deg + b0 + ng;
  int64_t mine = 0;
  for (int u = tid; u < npk; u += MT_WG) {
    const int4 b = P[u];
    int d = 0;
    if (b.x < b.y && b.z < b.w) {
      int lo, hi;
      match_window(G, ng, wmax, b, lo, hi);
      for (int g = lo; g < hi; ++g) {
        const int4 a = G[g];
        d += iou_edge(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, A.t) ? 1 : 0;
      }
    }
    deg[u] = d;
    mine += d;
  }
  const int64_t tot = block_sum64<MT_WG>(mine, red);
  if (tid == 0) A.etot[p] = tot;
}

__global__ __launch_bounds__(MT_WG) void k_score_match(MatchArgs A) {
  __shared__ int s_scan[MT_WG / 64];
  __shared__ int64_t red[MT_WG / 64];
  __shared__ int s_any, s_found, s_next, s_bad;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = A.base[p];
  const int ng = A.n_gt[p];
  const int npk = (int)(A.base[p + 1] - b0) - ng;
  if (ng == 0 || npk == 0) {           // (the whole workgroup: no barrier is skipped)
    for (int u = tid; u < npk; u += MT_WG) A.mate[b0 + ng + u] = -1;
    if (tid == 0) { A.tp[p] = 0; A.status[p] = 0; }
    return;
  }
  const int wmax = A.gt_wmax[p];
  const int4* G = A.boxes + b0;
  const int4* P = G + ng;
  // per-box state: the ground truth's part and the picks' part of each array
  int32_t* mate_g = A.mate + b0;  int32_t* mate_p = mate_g + ng;
  int32_t* par_g = A.par + b0;    int32_t* root_p = par_g + ng;
  int32_t* lvl_g = A.lvl + b0;    int32_t* lvl_p = lvl_g + ng;
  int32_t* found_p = A.found + b0 + ng;
  const int32_t* deg = A.deg + b0 + ng;
  int32_t* rowp = A.rowp + b0 + ng;
  int32_t* adj = A.adj + A.ebase[p];
  const int64_t nmin = ng < npk ? ng : npk;
  const int64_t phase_cap = nmin + 1, level_cap = 2 * nmin + 2;

  // ---- CSR: exclusive scan of the degrees (the pair's edges fit 31 bits: the host checked),
  // then each pick writes its ground-truth boxes in ascending index
  if (tid == 0) s_bad = 0;
  int carry = 0;
  for (int c0 = 0; c0 < npk; c0 += MT_WG) {
    const int u = c0 + tid;
    const int d = u < npk ? deg[u] : 0;
    int tot;
    const int ex = block_excl_scan_add32<MT_WG>(d, s_scan, &tot);
    if (u < npk) rowp[u] = carry + ex;
    carry += tot;
    __syncthreads();
  }
  for (int u = tid; u < npk; u += MT_WG) {
    const int4 b = P[u];
    mate_p[u] = -1;
    if (deg[u] == 0) continue;
    int lo, hi;
    match_window(G, ng, wmax, b, lo, hi);
    int e = rowp[u];
    for (int g = lo; g < hi; ++g) {
      const int4 a = G[g];
      if (iou_edge(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, A.t)) adj[e++] = g;
    }
  }
  for (int g = tid; g < ng; g += MT_WG) {
    mate_g[g] = -1;
    par_g[g] = INT_MAX;
  }
  __syncthreads();

  // ---- greedy maximal matching by rounds: every free pick proposes to its lowest free
  // ground-truth box, the lowest proposer of a box wins it.  Every box proposed to is won, so
  // the claim words of the free boxes are still INT_MAX in the next round; a round that makes a
  // proposal makes a match, so the rounds end within phase_cap.
  for (int64_t round = 0; round < phase_cap; ++round) {
    if (tid == 0) s_any = 0;
    __syncthreads();
    for (int u = tid; u < npk; u += MT_WG) {
      int want = -1;
      if (mate_p[u] < 0) {
        const int e1 = rowp[u] + deg[u];
        for (int e = rowp[u]; e < e1; ++e) {
          const int g = adj[e];
          if (mate_g[g] < 0) { want = g; break; }
        }
      }
      found_p[u] = want;
      if (want >= 0) {
        atomicMin(&par_g[want], u);
        s_any = 1;
      }
    }
    __syncthreads();
    if (!s_any) break;   // (uniform; s_any is next written after the barrier below)
    for (int u = tid; u < npk; u += MT_WG) {
      const int want = found_p[u];
      if (want >= 0 && claim_load(&par_g[want]) == u) {
        mate_p[u] = want;
        mate_g[want] = u;
      }
    }
    __syncthreads();
  }
  __syncthreads();

  // ---- phases: alternating BFS from all free picks at once.  A ground-truth box is claimed
  // once per phase (by the lowest pick of the level that reaches it), so the trees are vertex
  // disjoint; the BFS stops at the first level that reaches a free box, and every tree that
  // reached one augments along the path to the lowest of them.  A phase that reaches no free
  // box ends the loop: no augmenting path is left, the matching is maximum (Berge).
  bool done = false;
  for (int64_t phase = 0; phase < phase_cap && !done; ++phase) {
    for (int g = tid; g < ng; g += MT_WG) {
      par_g[g] = INT_MAX;
      lvl_g[g] = -1;
    }
    for (int u = tid; u < npk; u += MT_WG) {
      const bool free_u = mate_p[u] < 0;
      root_p[u] = free_u ? u : -1;
      lvl_p[u] = free_u ? 0 : -1;
      found_p[u] = INT_MAX;
    }
    if (tid == 0) s_found = 0;
    __syncthreads();
    bool reached = false, open = true;
    for (int64_t lev = 0; lev < level_cap; ++lev) {
      if (tid == 0) s_next = 0;
      // the picks of this level claim every box not yet reached (a matched pick's own box was
      // reached before it)
      for (int u = tid; u < npk; u += MT_WG) {
        if (lvl_p[u] != (int)lev) continue;
        const int e1 = rowp[u] + deg[u];
        for (int e = rowp[u]; e < e1; ++e) {
          const int g = adj[e];
          if (lvl_g[g] < 0) atomicMin(&par_g[g], u);
        }
      }
      __syncthreads();
      // the boxes claimed at this level: a free one is offered to its tree's root (lowest
      // wins), a matched one puts its pick into the next level
      for (int g = tid; g < ng; g += MT_WG) {
        if (lvl_g[g] >= 0) continue;
        const int u = claim_load(&par_g[g]);
        if (u == INT_MAX) continue;
        lvl_g[g] = (int)lev;
        const int r = root_p[u];   // (a pick of this level: it has a root)
        if ((unsigned)r >= (unsigned)npk) { s_bad = MATCH_ST_WALK; continue; }
        const int v = mate_g[g];
        if (v < 0) {
          atomicMin(&found_p[r], g);
          s_found = 1;
        } else {
          root_p[v] = r;
          lvl_p[v] = (int)lev + 1;
          s_next = 1;
        }
      }
      __syncthreads();
      reached = s_found != 0;
      open = s_next != 0;
      __syncthreads();
      if (reached || !open) break;
    }
    if (!reached) {
      if (open && tid == 0) s_bad = MATCH_ST_LEVELS;   // ran into level_cap
      done = true;
      break;
    }
    // one thread per tree walks its path back from the box to the root
    for (int r = tid; r < npk; r += MT_WG) {
      if (mate_p[r] >= 0) continue;
      int g = claim_load(&found_p[r]);
      if (g == INT_MAX) continue;
      bool home = false;   // (indices are checked before use: a broken tree ends the walk)
      for (int64_t step = 0; step < level_cap && (unsigned)g < (unsigned)ng; ++step) {
        const int u = par_g[g];
        if ((unsigned)u >= (unsigned)npk) break;
        const int prev = mate_p[u];
        mate_p[u] = g;
        mate_g[g] = u;
        home = u == r;
        if (home) break;
        g = prev;
      }
      if (!home) s_bad = MATCH_ST_WALK;
    }
    __syncthreads();
  }
  if (!done && tid == 0 && !s_bad) s_bad = MATCH_ST_PHASES;
  __syncthreads();

  int64_t mine = 0;
  for (int u = tid; u < npk; u += MT_WG) mine += mate_p[u] >= 0 ? 1 : 0;
  const int64_t tp = block_sum64<MT_WG>(mine, red);
  if (tid == 0) {
    A.tp[p] = tp;
    A.status[p] = s_bad;
  }
}

void launch_match_count(hipStream_t stream, int n_pairs, const MatchArgs& A) {
  if (n_pairs > 0)
    hipLaunchKernelGGL(k_score_match_count, dim3(n_pairs), dim3(MT_WG), 0, stream, A);
}

void launch_match(hipStream_t stream, int n_pairs, const MatchArgs& A) {
  if (n_pairs > 0) hipLaunchKernelGGL(k_score_match, dim3(n_pairs), dim3(MT_WG), 0, stream, A);
}

}  // namespace rgc

extern "C" int rgc_test_iou_edge(const int32_t a[4], const int32_t b[4], double t) {
  return rgc::iou_edge(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], t) ? 1 : 0;
}
