// rgc_match.hip — particle-level scoring: a maximum-cardinality one-to-one matching between
// the ground-truth boxes and the picks of every pair (rgc_score_match, rgc_score_match_sweep).
//
// Two boxes are joined iff their exact intersection over union exceeds the threshold
// (iou_edge, rgc_device.h).  One workgroup per pair, many pairs per launch; all per-pair state
// lives in HBM scratch indexed like the boxes (L2 resident at data-set sizes), so no pair size
// is compiled in: every step is a loop over the pair's boxes in chunks of MT_WG.
//
//   k_score_match_count   edges of every pick and of the pair (the host sizes the CSR from it)
//   k_score_match         scan of the degrees, CSR fill, greedy maximal matching by rounds,
//                         then phases of multi-source alternating BFS from all free picks
//   k_score_match_sweep   the same CSR once, then the matching at every confidence threshold of
//                         a sweep: each step augments the step before from its new picks only
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

// One pair's part of the launch's arrays (the ground truth's part and the picks' part of each
// per-box array) and the workgroup's flags in LDS.
struct MatchPair {
  int ng, npk;
  const int4 *G, *P;
  int32_t *mate_g, *mate_p;
  int32_t *par_g, *root_p;
  int32_t *lvl_g, *lvl_p;
  int32_t* found_p;
  const int32_t* deg;
  int32_t *rowp, *adj;
  int *s_any, *s_found, *s_next, *s_bad;
};

__device__ __forceinline__ MatchPair match_pair(const MatchArgs& A, int p, int* s_any, int* s_found,
                                                int* s_next, int* s_bad) {
  MatchPair M;
  const int64_t b0 = A.base[p];
  M.ng = A.n_gt[p];
  M.npk = (int)(A.base[p + 1] - b0) - M.ng;
  M.G = A.boxes + b0;
  M.P = M.G + M.ng;
  M.mate_g = A.mate + b0;  M.mate_p = M.mate_g + M.ng;
  M.par_g = A.par + b0;    M.root_p = M.par_g + M.ng;
  M.lvl_g = A.lvl + b0;    M.lvl_p = M.lvl_g + M.ng;
  M.found_p = A.found + b0 + M.ng;
  M.deg = A.deg + b0 + M.ng;
  M.rowp = A.rowp + b0 + M.ng;
  M.adj = A.adj + A.ebase[p];
  M.s_any = s_any;  M.s_found = s_found;  M.s_next = s_next;  M.s_bad = s_bad;
  return M;
}

// ---- CSR of all the pair's picks: exclusive scan of the degrees (the pair's edges fit 31 bits:
// the host checked), then each pick writes its ground-truth boxes in ascending index.  Leaves
// every box unmatched and every claim word free; ends with a barrier.
__device__ __forceinline__ void match_csr(const MatchPair& M, int wmax, double t, int* s_scan) {
  const int tid = threadIdx.x, ng = M.ng, npk = M.npk;
  if (tid == 0) *M.s_bad = 0;
  int carry = 0;
  for (int c0 = 0; c0 < npk; c0 += MT_WG) {
    const int u = c0 + tid;
    const int d = u < npk ? M.deg[u] : 0;
    int tot;
    const int ex = block_excl_scan_add32<MT_WG>(d, s_scan, &tot);
    if (u < npk) M.rowp[u] = carry + ex;
    carry += tot;
    __syncthreads();
  }
  for (int u = tid; u < npk; u += MT_WG) {
    const int4 b = M.P[u];
    M.mate_p[u] = -1;
    if (M.deg[u] == 0) continue;
    int lo, hi;
    match_window(M.G, ng, wmax, b, lo, hi);
    int e = M.rowp[u];
    for (int g = lo; g < hi; ++g) {
      const int4 a = M.G[g];
      if (iou_edge(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, t)) M.adj[e++] = g;
    }
  }
  for (int g = tid; g < ng; g += MT_WG) {
    M.mate_g[g] = -1;
    M.par_g[g] = INT_MAX;
  }
  __syncthreads();
}

// ---- greedy maximal matching by rounds: every free pick of [r0, r1) proposes to its lowest
// free ground-truth box, the lowest proposer of a box wins it.  The claim words of the free
// boxes are INT_MAX on entry.  Every box proposed to is won, so they still are in the next
// round; a round that makes a proposal makes a match, so the rounds end within `cap`
// (min(free boxes, r1 - r0) + 1 or more).  Ends with a barrier.
__device__ __forceinline__ void match_greedy(const MatchPair& M, int r0, int r1, int64_t cap) {
  const int tid = threadIdx.x;
  for (int64_t round = 0; round < cap; ++round) {
    if (tid == 0) *M.s_any = 0;
    __syncthreads();
    for (int u = r0 + tid; u < r1; u += MT_WG) {
      int want = -1;
      if (M.mate_p[u] < 0) {
        const int e1 = M.rowp[u] + M.deg[u];
        for (int e = M.rowp[u]; e < e1; ++e) {
          const int g = M.adj[e];
          if (M.mate_g[g] < 0) { want = g; break; }
        }
      }
      M.found_p[u] = want;
      if (want >= 0) {
        atomicMin(&M.par_g[want], u);
        *M.s_any = 1;
      }
    }
    __syncthreads();
    if (!*M.s_any) break;   // (uniform; s_any is next written after the barrier below)
    for (int u = r0 + tid; u < r1; u += MT_WG) {
      const int want = M.found_p[u];
      if (want >= 0 && claim_load(&M.par_g[want]) == u) {
        M.mate_p[u] = want;
        M.mate_g[want] = u;
      }
    }
    __syncthreads();
  }
  __syncthreads();
}

// ---- phases: alternating BFS from all free picks of [r0, r1) at once, in the graph of the
// picks [0, nact).  A ground-truth box is claimed once per phase (by the lowest pick of the
// level that reaches it), so the trees are vertex disjoint; the BFS stops at the first level
// that reaches a free box, and every tree that reached one augments along the path to the
// lowest of them.  A phase that reaches no free box ends the loop: no augmenting path from a
// root is left.  With roots = all free picks that makes the matching maximum (Berge).  A pick
// other than a root enters a level only as the mate of a box, so the free picks outside
// [r0, r1) and the picks from nact on take no part.  -> false: phase_cap ran out.
__device__ __forceinline__ bool match_phases(const MatchPair& M, int r0, int r1, int nact,
                                             int64_t phase_cap, int64_t level_cap) {
  const int tid = threadIdx.x, ng = M.ng;
  bool done = false;
  for (int64_t phase = 0; phase < phase_cap && !done; ++phase) {
    for (int g = tid; g < ng; g += MT_WG) {
      M.par_g[g] = INT_MAX;
      M.lvl_g[g] = -1;
    }
    for (int u = tid; u < nact; u += MT_WG) {
      const bool free_u = M.mate_p[u] < 0 && u >= r0 && u < r1;
      M.root_p[u] = free_u ? u : -1;
      M.lvl_p[u] = free_u ? 0 : -1;
      M.found_p[u] = INT_MAX;
    }
    if (tid == 0) *M.s_found = 0;
    __syncthreads();
    bool reached = false, open = true;
    for (int64_t lev = 0; lev < level_cap; ++lev) {
      if (tid == 0) *M.s_next = 0;
      // the picks of this level claim every box not yet reached (a matched pick's own box was
      // reached before it)
      for (int u = tid; u < nact; u += MT_WG) {
        if (M.lvl_p[u] != (int)lev) continue;
        const int e1 = M.rowp[u] + M.deg[u];
        for (int e = M.rowp[u]; e < e1; ++e) {
          const int g = M.adj[e];
          if (M.lvl_g[g] < 0) atomicMin(&M.par_g[g], u);
        }
      }
      __syncthreads();
      // the boxes claimed at this level: a free one is offered to its tree's root (lowest
      // wins), a matched one puts its pick into the next level
      for (int g = tid; g < ng; g += MT_WG) {
        if (M.lvl_g[g] >= 0) continue;
        const int u = claim_load(&M.par_g[g]);
        if (u == INT_MAX) continue;
        M.lvl_g[g] = (int)lev;
        const int r = M.root_p[u];   // (a pick of this level: it has a root)
        if ((unsigned)r >= (unsigned)nact) { *M.s_bad = MATCH_ST_WALK; continue; }
        const int v = M.mate_g[g];
        if (v < 0) {
          atomicMin(&M.found_p[r], g);
          *M.s_found = 1;
        } else if ((unsigned)v < (unsigned)nact) {
          M.root_p[v] = r;
          M.lvl_p[v] = (int)lev + 1;
          *M.s_next = 1;
        } else {
          *M.s_bad = MATCH_ST_WALK;   // (a mate is a pick of the graph)
        }
      }
      __syncthreads();
      reached = *M.s_found != 0;
      open = *M.s_next != 0;
      __syncthreads();
      if (reached || !open) break;
    }
    if (!reached) {
      if (open && tid == 0) *M.s_bad = MATCH_ST_LEVELS;   // ran into level_cap
      done = true;
      break;
    }
    // one thread per tree walks its path back from the box to the root
    for (int r = r0 + tid; r < r1; r += MT_WG) {
      if (M.mate_p[r] >= 0) continue;
      int g = claim_load(&M.found_p[r]);
      if (g == INT_MAX) continue;
      bool home = false;   // (indices are checked before use: a broken tree ends the walk)
      for (int64_t step = 0; step < level_cap && (unsigned)g < (unsigned)ng; ++step) {
        const int u = M.par_g[g];
        if ((unsigned)u >= (unsigned)nact) break;
        const int prev = M.mate_p[u];
        M.mate_p[u] = g;
        M.mate_g[g] = u;
        home = u == r;
        if (home) break;
        g = prev;
      }
      if (!home) *M.s_bad = MATCH_ST_WALK;
    }
    __syncthreads();
  }
  return done;
}

// the matched picks of [0, n) (every thread gets the sum)
__device__ __forceinline__ int64_t match_size(const MatchPair& M, int n, int64_t* red) {
  int64_t mine = 0;
  for (int u = threadIdx.x; u < n; u += MT_WG) mine += M.mate_p[u] >= 0 ? 1 : 0;
  return block_sum64<MT_WG>(mine, red);
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
  const MatchPair M = match_pair(A, p, &s_any, &s_found, &s_next, &s_bad);
  const int64_t nmin = ng < npk ? ng : npk;
  const int64_t phase_cap = nmin + 1, level_cap = 2 * nmin + 2;
  match_csr(M, A.gt_wmax[p], A.t, s_scan);
  match_greedy(M, 0, npk, phase_cap);
  const bool done = match_phases(M, 0, npk, npk, phase_cap, level_cap);
  if (!done && tid == 0 && !s_bad) s_bad = MATCH_ST_PHASES;
  __syncthreads();
  const int64_t tp = match_size(M, npk, red);
  if (tid == 0) {
    A.tp[p] = tp;
    A.status[p] = s_bad;
  }
}

// The matching at every threshold of a sweep.  The pair's picks are ordered so that the nact =
// keep[p * T + j] picks kept at threshold j are a prefix, nact non-increasing in j.  The CSR
// holds all picks; the steps go from the strictest threshold (j = T - 1) to the loosest, and
// each keeps the matching of the step before it, which is a matching of its own larger graph,
// and augments it from the picks that are new, [nprev, nact), alone.  That is enough: the
// matched picks are an independent set of the graph's transversal matroid, an augmentation
// keeps every matched pick matched, and a free pick from which no augmenting path existed was
// in the span of the matched set, where it stays as the set grows.  tp_out[p * T + j] = the
// size of the matching after step j.
__global__ __launch_bounds__(MT_WG) void k_score_match_sweep(MatchArgs A, int T,
                                                             const int64_t* keep,
                                                             int64_t* tp_out) {
  __shared__ int s_scan[MT_WG / 64];
  __shared__ int64_t red[MT_WG / 64];
  __shared__ int s_any, s_found, s_next, s_bad;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t b0 = A.base[p];
  const int ng = A.n_gt[p];
  const int npk = (int)(A.base[p + 1] - b0) - ng;
  const int64_t* kp = keep + (int64_t)p * T;
  int64_t* out = tp_out + (int64_t)p * T;
  if (ng == 0 || npk == 0) {           // (the whole workgroup: no barrier is skipped)
    for (int j = tid; j < T; j += MT_WG) out[j] = 0;
    if (tid == 0) A.status[p] = 0;
    return;
  }
  const MatchPair M = match_pair(A, p, &s_any, &s_found, &s_next, &s_bad);
  match_csr(M, A.gt_wmax[p], A.t, s_scan);
  int nprev = 0;
  int64_t tp = 0;
  for (int j = T - 1; j >= 0; --j) {
    // (every thread reads the same word: the branch below is uniform.  The host checked
    // 0 <= keep <= npk, non-increasing in j; the clamp keeps a bad table inside the pair)
    const int64_t k = kp[j];
    const int nact = k < nprev ? nprev : k > npk ? npk : (int)k;
    if (nact > nprev) {
      for (int g = tid; g < ng; g += MT_WG) M.par_g[g] = INT_MAX;   // greedy's claim words
      __syncthreads();
      const int64_t fresh = nact - nprev, nmin = ng < nact ? ng : nact;
      match_greedy(M, nprev, nact, fresh + 1);
      const bool done = match_phases(M, nprev, nact, nact, fresh + 1, 2 * nmin + 2);
      if (!done && tid == 0 && !s_bad) s_bad = MATCH_ST_PHASES;
      __syncthreads();
      tp = match_size(M, nact, red);
      nprev = nact;
    }
    if (tid == 0) out[j] = tp;
  }
  __syncthreads();
  if (tid == 0) A.status[p] = s_bad;
}

void launch_match_count(hipStream_t stream, int n_pairs, const MatchArgs& A) {
  if (n_pairs > 0)
    hipLaunchKernelGGL(k_score_match_count, dim3(n_pairs), dim3(MT_WG), 0, stream, A);
}

void launch_match(hipStream_t stream, int n_pairs, const MatchArgs& A) {
  if (n_pairs > 0) hipLaunchKernelGGL(k_score_match, dim3(n_pairs), dim3(MT_WG), 0, stream, A);
}

void launch_match_sweep(hipStream_t stream, int n_pairs, const MatchArgs& A, int n_thr,
                        const int64_t* keep, int64_t* tp_out) {
  if (n_pairs > 0)
    hipLaunchKernelGGL(k_score_match_sweep, dim3(n_pairs), dim3(MT_WG), 0, stream, A, n_thr, keep,
                       tp_out);
}

}  // namespace rgc

extern "C" int rgc_test_iou_edge(const int32_t a[4], const int32_t b[4], double t) {
  return rgc::iou_edge(a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3], t) ? 1 : 0;
}
