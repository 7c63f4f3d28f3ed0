// rgc_pick.hip — the device hand-off between get_cliques and run_ilp (`repic consensus`).
//
//   k_pick_cols    rgc_run's per-clique outputs -> the set-packing solver's CSC inputs, in HBM:
//                  column c of micrograph m (columns packed micrograph by micrograph, whatever
//                  order the clique ranges were reserved in) gets row_idx = rows + row_base[m],
//                  w widened to f64, col_ptr = c k, and col_mg = m.
//   k_pick_select  per micrograph: the columns with x == 1, compacted in ascending order.
//   k_pick_scan    pick_off = exclusive sum of min(selected, num_particles).
//   k_pick_emit    per micrograph: rank of every selected column by (confidence descending,
//                  column ascending) - the order of run_ilp.py:121-122's stable reverse sort,
//                  compared as floats so +0.0 == -0.0 - and the picks of rank < num_particles:
//                  np.rint of the consensus coordinates, the confidence, the column.
// and, only for `consensus --members`:
//   k_pick_clique_mark  every member box of every column is "in some clique".
//   k_pick_members      per written pick: np.rint of its k members' coordinates, picker order,
//                       and the members' "in a written pick" marks.
//   k_pick_left         per (micrograph, picker): the boxes in no written pick, in file order.
// gfx950, wave64.  One 256-thread workgroup per micrograph in the per-micrograph kernels.
#include <hip/hip_runtime.h>

#include "rgc_device.h"
#include "rgc_kernels.h"

namespace rgc {

namespace {

constexpr int PK_NT = 256;        // threads per workgroup
constexpr int PK_WAVES = PK_NT / 64;
constexpr int PK_TILE = 1024;     // confidences per LDS tile of the counting rank

__global__ __launch_bounds__(PK_NT) void k_pick_cols(PickArgs A) {
  const int64_t c = (int64_t)blockIdx.x * PK_NT + threadIdx.x;
  if (c == 0) A.col_ptr[A.n_cols] = A.n_cols * A.k;
  if (c >= A.n_cols) return;
  const int m = range_of(A.col_off, A.n_mg, c);   // (empty micrographs skipped)
  const int64_t src = A.src_base[m] + (c - A.col_off[m]);
  const int32_t rb = (int32_t)A.row_base[m];
  for (int j = 0; j < A.k; ++j) A.row_idx[c * A.k + j] = A.rows[src * A.k + j] + rb;
  A.w64[c] = (double)A.w[src];
  A.col_ptr[c] = c * A.k;
  A.col_mg[c] = m;
}

// Ordered compaction of a micrograph's selected columns into sel[col_off[m] ..], their count
// and the packing value sum of w over them (fixed summation order: per-thread strided partial
// sums, then a tree over the workgroup).
__global__ __launch_bounds__(PK_NT) void k_pick_select(PickArgs A) {
  __shared__ int s_wave[PK_WAVES];
  __shared__ double s_sum[PK_NT];
  const int m = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t c0 = A.col_off[m], n = A.col_off[m + 1] - c0;
  const int64_t src0 = A.src_base ? A.src_base[m] : c0;
  int64_t base = 0;
  double part = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += PK_NT) {
    const int64_t i = i0 + t;
    const bool on = i < n && A.x[c0 + i] == 1;
    const unsigned long long b = __ballot(on);
    const int before = __popcll(b & ((1ULL << lane) - 1));
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int v = 0; v < PK_WAVES; ++v) {
      if (v < wave) woff += s_wave[v];
      tot += s_wave[v];
    }
    if (on) {
      A.sel[c0 + base + woff + before] = (int32_t)i;
      if (A.w) part += (double)A.w[src0 + i];
    }
    base += tot;
    __syncthreads();
  }
  s_sum[t] = part;
  __syncthreads();
  for (int h = PK_NT / 2; h > 0; h >>= 1) {
    if (t < h) s_sum[t] += s_sum[t + h];
    __syncthreads();
  }
  if (t == 0) {
    A.sel_cnt[m] = (int32_t)base;
    A.primal[m] = s_sum[0];
  }
}

// pick_off[0 .. n_mg] = exclusive sum of min(sel_cnt, num_particles); one workgroup.
__global__ __launch_bounds__(PK_NT) void k_pick_scan(PickArgs A) {
  __shared__ int64_t s_part[PK_NT];
  const int t = threadIdx.x;
  const int per = (A.n_mg + PK_NT - 1) / PK_NT;
  const int m0 = min(A.n_mg, t * per), m1 = min(A.n_mg, m0 + per);
  auto kept = [&](int m) -> int64_t {
    const int64_t s = A.sel_cnt[m];
    return A.num_particles < 0 ? s : (s < A.num_particles ? s : A.num_particles);
  };
  int64_t sum = 0;
  for (int m = m0; m < m1; ++m) sum += kept(m);
  s_part[t] = sum;
  __syncthreads();
  int64_t off = 0;
  for (int v = 0; v < t; ++v) off += s_part[v];
  for (int m = m0; m < m1; ++m) {
    A.pick_off[m] = off;
    off += kept(m);
  }
  if (t == PK_NT - 1) A.pick_off[A.n_mg] = off;
}

// Counting rank over LDS tiles of the selected columns' confidences: exact about ties, no key
// transform.  rank(i) = #{j : conf_j > conf_i or (conf_j == conf_i and j < i)} (float compares).
__global__ __launch_bounds__(PK_NT) void k_pick_emit(PickArgs A) {
  __shared__ float s_conf[PK_TILE];
  const int m = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t c0 = A.col_off[m];
  const int64_t src0 = A.src_base ? A.src_base[m] : c0;
  const int S = A.sel_cnt[m];
  const int64_t o0 = A.pick_off[m], keep = A.pick_off[m + 1] - o0;
  if (keep == 0) return;   // (uniform per workgroup)
  for (int i0 = 0; i0 < S; i0 += PK_NT) {
    const int i = i0 + t;
    const bool live = i < S;
    const int32_t ci = live ? A.sel[c0 + i] : 0;
    const float fi = live ? A.conf[src0 + ci] : 0.f;
    int rank = 0;
    for (int j0 = 0; j0 < S; j0 += PK_TILE) {
      const int nj = min(PK_TILE, S - j0);
      __syncthreads();
      for (int j = t; j < nj; j += PK_NT) s_conf[j] = A.conf[src0 + A.sel[c0 + j0 + j]];
      __syncthreads();
      if (live) {
        for (int j = 0; j < nj; ++j) {
          const float fj = s_conf[j];
          rank += (fj > fi || (fj == fi && j0 + j < i)) ? 1 : 0;
        }
      }
    }
    if (live && rank < keep) {
      const int64_t s = src0 + ci;
      const int64_t b = A.cons ? (int64_t)A.cons[s] : s;
      A.px[o0 + rank] = rint(A.bx[b]);
      A.py[o0 + rank] = rint(A.by[b]);
      A.pconf[o0 + rank] = fi;
      A.pcol[o0 + rank] = ci;
    }
  }
}

// ---- consensus --members: launched only when members are asked for (PickMemArgs)

// One thread per column: its k member boxes are "in some clique".  Every writer stores the
// same byte value, so concurrent stores to one address need no atomic; the marks of written
// picks live in their own array (k_pick_members).
__global__ __launch_bounds__(PK_NT) void k_pick_clique_mark(PickMemArgs A) {
  const int64_t c = (int64_t)blockIdx.x * PK_NT + threadIdx.x;
  if (c >= A.n_cols) return;
  const int m = range_of(A.col_off, A.n_mg, c);
  const int64_t s = (A.src_base ? A.src_base[m] : A.col_off[m]) + (c - A.col_off[m]);
  for (int p = 0; p < A.k; ++p) {
    const int64_t b = A.members[s * A.k + p];
    const int64_t seg = (int64_t)m * A.k + p;
    if (b >= A.box_off[seg] && b < A.box_off[seg + 1]) A.in_clique[b] = 1;
    else *A.bad = 1;
  }
}

// One thread per written pick (output position i): np.rint of its k members' coordinates, and
// the members' "in a written pick" marks.  A member outside its segment is reported, not read.
__global__ __launch_bounds__(PK_NT) void k_pick_members(PickMemArgs A) {
  const int64_t i = (int64_t)blockIdx.x * PK_NT + threadIdx.x;
  if (i >= A.n_picked) return;
  const int m = range_of(A.pick_off, A.n_mg, i);
  const int64_t s = (A.src_base ? A.src_base[m] : A.col_off[m]) + A.pcol[i];
  for (int p = 0; p < A.k; ++p) {
    const int64_t b = A.members[s * A.k + p];
    const int64_t seg = (int64_t)m * A.k + p;
    const bool in = b >= A.box_off[seg] && b < A.box_off[seg + 1];
    A.pmx[i * A.k + p] = in ? rint(A.bx[b]) : 0.0;
    A.pmy[i * A.k + p] = in ? rint(A.by[b]) : 0.0;
    if (in) A.in_pick[b] = 1;
    else *A.bad = 1;
  }
}

// One workgroup per segment (micrograph, picker): ordered compaction, in file order, of the
// boxes not in a written pick (k_pick_select's ballot / popcount / per-wave offsets), cut at the
// segment's capacity, and the counts of such boxes and of boxes in some column.
__global__ __launch_bounds__(PK_NT) void k_pick_left(PickMemArgs A) {
  __shared__ int s_wave[PK_WAVES], s_cl[PK_WAVES];
  const int64_t seg = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (!A.ok[seg / A.k]) {   // (uniform per workgroup)
    if (t == 0) A.left_cnt[seg] = A.clique_cnt[seg] = 0;
    return;
  }
  const int64_t b0 = A.box_off[seg], n = A.box_off[seg + 1] - b0;
  const int64_t o0 = A.left_off[seg], cap = A.left_off[seg + 1] - o0;
  int64_t base = 0, ncl = 0;
  for (int64_t i0 = 0; i0 < n; i0 += PK_NT) {
    const int64_t i = i0 + t;
    const bool on = i < n && A.in_pick[b0 + i] == 0;
    const bool cl = i < n && A.in_clique[b0 + i] != 0;
    const unsigned long long b = __ballot(on);
    const unsigned long long bc = __ballot(cl);
    const int before = __popcll(b & ((1ULL << lane) - 1));
    if (lane == 0) {
      s_wave[wave] = __popcll(b);
      s_cl[wave] = __popcll(bc);
    }
    __syncthreads();
    int woff = 0, tot = 0, totc = 0;
    for (int v = 0; v < PK_WAVES; ++v) {
      if (v < wave) woff += s_wave[v];
      tot += s_wave[v];
      totc += s_cl[v];
    }
    const int64_t pos = base + woff + before;
    if (on && pos < cap) {
      A.left_x[o0 + pos] = rint(A.bx[b0 + i]);
      A.left_y[o0 + pos] = rint(A.by[b0 + i]);
    }
    base += tot;
    ncl += totc;
    __syncthreads();
  }
  if (t == 0) {
    A.left_cnt[seg] = (int32_t)base;
    A.clique_cnt[seg] = (int32_t)ncl;
  }
}

}  // namespace

void launch_pick_members(hipStream_t stream, const PickMemArgs& A) {
  if (A.n_cols > 0) {
    const unsigned g = (unsigned)((A.n_cols + PK_NT - 1) / PK_NT);
    hipLaunchKernelGGL(k_pick_clique_mark, dim3(g), dim3(PK_NT), 0, stream, A);
  }
  if (A.n_picked > 0) {
    const unsigned g = (unsigned)((A.n_picked + PK_NT - 1) / PK_NT);
    hipLaunchKernelGGL(k_pick_members, dim3(g), dim3(PK_NT), 0, stream, A);
  }
}

void launch_pick_left(hipStream_t stream, const PickMemArgs& A) {
  if (A.n_mg <= 0) return;
  hipLaunchKernelGGL(k_pick_left, dim3((unsigned)(A.n_mg * A.k)), dim3(PK_NT), 0, stream, A);
}

void launch_pick_cols(hipStream_t stream, const PickArgs& A) {
  if (A.n_cols <= 0) return;
  const unsigned g = (unsigned)((A.n_cols + PK_NT - 1) / PK_NT);
  hipLaunchKernelGGL(k_pick_cols, dim3(g), dim3(PK_NT), 0, stream, A);
}

void launch_pick_select(hipStream_t stream, const PickArgs& A) {
  if (A.n_mg <= 0) return;
  hipLaunchKernelGGL(k_pick_select, dim3(A.n_mg), dim3(PK_NT), 0, stream, A);
  hipLaunchKernelGGL(k_pick_scan, dim3(1), dim3(PK_NT), 0, stream, A);
}

void launch_pick_emit(hipStream_t stream, const PickArgs& A) {
  if (A.n_mg <= 0) return;
  hipLaunchKernelGGL(k_pick_emit, dim3(A.n_mg), dim3(PK_NT), 0, stream, A);
}

}  // namespace rgc
