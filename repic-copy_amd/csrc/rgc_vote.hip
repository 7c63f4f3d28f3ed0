// rgc_vote.hip — `repic consensus --min_pickers`: the device glue between two tiers.
//
// After a tier's picks are emitted (rgc_pick.hip) the boxes they explain are marked, and the next
// lower tier runs the clique pipeline on what is left, once per picker subset:
//
//   k_vote_picks    per written pick of the tier: its unrounded consensus coordinates, its column
//                   weight, its picker mask and its members by picker.
//   k_vote_explain  one workgroup per micrograph: the tier's picks go through LDS in tiles of
//                   VOTE_TILE; every thread owns boxes and tests them against each pick with
//                   jaccard() of rgc_device.h (the reference's f64 operation order, strict `> t`,
//                   the test of rgc_nms); a box still at 0 that a pick explains gets the tier.
//                   A box or pick with a non-finite coordinate takes no part.  Brute force:
//                   boxes x picks per micrograph is small next to the clique kernels.
//   k_vote_count    per (micrograph, picker) segment: its boxes still at 0.
//   k_vote_gather   per pseudo-batch segment: ordered compaction, in file order, of its source
//                   segment's boxes still at 0 (k_pick_left's ballot / popcount / per-wave
//                   offsets) into the pseudo-batch's x / y / score, with origin[] back to the
//                   full batch.  Nothing is written past the segment's range.
//   k_vote_cols     the tier's run -> the set-packing solver's CSC inputs over full-batch rows,
//                   columns packed micrograph-major over the micrograph's pseudo-micrographs.
// gfx950, wave64, 256-thread workgroups.  No workgroup waits for another.
#include "rgc_device.h"
#include "rgc_kernels.h"

namespace rgc {

namespace {

constexpr int VT_NT = 256;
constexpr int VT_WAVES = VT_NT / 64;

__device__ inline bool vote_finite(double x, double y) { return isfinite(x) && isfinite(y); }

__global__ __launch_bounds__(VT_NT) void k_vote_picks(VotePickArgs A) {
  const int64_t i = (int64_t)blockIdx.x * VT_NT + threadIdx.x;
  if (i >= A.n_picked) return;
  const int m = range_of(A.pick_off, A.n_mg, i);
  const int64_t s = (A.src_base ? A.src_base[m] : A.col_off[m]) + A.pcol[i];
  const int64_t b = A.cons[s];
  const bool in_b = b >= 0 && b < A.n_box;   // (else the pick explains nothing)
  A.pcx[i] = in_b ? A.bx[b] : HUGE_VAL;
  A.pcy[i] = in_b ? A.by[b] : HUGE_VAL;
  A.pw[i] = A.w[s];
  const int mask = A.cmask ? A.cmask[s] : (1 << A.k) - 1;
  A.pmask[i] = mask;
  int j = 0;
  for (int p = 0; p < A.k; ++p) {
    const bool in = ((mask >> p) & 1) && j < A.t;
    A.pmember[i * A.k + p] = in ? A.members[s * A.t + j] : -1;
    j += in ? 1 : 0;
  }
}

__global__ __launch_bounds__(VT_NT) void k_vote_explain(VoteArgs A) {
  __shared__ double s_x[VOTE_TILE], s_y[VOTE_TILE];
  const int m = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t p0 = A.pick_off[m], np = A.pick_off[m + 1] - p0;
  if (np <= 0) return;   // (uniform per workgroup)
  const int64_t b0 = A.box_off[(int64_t)m * A.k], b1 = A.box_off[(int64_t)(m + 1) * A.k];
  for (int64_t j0 = 0; j0 < np; j0 += VOTE_TILE) {
    const int nj = (int)(np - j0 < VOTE_TILE ? np - j0 : VOTE_TILE);
    __syncthreads();
    for (int j = t; j < nj; j += VT_NT) {
      const double x = A.pcx[p0 + j0 + j], y = A.pcy[p0 + j0 + j];
      // (a pick off the finite plane overlaps nothing: +inf makes both overlaps 0)
      const bool fin = vote_finite(x, y);
      s_x[j] = fin ? x : HUGE_VAL;
      s_y[j] = fin ? y : HUGE_VAL;
    }
    __syncthreads();
    for (int64_t b = b0 + t; b < b1; b += VT_NT) {
      if (A.box_tier[b] != 0) continue;
      const double x = A.bx[b], y = A.by[b];
      if (!vote_finite(x, y)) continue;
      bool hit = false;
      for (int j = 0; j < nj && !hit; ++j)
        hit = jaccard(x, y, s_x[j], s_y[j], A.B, A.two_b2) > A.thr;
      if (hit) A.box_tier[b] = A.tier;
    }
  }
}

__global__ __launch_bounds__(VT_NT) void k_vote_count(VoteArgs A) {
  __shared__ int s_wave[VT_WAVES];
  const int64_t seg = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t b0 = A.box_off[seg], n = A.box_off[seg + 1] - b0;
  int cnt = 0;
  for (int64_t i = t; i < n; i += VT_NT) cnt += A.box_tier[b0 + i] == 0 ? 1 : 0;
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d, 64);
  if (lane == 0) s_wave[wave] = cnt;
  __syncthreads();
  if (t == 0) {
    int tot = 0;
    for (int v = 0; v < VT_WAVES; ++v) tot += s_wave[v];
    A.seg_cnt[seg] = tot;
  }
}

__global__ __launch_bounds__(VT_NT) void k_vote_gather(VoteArgs A) {
  __shared__ int s_wave[VT_WAVES];
  const int64_t u = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t seg = A.pseg_src[u];
  const int64_t b0 = A.box_off[seg], n = A.box_off[seg + 1] - b0;
  const int64_t o0 = A.pbox_off[u], cap = A.pbox_off[u + 1] - o0;
  int64_t base = 0;
  for (int64_t i0 = 0; i0 < n; i0 += VT_NT) {
    const int64_t i = i0 + t;
    const bool on = i < n && A.box_tier[b0 + i] == 0;
    const unsigned long long b = __ballot(on);
    const int before = __popcll(b & ((1ULL << lane) - 1));
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int v = 0; v < VT_WAVES; ++v) {
      if (v < wave) woff += s_wave[v];
      tot += s_wave[v];
    }
    const int64_t pos = base + woff + before;
    if (on && pos < cap) {
      A.gx[o0 + pos] = A.bx[b0 + i];
      A.gy[o0 + pos] = A.by[b0 + i];
      A.gs[o0 + pos] = A.bs[b0 + i];
      A.origin[o0 + pos] = (int32_t)(b0 + i);
    }
    base += tot;
    __syncthreads();
  }
  if (t == 0) A.pseg_cnt[u] = (int32_t)base;
}

__global__ __launch_bounds__(VT_NT) void k_vote_cols(VoteColArgs A) {
  const int64_t c = (int64_t)blockIdx.x * VT_NT + threadIdx.x;
  if (c == 0) A.col_ptr[A.n_cols] = A.n_cols * A.t;
  if (c >= A.n_cols) return;
  const int q = range_of(A.qcol_off, A.n_q, c);
  const int64_t src = A.q_src[q] + (c - A.qcol_off[q]);
  bool bad = false;
  for (int j = 0; j < A.t; ++j) {
    const int64_t mb = A.members[src * A.t + j];
    const bool in = mb >= 0 && mb < A.n_pbox;
    int32_t full = in ? A.origin[mb] : 0;
    if (full < 0 || full >= A.n_box) { full = 0; bad = true; }
    bad = bad || !in;
    A.row_idx[c * A.t + j] = full;
    A.cmemb[c * A.t + j] = full;
  }
  const int64_t cb = A.cons[src];
  const bool cin = cb >= 0 && cb < A.n_pbox;
  int32_t cfull = cin ? A.origin[cb] : 0;
  if (cfull < 0 || cfull >= A.n_box) { cfull = 0; bad = true; }
  bad = bad || !cin;
  const float w = A.w[src];
  A.w64[c] = (double)w;
  A.cw[c] = w;
  A.cconf[c] = A.conf[src];
  A.ccons[c] = cfull;
  A.cmask[c] = A.q_mask[q];
  A.col_ptr[c] = c * A.t;
  A.col_mg[c] = A.q_mg[q];
  if (bad) *A.bad = 1;
}

}  // namespace

void launch_vote_picks(hipStream_t stream, const VotePickArgs& A) {
  if (A.n_picked <= 0) return;
  const unsigned g = (unsigned)((A.n_picked + VT_NT - 1) / VT_NT);
  hipLaunchKernelGGL(k_vote_picks, dim3(g), dim3(VT_NT), 0, stream, A);
}

void launch_vote_explain(hipStream_t stream, const VoteArgs& A) {
  if (A.n_mg <= 0) return;
  hipLaunchKernelGGL(k_vote_explain, dim3(A.n_mg), dim3(VT_NT), 0, stream, A);
}

void launch_vote_count(hipStream_t stream, const VoteArgs& A) {
  if (A.n_mg <= 0) return;
  hipLaunchKernelGGL(k_vote_count, dim3((unsigned)(A.n_mg * A.k)), dim3(VT_NT), 0, stream, A);
}

void launch_vote_gather(hipStream_t stream, const VoteArgs& A) {
  if (A.n_pseg <= 0) return;
  hipLaunchKernelGGL(k_vote_gather, dim3((unsigned)A.n_pseg), dim3(VT_NT), 0, stream, A);
}

void launch_vote_cols(hipStream_t stream, const VoteColArgs& A) {
  if (A.n_cols <= 0) return;
  const unsigned g = (unsigned)((A.n_cols + VT_NT - 1) / VT_NT);
  hipLaunchKernelGGL(k_vote_cols, dim3(g), dim3(VT_NT), 0, stream, A);
}

}  // namespace rgc
