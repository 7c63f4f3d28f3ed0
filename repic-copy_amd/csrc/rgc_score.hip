// rgc_score.hip — particle-set scoring: the raster/reduce of score_detections.
//
// Reference repic/utils/score_detections.py:16-48 (get_segmentation_scores): every ground-
// truth and every picked box (above the confidence threshold) is painted into an int16
// (H x W) mask with numpy slice assignment; the scores are sum(pckr), sum(gt * pckr) and
// sum(gt).  Here the masks never exist in HBM: each workgroup owns one tile of the image
// (R rows x TW 64-pixel words, two 1-bit masks in LDS), paints the part of every box that
// falls into it with LDS atomic ORs, and reduces three popcounts into the pair's counters.
// The host normalises each box to its numpy slice bounds (Python slice.indices semantics:
// negative starts wrap, everything clamps to the mask), so a box is the pixel rectangle
// [r0, r1) x [c0, c1) with r0 < r1, c0 < c1.
#include "rgc_kernels.h"

namespace rgc {

constexpr int SC_WG = 256;
constexpr int SC_WORDS = 2048;   // 64-bit words per mask per tile (16 KB): 32 KB of LDS per WG

__device__ __forceinline__ void paint(uint64_t* m, int tr0, int tw0, int R, int TW, int4 b,
                                      int lane) {
  // overlap of box b with the tile, in tile-local rows and pixel columns
  const int pr0 = max(b.x, tr0), pr1 = min(b.y, tr0 + R);
  const int pc0 = max(b.z, tw0 * 64), pc1 = min(b.w, (tw0 + TW) * 64);
  if (pr0 >= pr1 || pc0 >= pc1) return;
  const int w0 = pc0 / 64, w1 = (pc1 - 1) / 64;   // inclusive word range
  const int nw = w1 - w0 + 1;
  const int items = (pr1 - pr0) * nw;
  for (int it = lane; it < items; it += 64) {
    const int r = pr0 + it / nw, w = w0 + it % nw;
    uint64_t bits = ~0ull;
    if (w == w0) bits &= ~0ull << (pc0 & 63);
    if (w == w1) bits &= ~0ull >> (63 - ((pc1 - 1) & 63));
    atomicOr(reinterpret_cast<unsigned long long*>(&m[(r - tr0) * TW + (w - tw0)]),
             (unsigned long long)bits);
  }
}

// One workgroup per (pair, tile).  Boxes of the pair are scanned in chunks of SC_WG: the ones
// touching the tile are compacted into LDS, then each wavefront paints whole boxes (lanes
// over the box's (row, word) items, so a 180 x 180 box is ~3 items per lane).
__global__ __launch_bounds__(SC_WG) void k_score_raster(ScoreArgs A) {
  __shared__ uint64_t m[2][SC_WORDS];
  __shared__ int list[SC_WG];
  __shared__ int nlist;
  __shared__ unsigned long long red[3][SC_WG / 64];
  const int t = blockIdx.x;
  const int p = A.tile_pair[t];
  const int tr0 = A.tile_r0[t], tw0 = A.tile_w0[t];
  const int R = A.R, TW = A.TW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < 2 * SC_WORDS; i += SC_WG) (&m[0][0])[i] = 0;
  const int tc0 = tw0 * 64, tc1 = (tw0 + TW) * 64;
  for (int which = 0; which < 2; ++which) {
    const int64_t b0 = which ? A.pk_off[p] : A.gt_off[p];
    const int64_t b1 = which ? A.pk_off[p + 1] : A.gt_off[p + 1];
    for (int64_t c0 = b0; c0 < b1; c0 += SC_WG) {
      if (tid == 0) nlist = 0;
      __syncthreads();
      const int64_t i = c0 + tid;
      if (i < b1) {
        const int4 b = A.boxes[i];
        if (b.x < tr0 + R && b.y > tr0 && b.z < tc1 && b.w > tc0)
          list[atomicAdd(&nlist, 1)] = (int)(i - c0);
      }
      __syncthreads();
      const int n = nlist;
      for (int j = wv; j < n; j += SC_WG / 64) paint(m[which], tr0, tw0, R, TW, A.boxes[c0 + list[j]], lane);
      __syncthreads();
    }
  }
  unsigned long long g = 0, k = 0, tp = 0;
  for (int i = tid; i < R * TW; i += SC_WG) {
    const uint64_t a = m[0][i], b = m[1][i];
    g += __popcll(a);
    k += __popcll(b);
    tp += __popcll(a & b);
  }
  for (int o = 32; o > 0; o >>= 1) {
    g += __shfl_xor(g, o, 64);
    k += __shfl_xor(k, o, 64);
    tp += __shfl_xor(tp, o, 64);
  }
  if (lane == 0) { red[0][wv] = g; red[1][wv] = k; red[2][wv] = tp; }
  __syncthreads();
  if (tid < 3) {
    unsigned long long s = 0;
    for (int w = 0; w < SC_WG / 64; ++w) s += red[tid][w];
    if (s) atomicAdd(&A.counts[3 * p + tid], s);
  }
}

// ---- threshold sweep: every confidence threshold of a list in one raster pass.
//
// The picks of a pair arrive ordered so that the ones kept at threshold j are the prefix
// [0, keep[j]) (keep non-increasing in j): pick i first appears at its level, the largest j with
// keep[j] > i, and stays for every lower j.  A pixel of the pick mask therefore first appears at
// the highest level of the picks covering it.  The LDS atomic OR that paints a word returns the
// word's earlier bits, so the lane that sets a bit knows it is the first to do so: it counts the
// bit (and the bit under the ground truth) for the level of its box.  counts[p][j] receives the
// pixels that FIRST appear at threshold j; the host's suffix sum over j turns them into the
// sums at each threshold.  Every box is painted once and no tile is ever reduced.
//
// Only the order between levels matters: a pick must not claim a pixel before a pick of a
// higher level has had its chance.  Picks are scanned in index order (= level descending) in
// chunks of SC_WG, compacted in that order, and the compacted list is painted one run of equal
// levels at a time with a barrier between runs.

// paint() that also counts the bits this lane is the first to set (and those under gt)
__device__ __forceinline__ void paint_fresh(uint64_t* m, const uint64_t* gt, int tr0, int tw0,
                                            int R, int TW, int4 b, int lane, unsigned& fresh,
                                            unsigned& fresh_gt) {
  const int pr0 = max(b.x, tr0), pr1 = min(b.y, tr0 + R);
  const int pc0 = max(b.z, tw0 * 64), pc1 = min(b.w, (tw0 + TW) * 64);
  if (pr0 >= pr1 || pc0 >= pc1) return;
  const int w0 = pc0 / 64, w1 = (pc1 - 1) / 64;   // inclusive word range
  const int nw = w1 - w0 + 1;
  const int items = (pr1 - pr0) * nw;
  for (int it = lane; it < items; it += 64) {
    const int r = pr0 + it / nw, w = w0 + it % nw;
    uint64_t bits = ~0ull;
    if (w == w0) bits &= ~0ull << (pc0 & 63);
    if (w == w1) bits &= ~0ull >> (63 - ((pc1 - 1) & 63));
    const int at = (r - tr0) * TW + (w - tw0);
    const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(&m[at]),
                                  (unsigned long long)bits);
    const uint64_t f = bits & ~old;
    fresh += __popcll(f);
    if (gt) fresh_gt += __popcll(f & gt[at]);
  }
}

// a wavefront's (fresh, fresh under gt) pixel counts of one level -> the pair's counters
__device__ __forceinline__ void sweep_flush(unsigned long long* cnt, unsigned a, unsigned b,
                                            int lane) {
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  if (lane == 0) {
    if (a) atomicAdd(&cnt[1], (unsigned long long)a);
    if (b) atomicAdd(&cnt[2], (unsigned long long)b);
  }
}

// One workgroup per (pair, tile), k_score_raster's tiling.  A lane's counters stay below the
// tile's 2^17 pixels.
__global__ __launch_bounds__(SC_WG) void k_score_sweep(ScoreArgs A, int T, const int64_t* keep) {
  __shared__ uint64_t m[2][SC_WORDS];
  __shared__ int list[SC_WG];     // touching boxes of the chunk, in index order: level << 8 | slot
  __shared__ int wcnt[SC_WG / 64];
  const int t = blockIdx.x;
  const int p = A.tile_pair[t];
  const int tr0 = A.tile_r0[t], tw0 = A.tile_w0[t];
  const int R = A.R, TW = A.TW;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int i = tid; i < 2 * SC_WORDS; i += SC_WG) (&m[0][0])[i] = 0;
  const int tc0 = tw0 * 64, tc1 = (tw0 + TW) * 64;
  const int64_t* kp = keep + (int64_t)p * T;
  unsigned long long* cnt = A.counts + (int64_t)p * T * 3;
  unsigned g = 0, none = 0;        // ground-truth pixels this lane set
  unsigned dk = 0, dtp = 0;        // pick pixels this lane was first to set at level cur
  int cur = 0;
  for (int which = 0; which < 2; ++which) {
    const int64_t b0 = which ? A.pk_off[p] : A.gt_off[p];
    const int64_t b1 = which ? b0 + kp[0] : A.gt_off[p + 1];
    for (int64_t c0 = b0; c0 < b1; c0 += SC_WG) {
      const int64_t i = c0 + tid;
      bool touch = false;
      int lvl = 0;
      if (i < b1) {
        const int4 b = A.boxes[i];
        touch = b.x < tr0 + R && b.y > tr0 && b.z < tc1 && b.w > tc0;
        if (touch && which) {        // largest j with keep[j] > i - b0 (keep[0] > i - b0 here)
          int hi = T;
          while (hi - lvl > 1) {
            const int mid = (lvl + hi) >> 1;
            if (kp[mid] > i - b0) lvl = mid; else hi = mid;
          }
        }
      }
      const unsigned long long bal = __ballot(touch);
      if (lane == 0) wcnt[wv] = __popcll(bal);
      __syncthreads();
      int n = 0, pos = 0;
      for (int w = 0; w < SC_WG / 64; ++w) {
        if (w < wv) pos += wcnt[w];
        n += wcnt[w];
      }
      if (touch) list[pos + __popcll(bal & ((1ull << lane) - 1))] = lvl << 8 | tid;
      __syncthreads();
      for (int s = 0; s < n;) {      // runs of equal level, highest first
        const int L = list[s] >> 8;
        int e = s;                   // end of the run: 64 entries per step, the same in every wave
        for (;;) {
          const unsigned long long same = __ballot(e + lane < n && (list[e + lane] >> 8) == L);
          const int c = same == ~0ull ? 64 : __ffsll((long long)~same) - 1;
          e += c;
          if (c < 64) break;
        }
        if (!which) {
          for (int j = s + wv; j < e; j += SC_WG / 64)
            paint_fresh(m[0], nullptr, tr0, tw0, R, TW, A.boxes[c0 + (list[j] & 255)], lane, g, none);
        } else if (s + wv < e) {
          if (L != cur) {
            sweep_flush(cnt + 3 * cur, dk, dtp, lane);
            dk = dtp = 0;
            cur = L;
          }
          for (int j = s + wv; j < e; j += SC_WG / 64)
            paint_fresh(m[1], m[0], tr0, tw0, R, TW, A.boxes[c0 + (list[j] & 255)], lane, dk, dtp);
        }
        if (e < n) __syncthreads();  // the next run is of a lower level
        s = e;
      }
    }
  }
  sweep_flush(cnt + 3 * cur, dk, dtp, lane);
  for (int o = 32; o > 0; o >>= 1) g += __shfl_xor(g, o, 64);
  if (lane == 0 && g) atomicAdd(&cnt[0], (unsigned long long)g);
}

int score_tile_words() { return SC_WORDS; }

void launch_score_raster(hipStream_t stream, int n_tiles, const ScoreArgs& A) {
  if (n_tiles > 0)
    hipLaunchKernelGGL(k_score_raster, dim3(n_tiles), dim3(SC_WG), 0, stream, A);
}

void launch_score_sweep(hipStream_t stream, int n_tiles, const ScoreArgs& A, int T,
                        const int64_t* keep) {
  if (n_tiles > 0)
    hipLaunchKernelGGL(k_score_sweep, dim3(n_tiles), dim3(SC_WG), 0, stream, A, T, keep);
}

}  // namespace rgc
