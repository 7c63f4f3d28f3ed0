// rgc_fused.hip — the whole get_cliques hot path for one micrograph in ONE workgroup.
//
// Everything between reading a micrograph's boxes and writing its ILP structures stays in
// LDS: boxes (f32 or f64 x/y), one uniform grid per picker, the forward adjacency CSR (u16
// targets), union-find, the clique DFS and the vertex ranks.  Graph nodes are the boxes'
// SORTED POSITIONS (picker-major grid order, local index order inside a cell): stencil
// ranges then yield every forward list already sorted, and all per-node arrays are indexed
// by position; local (file-order) indices only enter where the reference orders by box id.  HBM sees
// the compulsory traffic only: 16 B/box of coordinates in, 8 B per clique member of scores
// in (gathered), and C*(4k + 12) bytes of clique outputs out.  No global scans, no
// mid-pipeline host syncs, no global atomics except one clique-range reservation per
// micrograph.  Micrographs whose boxes/edges do not fit the launch's LDS capacities are
// returned with status DEFER and run through the multi-kernel path (rgc_kernels.hip).
//
// Phases (barrier-separated), reference repic/commands/get_cliques.py:
//   P0 load x, y; bounding box
//   P1 grid + LDS counting sort by cell                       (pair loop structure :62-63)
//   P2 JI pairs: count and write each sorted list, one pass   (:40-46, :59-69, :138)
//   P3 union-find, CC stats, --get_cc target                  (:145-156)
//   P4 k-clique DFS count, mark vertices, reserve outputs    (:49-56, :160-161)
//   P5 vertex rank by (x, y, id) via x-major grid columns    (:164, :193)
//   P6 clique DFS fill + epilogue + COO rows                 (:169-202)
#pragma clang fp contract(off)

#include <type_traits>

#ifdef RGC_STAMPS
// Diagnostic build only: every workgroup barrier of this file (and of the rgc_device.h scans
// it inlines) adds the cycles each wave waits in it to that wave's counter, read and reset by
// STAMP at each phase end, so a phase's barrier-wait share (waves idle behind the slowest
// wave of the workgroup) separates from its other stalls.
#include <hip/hip_runtime.h>
namespace rgc {
__shared__ unsigned long long g_bwait[16];
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void timed_barrier() {
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  raw_barrier();
  if ((threadIdx.x & 63) == 0) g_bwait[threadIdx.x >> 6] += __builtin_amdgcn_s_memtime() - t0;
}
}  // namespace rgc
#define __syncthreads() ::rgc::timed_barrier()
#endif

#include "rgc_device.h"
#include "rgc_kernels.h"

namespace rgc {

constexpr int MAXW = 16;            // reduction slots: up to 1024-thread workgroups
// Workgroup sizes compiled: 512 for every k; 768 / 1024 threads (12 / 16 waves) for k <= 5,
// launched when LDS allows few workgroups per CU but VGPRs allow more waves (rgc_run.cpp);
// 256 threads for k <= 3 (fewer per-wave fixed costs per micrograph, fewer resident waves).
// boxes per thread kept in registers from P0 to P1: 2 (4 with 256-thread workgroups; 5 with
// 1024: C3's ~4.1k boxes all stay in registers, VGPRs to spare at 4 waves per SIMD; boxes past
// RB * NT are re-read from HBM in each of P0's and P1's passes)
constexpr int fused_rb(int nt) { return nt <= 256 ? 4 : nt >= 1024 ? 5 : 2; }
// of those, the boxes whose P1 key and arrival ordinal stay in a register from the count to
// the placement (the others park both in LDS), and the positions whose P5 bucket and ordinal
// stay in one across the scan.  The 1024-thread instances hold none: with five more live
// registers in P1 or P5 they drop an occupancy step (`make resources`).
constexpr int fused_rq(int nt) { return nt >= 1024 ? 0 : fused_rb(nt); }
constexpr int fused_rv(int nt) { return nt >= 1024 ? 0 : fused_rb(nt); }
// The per-box / per-edge / per-vertex loops of P1, P2c, P3, P5 and P6a run one item of a thread
// at a time, each iteration staged: its loads at known addresses first, then the flag test,
// then the action.  That order is the measured gain.  Keeping two items of a thread in flight
// on top of it was inside the spread or slower in every phase (DESIGN.md section 4,
// profiles/r11f); those pair forms were taken out of the source and rebuild from a42a7dc.
// Two barriers are off the workgroup's chain because their work sits in front of one that is
// there anyway: P5's counter zeroing in front of P4's reservation barrier, and P3b's stats
// summed behind P4's barriers when --get_cc is off (profiles/r12; the switches that timed
// them rebuild from 25f33ec).  A third goes with P3b's second loop: the compress loop takes the
// stats itself, and where P4's root pass only reads (the one-trip form) nothing waits for it.

struct FusedHdr {
  // reduction scratch: the single-value reductions alias the 4-way one (every reduction
  // starts behind a barrier)
  union {
    struct {
      double redd[MAXW];
      int64_t red64[MAXW];
      uint64_t redu[MAXW];
      int redi[MAXW];
    };
    double red4[4][MAXW];
  };
  double minx, miny, cell, inv_cell, inv_celly;
  double xbs;       // P5 x-bucket scale: bucket(x) = min(trunc((x - minx) * xbs), n - 1)
  float inv_gy;
  int gx, gy, ncell, nkey;   // per-picker grid gx x gy; keys picker * ncell + cell; nkey = none
  // E: forward edges; P2's cursor (each wave-round reserves its block's lists on it)
  int E, nodes, cc_cnt, cc_max, V, status;
  uint32_t ccur;    // P4 clique-queue cursor
  uint32_t ntie;    // P6: cliques handed to k_fused_ties so far (the next one's segment slot)
  int tief[2];      // P6: some clique of the chunk needs the second loop (by chunk parity)
  int qslot;        // QG (K = 4): the workgroup's HBM level-tree slot (-1: none, LDS queue)
  int64_t C, base;
};

// cell budget (keys over all pickers' grids) of a size class: 4 n up to 2048 boxes; 2 n above,
// where LDS is the limit (one workgroup per CU) and larger cells only cost P2 candidates
__host__ __device__ inline int fused_cells(int nmax) { return nmax <= 2048 ? 4 * nmax : 2 * nmax; }

// P2 reserves the lists of one aligned block of 64 positions at a time, in the waves' arrival
// order, so a box's list ends where the next box's begins only inside a block: fwd holds every
// box's list begin, and bend (behind fwd's fwd_blocks(nmax) * 64 begins) every block's end, read
// for the last box of a block only.  A begin costs what it did with one monotone offset array
// (P4's level expansion reads begins only).
__host__ __device__ inline int fwd_blocks(int nmax) { return (nmax + 63) / 64; }

// wide: f64 coordinates in LDS; otherwise f32 (every coordinate of the micrograph is exactly
// representable as f32, checked in P0, so the f64 values are recovered exactly)
__host__ __device__ inline FusedLayout fused_layout(int nmax, int ecap, bool wide) {
  FusedLayout L;
  auto al = [](int v) { return (v + 15) & ~15; };
  int o = al((int)sizeof(FusedHdr));
  // live until the end of the kernel
  L.off_sxy = o; o += al((wide ? 16 : 8) * nmax);   // (x, y) in cell-sorted order
  L.off_cnt = o; o += al(4 * (nmax + 4));
  // u16 list bounds (E <= ecap <= 65535): each box's list begin, then each block's end (bend)
  L.off_fwd = o; o += al(2 * (fwd_blocks(nmax) * 65 + 4));
  L.off_pos = o; o += al(2 * nmax);           // local box index -> sorted position
  L.off_vrank = o; o += al(2 * nmax);
  L.off_dst = o; o += al(2 * ecap);
  // P1-P3 grid and union-find; the cell starts (dead after P2) become the clique buffer of
  // P4-P6, parent..scell (dead after P5) the f64 scores of P6
  L.off_union = o;
  L.off_cstart = o; o += al(2 * (fused_cells(nmax) + 8));   // u16 cell starts
  L.off_parent = o; o += al(2 * (nmax + 8));    // u16 union-find parents; P5 u16 bucket counts
  L.off_scell = o; o += al(2 * nmax);         // sorted position -> cell
  L.off_citems = o; o += al(2 * nmax);        // sorted position -> local box index
  L.off_flags = o; o += al(nmax);             // by local index: 1 graph node, 3 clique vertex
  L.off_smark = o;
  L.total = o;
  L.off_cbuf = L.off_cstart;
  return L;
}

int fused_lds_bytes(int nmax, int ecap, bool wide) { return fused_layout(nmax, ecap, wide).total; }

struct FShared {
  void* sxy;        // cell-sorted coordinates: double2 (wide) or float2
  uint16_t* cstart;
  uint32_t* cnt;
  uint16_t* fwd;
  uint16_t* bend;   // end of each block's lists (see fwd_blocks)
  uint16_t* parent;
  uint16_t* citems;
  uint16_t* pos;
  uint16_t* scell;
  uint16_t* vrank;
  uint8_t* flags;   // by local index: 0 no edge, 1 graph node, 3 clique vertex
  uint16_t* dst;
  uint16_t* split;  // P2-P4 (scell region): end of each box's first picker segment in dst,
                    // written by P2 beside fwd (position ts's slot once its thread has read
                    // scell[ts])
  uint16_t* cbuf;   // P4-P6 (cell starts): clique queue, or the current chunk of the re-walk
  double* vscore;   // P6 (parent..scell, dead after P5): score of each clique vertex by row
                    // rank, used when 8 V bytes fit there (vstaged); else scores are
                    // gathered from HBM
  bool vstaged;
  // forward list of the box at position i: dst[eb(i), ee(i))
  __device__ __forceinline__ int eb(int i) const { return fwd[i]; }
  __device__ __forceinline__ int ee(int i) const {
    return (i & 63) == 63 ? bend[i >> 6] : fwd[i + 1];
  }
};

template <bool W>
__device__ __forceinline__ double2 ld_xy(const FShared& S, int t) {
  if constexpr (W) {
    return reinterpret_cast<const double2*>(S.sxy)[t];
  } else {
    const float2 f = reinterpret_cast<const float2*>(S.sxy)[t];
    return make_double2((double)f.x, (double)f.y);
  }
}
template <bool W>
__device__ __forceinline__ void st_xy(const FShared& S, int t, double x, double y) {
  if constexpr (W) reinterpret_cast<double2*>(S.sxy)[t] = make_double2(x, y);
  else reinterpret_cast<float2*>(S.sxy)[t] = make_float2((float)x, (float)y);
}

template <int K>
struct FCtx {
  // copies of the kernel arguments (taking the address of the kernarg struct would move it
  // to scratch)
  double B, two_b2;
  float Bf, two_b2f;   // (float) copies, wave-uniform (SGPRs)
  int flags;
  gptr<const double> score;
  gptr<int32_t> rows;
  gptr<float> w;
  gptr<float> conf;
  gptr<int32_t> consensus;
  gptr<int32_t> members;
  gptr<uint8_t> order;
  FShared S;
  int pb[K + 1];     // picker bounds (local box indices)
  int pp[K + 1];     // picker bounds (sorted positions; pp[K] = first non-finite box)
  int m, b0, n;
  int64_t idb;       // global id of local box 0
  bool set_order;    // networkx iterates set(sorted(clique)) (2k < |G|)
  int64_t out;       // next clique index within the micrograph (fill)
  int64_t c0, c1;    // clique chunk being buffered in cbuf (fill)
  int64_t count;
  uint16_t* cq_ord;  // P4 queue: ordinal of each queued clique within its root's DFS
  uint32_t* ccur;    // P4 queue cursor (LDS)
  int cq_cap;        // P4 queue capacity (cliques)
  // cliques left to k_fused_ties: the micrograph's segment of the tie list (it starts at the
  // micrograph's own clique base) and the LDS counter that hands out its slots
  gptr<int32_t> tie_seg;
  uint32_t* ntie;
};

__device__ __forceinline__ uint32_t lds_ld(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_st(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t p16_ld(uint16_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void p16_st(uint16_t* p, uint32_t v) {
  __hip_atomic_store(p, (uint16_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// u16 parents (positions < 2^16), path halving
__device__ __forceinline__ uint32_t uf_find_lds(uint16_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = p16_ld(parent + x);
    if (p == x) return x;
    const uint32_t gp = p16_ld(parent + p);
    if (gp != p) p16_st(parent + x, gp);
    x = gp;
  }
}
// lock-free union (link the larger root under the smaller): CAS on the 32-bit word holding
// the root's u16 entry (a concurrent store to the other half only makes the CAS retry)
__device__ __forceinline__ void uf_union_lds(uint16_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find_lds(parent, a);
    b = uf_find_lds(parent, b);
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    uint32_t* wp = reinterpret_cast<uint32_t*>(parent) + (a >> 1);
    const int sh = 16 * (a & 1);
    const uint32_t w = lds_ld(wp);
    if (((w >> sh) & 0xFFFFu) != a) continue;   // a was linked meanwhile
    const uint32_t nw = (w & ~(0xFFFFu << sh)) | (b << sh);
    if (atomicCAS(wp, w, nw) == w) return;
  }
}

// u32 parents (the dead P2 count words, see P2's union): path halving by plain stores (any
// ancestor is a valid parent, and parents only ever decrease), linking by atomicMin of the
// larger root's word to the smaller root - no CAS retry loop, no false conflicts between two
// u16 halves of one word.  If the larger root was linked meanwhile (old != a), its old parent
// and b are joined in turn (hooking as in ECL-CC).
__device__ __forceinline__ uint32_t uf_find32(uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = lds_ld(parent + x);
    if (p == x) return x;
    const uint32_t gp = lds_ld(parent + p);
    if (gp != p) lds_st(parent + x, gp);
    x = gp;
  }
}
// the find of x given p, a value loaded from parent[x] earlier (a stale p is still an ancestor
// of x, or x itself if x was a root then: the race every find here has with a concurrent link)
__device__ __forceinline__ uint32_t uf_find32p(uint32_t* parent, uint32_t x, uint32_t p) {
  if (p == x) return x;
  const uint32_t gp = lds_ld(parent + p);
  if (gp != p) lds_st(parent + x, gp);
  return uf_find32(parent, gp);
}
// union of a and b given pa, pb loaded from parent[a], parent[b]: the caller issues those loads
// (of both endpoints) together
__device__ __forceinline__ void uf_union32p(uint32_t* parent, uint32_t a, uint32_t pa,
                                            uint32_t b, uint32_t pb) {
  a = uf_find32p(parent, a, pa);
  b = uf_find32p(parent, b, pb);
  for (;;) {
    if (a == b) return;
    if (a < b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicMin(parent + a, b);
    if (old == a) return;
    a = uf_find32(parent, old);
    b = uf_find32(parent, b);
  }
}
__device__ __forceinline__ void uf_union32(uint32_t* parent, uint32_t a, uint32_t b) {
  const uint32_t pa = lds_ld(parent + a), pb = lds_ld(parent + b);
  uf_union32p(parent, a, pa, b, pb);
}

template <int K>
__device__ __forceinline__ int picker_of(const int (&pb)[K + 1], int i) {
  int p = 0;
#pragma unroll
  for (int q = 1; q < K; ++q) p += (i >= pb[q]);
  return p;
}
// first box index after box i's picker.  Written as sums of differences, never as a select
// between array elements: the optimiser folds such selects into a dynamically indexed load,
// which would move the whole context struct to scratch.
template <int K>
__device__ __forceinline__ int picker_end(const int (&pb)[K + 1], int i) {
  int e = pb[1];
#pragma unroll
  for (int q = 1; q < K; ++q) e += (i >= pb[q]) ? (pb[q + 1] - pb[q]) : 0;
  return e;
}
// end (in box index) of the picker after box i's picker: targets of box i below it form the
// first segment of i's forward list
template <int K>
__device__ __forceinline__ int next_picker_end(const int (&pb)[K + 1], int i) {
  int e = pb[K < 2 ? K : 2];
#pragma unroll
  for (int q = 1; q < K; ++q) e += (i >= pb[q]) ? (q + 2 <= K ? pb[q + 2] - pb[q + 1] : 0) : 0;
  return e;
}
template <int K>
__device__ __forceinline__ int picker_begin(const int (&pb)[K + 1], int p) {
  int b = pb[0];
#pragma unroll
  for (int q = 1; q < K; ++q) b += (p >= q) ? (pb[q] - pb[q - 1]) : 0;
  return b;
}

__device__ __forceinline__ int lb16(const uint16_t* a, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// lb16 with select-updated bounds: a step is a probe and two selects, no branch on the compare
// (an empty range, lo >= hi, probes nothing and returns lo)
__device__ __forceinline__ int lb16s(const uint16_t* a, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool up = (int)a[mid] < v;
    lo = up ? mid + 1 : lo;
    hi = up ? hi : mid;
  }
  return lo;
}

__device__ __forceinline__ bool contains16(const uint16_t* a, int lo, int hi, int v) {
  const int p = lb16(a, lo, hi, v);
  return p < hi && (int)a[p] == v;
}

// wave-uniform copies (SGPRs) of values every lane reads from the LDS header
__device__ __forceinline__ int ufl(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uff(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ double ufd(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xFFFFFFFF));
  const int hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ int64_t ufl64(int64_t v) {
  const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xFFFFFFFF));
  const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// the micrograph's grid geometry, uniform across the workgroup
struct GridU {
  double minx, miny, inv_cell, inv_celly;   // columns >= 2 row_min wide, rows >= row_min tall
  float inv_cellf;                          // (float)inv_cell: P2's half-column test
  float inv_gy;
  int gx, gy, ncell, nkey;
};
__device__ __forceinline__ GridU grid_u(const FusedHdr& H) {
  GridU G;
  G.minx = ufd(H.minx); G.miny = ufd(H.miny); G.inv_cell = ufd(H.inv_cell);
  G.inv_celly = ufd(H.inv_celly); G.inv_cellf = uff((float)H.inv_cell);
  G.inv_gy = uff(H.inv_gy);
  G.gx = ufl(H.gx); G.gy = ufl(H.gy); G.ncell = ufl(H.ncell); G.nkey = ufl(H.nkey);
  return G;
}

// P1 sort key of a box of picker p: its cell in picker p's grid (x-major), or nkey when the
// box cannot have an edge (non-finite coordinates).  Monotone in x and y per picker.
// f32 layout (!W): on floats.  The column is floor of the very product P2's half-column test
// takes (f32 difference of the exact f32 values, times (float)inv_cell), and any consistent
// map with the cell sizes' slack keeps the stencil exact (see P1).
template <bool W>
__device__ __forceinline__ int box_key(const GridU& H, int p, double x, double y) {
  if (H.ncell == 0 || !isfinite(x) || !isfinite(y)) return H.nkey;
  int cx, cy;
  if constexpr (W) {
    cx = (int)fmin(floor((x - H.minx) * H.inv_cell), (double)(H.gx - 1));
    cy = (int)fmin(floor((y - H.miny) * H.inv_celly), (double)(H.gy - 1));
  } else {
    cx = min((int)floorf(((float)x - (float)H.minx) * H.inv_cellf), H.gx - 1);
    cy = min((int)floorf(((float)y - (float)H.miny) * (float)H.inv_celly), H.gy - 1);
  }
  return p * H.ncell + cx * H.gy + cy;
}

// graph insertion key of a clique vertex u (a position; tiny graphs only): first appearance
// of the node in the edge enumeration (picker pair, a index, b index, side) in local (file)
// order, get_cliques.py:33-34,135-143
template <int K>
__device__ __forceinline__ uint64_t ins_key(const FCtx<K>& c, int u) {
  const int pu = picker_of<K>(c.pp, u);
  const int bu = picker_begin<K>(c.pb, pu);
  const int lu = (int)c.S.citems[u] - bu;
  for (int a = 0; a < bu; ++a) {   // lower-picker boxes in file order
    const int ap = c.S.pos[a];
    if (contains16(c.S.dst, c.S.eb(ap), c.S.ee(ap), u)) {
      const int qa = picker_of<K>(c.pb, a);
      return ((uint64_t)pair_index(qa, pu, K) << 49) |
             ((uint64_t)(a - picker_begin<K>(c.pb, qa)) << 25) | ((uint64_t)lu << 1) | 1ULL;
    }
  }
  // no incoming edge: its first outgoing edge = lowest target picker, smallest file index
  const int e0 = c.S.eb(u), e1 = c.S.ee(u);
  const int d0 = c.S.dst[e0];
  const int pd = picker_of<K>(c.pp, d0);
  const int se = lb16(c.S.dst, e0, e1, picker_end<K>(c.pp, d0));
  int dmin = 1 << 30;
  for (int e = e0; e < se; ++e) dmin = min(dmin, (int)c.S.citems[c.S.dst[e]]);
  return ((uint64_t)pair_index(pu, pd, K) << 49) | ((uint64_t)lu << 25) |
         ((uint64_t)(dmin - picker_begin<K>(c.pb, pd)) << 1);
}

// A clique this kernel does not decide (set-order micrographs: the f32 degrees are within the
// margin, or --multi_out wants the node order) goes to k_fused_ties: the next slot of the
// micrograph's tie segment, handed out by an LDS counter (the segment has a slot per clique of
// the micrograph, so nothing is counted in HBM and nothing can overflow).  li = the members'
// local (file-order) indices in picker order.
template <int K>
__device__ __forceinline__ void fused_tie_handoff(const FCtx<K>& c, int64_t j, const int (&li)[K]) {
  const uint32_t t = atomicAdd(c.ntie, 1u);
  gptr<int32_t> e = c.tie_seg + (int64_t)t * (4 + K);
  e[0] = (int32_t)(uint32_t)(uint64_t)j;
  e[1] = (int32_t)(uint32_t)((uint64_t)j >> 32);
  e[2] = c.m;
  e[3] = (c.flags & 2) ? 1 : 0;
#pragma unroll
  for (int i = 0; i < K; ++i) e[4 + i] = c.b0 + li[i];
}

// what fused_epilogue_main does with a clique it cannot decide: a set-order micrograph's is
// handed off on the spot (every instance affords the entry store inside P6's main loop: none
// loses an occupancy step or gains scratch for it, `make resources`); true = an insertion-order
// graph's, flagged for the second loop
template <int K>
__device__ __forceinline__ bool fused_undecided(const FCtx<K>& c, int64_t j, const int (&li)[K]) {
  if (c.set_order) {
    fused_tie_handoff<K>(c, j, li);
    return false;
  }
  return true;
}

// ILP epilogue of one buffered clique (thread per clique): reference get_cliques.py:169-202.
// j = output index; mem = member positions in picker order.  Main pass: COO rows, weight,
// confidence, members and the consensus when one member's weighted degree is the largest by
// a clear margin.  Anything closer, and every clique under --multi_out, is decided exactly
// elsewhere: k_fused_ties for set-order micrographs (fused_undecided), the second loop's
// fused_epilogue_order for the tiny insertion-order graphs (returns true for those).
// INTP (integer coordinates below 2^23, B <= 2896, f32 layout): every overlap B - |dx| and
// product is an integer below 2^24, exact in f32, so the overlaps, their median network and the
// f32 degree JIs (2 B^2 - I exact too) run on floats; the median overlaps are converted back
// to f64 exactly for the reference's divisions.  Same results, half the registers.
template <int K, bool W, bool INTP = false>
__device__ __forceinline__ bool fused_epilogue_main(const FCtx<K>& c, int64_t j,
                                                    const int (&mem)[K]) {
  constexpr int NE = K * (K - 1) / 2;
  using OT = typename std::conditional<INTP, float, double>::type;
  OT I[NE];       // overlaps of the member pairs (a < b) in reference op order
  int li[K];      // local (file-order) indices: id order
  {
    double s[K];
    OT xs[K], ys[K];
    int r[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      if constexpr (INTP) {
        const float2 xy = reinterpret_cast<const float2*>(c.S.sxy)[mem[i]];
        xs[i] = xy.x;
        ys[i] = xy.y;
      } else {
        const double2 xy = ld_xy<W>(c.S, mem[i]);
        xs[i] = xy.x;
        ys[i] = xy.y;
      }
      li[i] = c.S.citems[mem[i]];
      r[i] = c.S.vrank[mem[i]];
    }
    if (c.S.vstaged) {
#pragma unroll
      for (int i = 0; i < K; ++i) s[i] = c.S.vscore[r[i]];
    } else {
#pragma unroll
      for (int i = 0; i < K; ++i) s[i] = c.score[c.b0 + li[i]];
    }
    cmpnet_apply<K, false>(r);   // ascending rows
#pragma unroll
    for (int i = 0; i < K; ++i) c.rows[j * K + i] = r[i];
    {
      int t = 0;
#pragma unroll
      for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = a + 1; b < K; ++b) {
          if constexpr (INTP) {
            I[t++] = fmaxf(c.Bf - fabsf(xs[a] - xs[b]), 0.0f) *
                     fmaxf(c.Bf - fabsf(ys[a] - ys[b]), 0.0f);
          } else {
            I[t++] = overlap(xs[a], ys[a], xs[b], ys[b], c.B);
          }
        }
    }
    // conf = f32(median score); w = f32(f64(conf) * median JI) where median JI = JI of the
    // median overlap (JI = I / (2 B^2 - I) is non-decreasing in I, so sorting by I sorts the
    // JIs): one or two reference divisions instead of one per pair
    const double cf = median_n<K>(s);
    OT Is[NE];
#pragma unroll
    for (int t = 0; t < NE; ++t) Is[t] = I[t];
    double med;
    if constexpr (INTP) {   // finite integers: no NaN
      mid_n<NE>(Is);
      if (NE & 1) {
        med = (double)Is[NE / 2];
        med = med / (c.two_b2 - med);
      } else {
        const double a = (double)Is[NE / 2 - 1], b = (double)Is[NE / 2];
        med = ((a / (c.two_b2 - a)) + (b / (c.two_b2 - b))) / 2.0;
      }
    } else if (NE & 1) {
      med = median_n<NE>(Is);   // sorted copy's middle element
      med = med / (c.two_b2 - med);
    } else {
      bool nan = false;
#pragma unroll
      for (int t = 0; t < NE; ++t) nan |= isnan(Is[t]);
      mid_n<NE>(Is);
      const double a = Is[NE / 2 - 1], b = Is[NE / 2];
      med = nan ? NAN : ((a / (c.two_b2 - a)) + (b / (c.two_b2 - b))) / 2.0;
    }
    const float conf32 = (float)cf;
    c.w[j] = (float)((double)conf32 * med);
    c.conf[j] = conf32;
  }
  if (c.flags & (2 | 32)) {
#pragma unroll
    for (int i = 0; i < K; ++i) c.members[j * K + i] = c.b0 + li[i];
  }
  if (c.flags & 2) return fused_undecided<K>(c, j, li);
  // weighted degrees from f32 JIs: f32 operands (2^-24 each) and v_rcp_f32 (1 ulp) give
  // < 4e-7 per JI <= 1, < 5.5e-6 per sum of <= 7 terms with its f32 additions; a maximum
  // clear by 3e-5 is the reference's, anything closer goes to an exact f64 pass
  float deg[K];
#pragma unroll
  for (int i = 0; i < K; ++i) deg[i] = 0.0f;
  {
    int t = 0;
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
      for (int b = a + 1; b < K; ++b) {
        float jf;
        if constexpr (INTP) jf = I[t] * __builtin_amdgcn_rcpf(c.two_b2f - I[t]);
        else jf = (float)I[t] * __builtin_amdgcn_rcpf((float)(c.two_b2 - I[t]));
        deg[a] += jf;
        deg[b] += jf;
        ++t;
      }
  }
  float d1 = deg[0], d2 = -INFINITY;
  int arg = 0;
#pragma unroll
  for (int i = 1; i < K; ++i) {
    const float d = deg[i];
    d2 = d > d1 ? d1 : fmaxf(d2, d);
    arg = d > d1 ? i : arg;
    d1 = fmaxf(d1, d);
  }
#ifndef RGC_ABL_NO_TIES
  // (ablation build only, RGC_ABL_NO_TIES: every maximum counts as clear -- what the kernel
  // would cost with no near-tie to hand off; its consensus is wrong by design)
  if (!(d1 - d2 > 3e-5f)) return fused_undecided<K>(c, j, li);
#endif
  int cons = li[0];
#pragma unroll
  for (int i = 1; i < K; ++i) cons = (arg == i) ? li[i] : cons;
  c.consensus[j] = c.b0 + cons;
  return false;
}

// second loop, insertion-order graphs (2k >= |G|, tiny): the exact f64 degrees, graph insertion
// order (ins_key reads the LDS graph, so this stays in the kernel), consensus among the tied
// maximal members, and the --multi_out member order
template <int K, bool W>
__device__ __forceinline__ void fused_epilogue_order(const FCtx<K>& c, int64_t j,
                                                     const int (&mem)[K]) {
  double ji[K][K], xs[K], ys[K];
  int li[K];
  uint64_t ins[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double2 xy = ld_xy<W>(c.S, mem[i]);
    xs[i] = xy.x;
    ys[i] = xy.y;
    li[i] = c.S.citems[mem[i]];
  }
#pragma unroll
  for (int a = 0; a < K; ++a)
#pragma unroll
    for (int b = a + 1; b < K; ++b) ji[a][b] = jaccard(xs[a], ys[a], xs[b], ys[b], c.B, c.two_b2);
  for (int i = 0; i < K; ++i) ins[i] = ins_key<K>(c, mem[i]);
  uint32_t top;
  int arg = epi_degree_max<K>(ji, &top);
  const bool tie = (top & (top - 1)) != 0;
  const bool multi = (c.flags & 2) != 0;
  if (tie || multi) {
    const uint32_t ord = node_order_ins<K>(ins);
    if (tie) arg = epi_tie_arg<K>(top, ord);
    if (multi) {
#pragma unroll
      for (int i = 0; i < K; ++i) c.order[j * K + i] = (uint8_t)((ord >> (4 * i)) & 15);
    }
  }
  int cons = li[0];
#pragma unroll
  for (int i = 1; i < K; ++i) cons = (arg == i) ? li[i] : cons;
  c.consensus[j] = c.b0 + cons;
}

// Static-recursion DFS: level D picks the picker-D member among the forward neighbours of
// the picker-(D-1) member that are also forward neighbours of every earlier member.
template <int K, int D, bool FILL>
struct FLevel {
  __device__ __forceinline__ static void run(FCtx<K>& c, int (&mem)[K]) {
    // the picker-D neighbours of mem[D-1] (a picker D-1 box) are the first segment of its
    // forward list: [fwd, split) from P3, or by binary search in the P6 re-walk (split's
    // LDS is reused by then)
    const int prev = mem[D - 1];
    const int lo = c.S.eb(prev);
    int hi;
    if (FILL) hi = lb16(c.S.dst, lo, c.S.ee(prev), c.pp[D + 1]);
    else hi = c.S.split[prev];
    for (int e = lo; e < hi; ++e) {
      const int h = c.S.dst[e];
      bool ok = true;
#pragma unroll
      for (int q = 0; q < D - 1; ++q) {
        if (!contains16(c.S.dst, c.S.eb(mem[q]), c.S.ee(mem[q]), h)) { ok = false; break; }
      }
      if (!ok) continue;
      mem[D] = h;
      FLevel<K, D + 1, FILL>::run(c, mem);
    }
  }
};
template <int K, bool FILL>
struct FLevel<K, K, FILL> {
  __device__ __forceinline__ static void run(FCtx<K>& c, int (&mem)[K]) {
    if (FILL) {
      const int64_t j = c.out++;
      if (j >= c.c0 && j < c.c1) {
        uint16_t* dstb = c.S.cbuf + (j - c.c0) * K;
#pragma unroll
        for (int i = 0; i < K; ++i) dstb[i] = (uint16_t)mem[i];
        c.cq_ord[j - c.c0] = 0;
      }
    } else {
      // queue the clique (members + ordinal within the root's DFS) while the queue has room;
      // its output index is known once the per-root counts are scanned
      const uint32_t o = (uint32_t)c.count++;
      const uint32_t slot = atomicAdd(c.ccur, 1u);
      if (slot < (uint32_t)c.cq_cap) {
#pragma unroll
        for (int i = 0; i < K; ++i) c.S.cbuf[slot * K + i] = (uint16_t)mem[i];
        c.cq_ord[slot] = (uint16_t)o;
      }
#pragma unroll
      for (int i = 0; i < K; ++i) {
        c.S.flags[mem[i]] = 3;
      }
    }
  }
};

// ----------------------------------------------------------------------------- P4 (BFS)
// Level-synchronous k-clique enumeration (get_cliques.py:49-56 restated for a k-partite
// graph).  Level D holds every D-member prefix (one member per picker 0..D-1, pairwise
// adjacent) in lexicographic order as a tree entry (index of its parent prefix << 16 | last
// member); level 1 is implicit (the picker-0 roots).  Expanding a level: count + 32-bit mask
// of the valid extensions per entry (candidates = first forward segment of the last member,
// kept if every earlier member's list contains them), workgroup scan, write pass.  Level K
// holds the cliques (lexicographic = per-root DFS order), followed by one zeroed flag word
// per clique; the last expansion marks the members.  All levels live in the queue region
// q[0, qbytes); the temps of the level being expanded sit at its top.  Every prefix is one
// thread's work, so a root's subtree no longer serialises on one lane.
template <int K>
struct BfsOut {
  int64_t C;        // cliques, or -1: a level did not fit (caller falls back to the DFS)
  int lvl[K + 1];   // byte offset in q of each level's entries (2..K)
  float fit;        // capacity / demand: of the level that overflowed (C = -1, < 1), else the
                    // smallest over the levels (>= 1)
};
__device__ __forceinline__ float bfs_fit(int64_t need, int64_t have) {
  return need > 0 ? (float)max(have, (int64_t)0) / (float)need : 1.0f;
}

// REWALK (P6 re-run of a root chunk): the split array and the union-find parents are dead by
// then, so first segments come from a binary search for the next picker's first position and
// a root is valid iff it was marked as a clique vertex in P4 (it has a clique, which lies in
// the --get_cc target component); vertices are already marked.
// WE (wide entries, K <= 4, the HBM level-tree slot of the QG launches): an entry holds its
// prefix's members themselves (four u16 in 8 bytes) instead of (parent index, last member), so
// reading a prefix is one load instead of a chain of D - 1 dependent ones (L2 latency each).
template <bool WE>
constexpr int bfs_es() { return WE ? 8 : 4; }
__device__ __forceinline__ uint2 we_pack(const int (&mm)[4], int d, int h) {
  int t[4] = {mm[0], mm[1], mm[2], mm[3]};
  t[d] = h;
  return make_uint2((uint32_t)t[0] | ((uint32_t)t[1] << 16), (uint32_t)t[2] | ((uint32_t)t[3] << 16));
}
// One-trip form: a level (or the root pass) of at most NT entries runs as one staged body per
// thread, count to fill in registers around a one-barrier scan: two barriers per level instead
// of four, no count / mask round trip through LDS.  Levels above NT entries take the general
// count / scan / fill form; both produce the same entry order, so a micrograph may mix them.
// Instances: K <= 3 with up to 768 threads.  The others pay for the second form in registers
// (`make resources`): K = 3 / 1024 and every K = 4 instance drop an
// occupancy step, K = 5 / 768 (f64 layout) grows its scratch and K = 5 / 768 (f32) drops a step,
// and so on up to K = 8; they keep the general form alone.
constexpr bool bfs_one_trip(int k, int nt) { return k <= 3 && nt <= 768; }
// Per-wave slots of the one-trip scans.  Not redi / redu: P3b's stats reduction reads those
// up to the first barrier P4 takes, which is the root pass's scan barrier.  Consecutive
// one-trip scans are separated by the barrier behind the fill (or, on overflow, behind the
// capacity check), so one set of slots serves every level.
__device__ __forceinline__ int* bfs_scan_slots(FusedHdr& H) { return reinterpret_cast<int*>(H.red64); }

template <int K, int D, int NT, bool WE = false>
struct BfsLevel {
  // prefix members of entry e of level D (D members, compile-time indices only)
  __device__ __forceinline__ static void unpack(const uint2 v, int (&mm)[K]) {
    const int t[4] = {(int)(v.x & 0xFFFF), (int)(v.x >> 16), (int)(v.y & 0xFFFF), (int)(v.y >> 16)};
#pragma unroll
    for (int d = 0; d < D && d < 4; ++d) mm[d] = t[d];
  }
  __device__ __forceinline__ static void prefix(const char* q, const int (&lvl)[K + 1],
                                                uint32_t e, int (&mm)[K]) {
    if constexpr (WE) {
      unpack(reinterpret_cast<const uint2*>(q + lvl[D])[e], mm);
      return;
    }
    uint32_t ent = reinterpret_cast<const uint32_t*>(q + lvl[D])[e];
    mm[D - 1] = (int)(ent & 0xFFFF);
    uint32_t cur = ent >> 16;
#pragma unroll
    for (int d = D - 1; d >= 2; --d) {
      ent = reinterpret_cast<const uint32_t*>(q + lvl[d])[cur];
      mm[d - 1] = (int)(ent & 0xFFFF);
      cur = ent >> 16;
    }
    mm[0] = (int)cur;
  }

  template <bool REWALK>
  __device__ __forceinline__ static int seg_end(const FShared& S, const int (&pp)[K + 1], int m) {
    if (REWALK) return lb16(S.dst, S.eb(m), S.ee(m), pp[D + 1]);
    return S.split[m];
  }

  template <bool REWALK, typename EP>
  __device__ __forceinline__ static BfsOut<K> run(const FShared& S, FusedHdr& H, char* q,
                                                  int qbytes, BfsOut<K>& out, int64_t nD, int tid,
                                                  const int (&pp)[K + 1], const EP& ep) {
    int (&lvl)[K + 1] = out.lvl;
    constexpr int ES = bfs_es<WE>();
    // temps of this level at the top of q
    const int tb = (qbytes - 8 * (int)(nD + 1)) & ~7;
    if (K >= 4) {   // (K = 3 runs one attempt: no chunk sizing)
      const float f = fminf(bfs_fit(nD, 65535), bfs_fit((8 + ES) * nD, qbytes - lvl[D] - 8));
      out.fit = fminf(out.fit, f);
    }
    if (nD > 65535 || tb < lvl[D] + ES * (int)nD) {
      out.C = -1;
      out.fit = fminf(out.fit, 0.999f);
      return out;
    }
    constexpr bool last = D + 1 == K;
    const int nb = ufl((lvl[D] + ES * (int)nD + 7) & ~7);   // next level starts here
    // the next level's capacity checks, on its size nN (both forms)
    auto next_fits = [&](int64_t nN) {
      if (K >= 4) {
        const float f = fminf(bfs_fit(nN, 65535), bfs_fit(nN * (last ? ES + 2 : ES), tb - nb));
        out.fit = fminf(out.fit, f);
      }
      if (nN > 65535 || nN * (last ? ES + 2 : ES) > tb - nb) {
        out.C = -1;
        out.fit = fminf(out.fit, 0.999f);
        return false;
      }
      return true;
    };
    // a child of entry e (prefix mm) with last member h at index o of the next level
    auto put = [&](uint32_t e, const int (&mm)[K], int h, uint32_t o, int64_t nN) {
      if constexpr (WE) {
        int m4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int d = 0; d < D && d < 4; ++d) m4[d] = mm[d];
        reinterpret_cast<uint2*>(q + nb)[o] = we_pack(m4, D < 4 ? D : 3, h);
      } else {
        reinterpret_cast<uint32_t*>(q + nb)[o] = (e << 16) | (uint32_t)h;
      }
      if (last) {
        if (!REWALK) {
#pragma unroll
          for (int d = 0; d < K - 1; ++d) S.flags[mm[d]] = 3;
          S.flags[h] = 3;
        }
        reinterpret_cast<uint16_t*>(q + nb + ES * (int)nN)[o] = 0;
      }
    };
    using CT = typename EP::CT;
    constexpr int NC = K > 2 ? K - 2 : 1;
    // Candidate walk of an entry: count and 32-bit mask of the valid extensions among dst[lo, hi),
    // the first segment of its last member's list.  An extension h (picker D) must be adjacent to
    // every earlier member: the graph's edges are exactly the pairs of different pickers with
    // JI > threshold, so instead of a binary search of h in each member's sorted list (three
    // dependent LDS loads each), P2's own test on the two boxes' coordinates decides it (ep.edge: the same
    // function on the same LDS values, so the same answer); the members' coordinates mc stay in
    // registers.
    auto candidates = [&](int lo, int hi, const CT (&mc)[NC], uint32_t& cnt, uint32_t& mask) {
      for (int t = lo; t < hi; ++t) {
        const int h = S.dst[t];
        const CT ch = ep.pt(S, h);
        bool ok = true;
#pragma unroll
        for (int d = 0; d < D - 1; ++d) ok &= ep.edge(mc[d], ch);
        cnt += ok ? 1u : 0u;
        mask |= (ok && t - lo < 32) ? (1u << (t - lo)) : 0u;
      }
    };
    // Fill walk of entry e (prefix mm): its valid extensions, by the mask or past the 32nd
    // candidate by the test again (member d's coordinates from mc(d)), become the next level's
    // entries from index o, in list order.
    auto fill = [&](uint32_t e, const int (&mm)[K], int lo, int hi, uint32_t mask, uint32_t o,
                    int64_t nN, auto&& mc) {
      for (int t = lo; t < hi; ++t) {
        const int h = S.dst[t];
        bool ok;
        if (t - lo < 32) {
          ok = (mask >> (t - lo)) & 1u;
        } else {
          const CT ch = ep.pt(S, h);
          ok = true;
#pragma unroll
          for (int d = 0; d < D - 1; ++d) ok &= ep.edge(mc(d), ch);
        }
        if (!ok) continue;
        put(e, mm, h, o, nN);
        ++o;
      }
    };
    int64_t nN;
    if (bfs_one_trip(K, NT) && nD <= NT) {
      // One trip: thread e holds entry e.  Its count, mask, prefix members and segment bounds
      // stay in registers from the count to the fill; the offsets come from a one-barrier scan
      // (no MK / CN round trip, no second prefix walk; the capacity above still reserves the
      // temps, so the same levels overflow as in the general form).  Same entry order: offset =
      // exclusive prefix in entry order, children in list order.
      int mm[K] = {};
      int lo = 0, hi = 0;
      uint32_t mask = 0, cnt = 0;
      CT mc[NC] = {};
      if (tid < (int)nD) {
        prefix(q, lvl, (uint32_t)tid, mm);
        const int m = mm[D - 1];
        lo = S.eb(m);
        hi = seg_end<REWALK>(S, pp, m);
#pragma unroll
        for (int d = 0; d < D - 1; ++d) mc[d] = ep.pt(S, mm[d]);
        candidates(lo, hi, mc, cnt, mask);
      }
      int tot;
      const uint32_t o = (uint32_t)block_excl_scan_add32<NT>((int)cnt, bfs_scan_slots(H), &tot);
      nN = ufl(tot);
      if (!next_fits(nN)) {
        __syncthreads();   // the scan slots are read: the caller's next attempt may write them
        return out;
      }
      fill((uint32_t)tid, mm, lo, hi, mask, o, nN, [&](int d) { return mc[d]; });
    } else {
      uint32_t* MK = reinterpret_cast<uint32_t*>(q + tb);
      uint32_t* CN = MK + nD;
      for (int e = tid; e < nD; e += NT) {
        int mm[K];
        prefix(q, lvl, (uint32_t)e, mm);
        const int m = mm[D - 1];
        const int lo = S.eb(m), hi = seg_end<REWALK>(S, pp, m);
        uint32_t mask = 0, cnt = 0;
        CT mc[NC];
#pragma unroll
        for (int d = 0; d < D - 1; ++d) mc[d] = ep.pt(S, mm[d]);
        candidates(lo, hi, mc, cnt, mask);
        MK[e] = mask;
        CN[e] = cnt;
      }
      __syncthreads();
      // (32-bit scan: nD <= 65535 entries of at most n <= 4608 extensions each, < 2^31)
      nN = ufl(block_scan_dpp32<NT>(CN, (int)nD, H.redi));
      if (!next_fits(nN)) return out;
      for (int e = tid; e < nD; e += NT) {
        int mm[K];
        prefix(q, lvl, (uint32_t)e, mm);
        const int m = mm[D - 1];
        // (the members' coordinates are not held across this walk: read where a list passes 32
        // candidates, which is rare)
        fill((uint32_t)e, mm, S.eb(m), seg_end<REWALK>(S, pp, m), MK[e], CN[e], nN,
             [&](int d) { return ep.pt(S, mm[d]); });
      }
    }
    __syncthreads();
    lvl[D + 1] = nb;
    if constexpr (D + 1 < K) {
      return BfsLevel<K, D + 1, NT, WE>::template run<REWALK>(S, H, q, qbytes, out, nN, tid, pp, ep);
    } else {
      out.C = nN;
      return out;
    }
  }
};

// Cliques of the roots [r0, r1) (picker-0 positions).  Returns C = -1 when a level does not
// fit the queue region; the caller then retries with fewer roots (root chunks, P4) and falls
// back to the per-root DFS only when a single root does not fit.
template <int K, bool REWALK, int NT, bool WE = false, typename EP>
__device__ __forceinline__ BfsOut<K> bfs_cliques(const FShared& S, FusedHdr& H, char* q,
                                                 int qbytes, int r0, int r1, bool get_cc,
                                                 uint32_t target, int tid,
                                                 const int (&pp)[K + 1], const EP& ep) {
  BfsOut<K> out;
  out.C = -1;
  out.fit = 4.0f;
#pragma unroll
  for (int d = 0; d <= K; ++d) out.lvl[d] = 0;
  const int nr = r1 - r0;
  auto root_ok = [&](int r) {
    if (REWALK) return S.flags[r] == 3;
    return S.eb(r) < S.ee(r) && (!get_cc || S.parent[r] == target);
  };
  auto seg_end = [&](int r) {
    if (REWALK) return lb16(S.dst, S.eb(r), S.ee(r), pp[2]);
    return (int)S.split[r];
  };
  // level 1 -> 2: every root's first segment (picker-1 neighbours), no checks needed
  uint32_t* cnt = S.cnt;
  constexpr bool last = K == 2;
  constexpr int ES = bfs_es<WE>();
  auto level2_fits = [&](int64_t n2) {
    if (K >= 4) out.fit = fminf(bfs_fit(n2, 65535), bfs_fit(n2 * (last ? ES + 2 : ES), qbytes));
    if (n2 > 65535 || n2 * (last ? ES + 2 : ES) > qbytes) {
      out.fit = fminf(out.fit, 0.999f);
      return false;
    }
    return true;
  };
  // the level-2 entries of root r, its first segment dst[lo, hi), from index o
  auto put = [&](int r, int lo, int hi, uint32_t o, int64_t n2) {
    for (int t = lo; t < hi; ++t, ++o) {
      const int h = S.dst[t];
      if constexpr (WE) reinterpret_cast<uint2*>(q)[o] = make_uint2((uint32_t)r | ((uint32_t)h << 16), 0u);
      else reinterpret_cast<uint32_t*>(q)[o] = ((uint32_t)r << 16) | (uint32_t)h;
      if (last) {
        if (!REWALK) {
          S.flags[r] = 3;
          S.flags[h] = 3;
        }
        reinterpret_cast<uint16_t*>(q + ES * (int)n2)[o] = 0;
      }
    }
  };
  int64_t n2;
  if (bfs_one_trip(K, NT) && nr <= NT) {
    // one trip (see bfs_one_trip): thread i holds root r0 + i and its segment bounds; cnt is
    // not written (nothing reads it behind a BFS: the chunk table sits past its n0 entries
    // and the DFS fallback fills it itself)
    const int r = r0 + tid;
    int lo = 0, hi = 0;
    if (tid < nr && root_ok(r)) {
      lo = S.eb(r);
      hi = seg_end(r);
    }
    int tot;
    const uint32_t o = (uint32_t)block_excl_scan_add32<NT>(hi - lo, bfs_scan_slots(H), &tot);
    n2 = ufl(tot);   // (< n^2 < 2^31)
    if (!level2_fits(n2)) {
      __syncthreads();   // the scan slots are read: the caller's next attempt may write them
      return out;
    }
    put(r, lo, hi, o, n2);
  } else {
    for (int i = tid; i < nr; i += NT) {
      const int r = r0 + i;
      cnt[i] = root_ok(r) ? (uint32_t)(seg_end(r) - S.eb(r)) : 0u;
    }
    __syncthreads();
    n2 = ufl(block_scan_dpp32<NT>(cnt, nr, H.redi));   // (< n^2 < 2^31)
    if (!level2_fits(n2)) return out;
    for (int i = tid; i < nr; i += NT) {
      const int r = r0 + i;
      if (!root_ok(r)) continue;
      put(r, S.eb(r), seg_end(r), cnt[i], n2);
    }
  }
  __syncthreads();
  out.lvl[2] = 0;
  if constexpr (K > 2) {
    return BfsLevel<K, 2, NT, WE>::template run<REWALK>(S, H, q, qbytes, out, n2, tid, pp, ep);
  } else {
    out.C = n2;
    return out;
  }
}

// P2: a box with up to FILL_FAST forward edges has its targets packed by the count itself;
// its list is written from them without walking the edge bitmask
constexpr int FILL_FAST = 2;

// Candidates of a box: the 2x3 cell stencil at its cell in the grid of every HIGHER picker
// (forward edges only): columns cx, cx + 1 from cx = its column - 1 or its column (by the
// half of the column the box lies in), rows y0..y1, i.e. up to 2 (K - 1 - p) ranges of
// sorted positions.
struct Stencil {
  int p, cx, y0, y1;   // p = K: no candidates
  double2 a;
};

template <int K, bool W>
__device__ __forceinline__ void stencil_setup(Stencil& st, int ts, const FShared& S,
                                              const GridU& H) {
  const int key = S.scell[ts];
  st.a = ld_xy<W>(S, ts);
  st.p = K;
  st.cx = 0;
  st.y0 = 0;
  st.y1 = -1;
  const int gy = H.gy, nc = H.ncell;
  // (a box of the last picker has no higher picker to search: no candidates either, and its
  // waves skip the decode)
  if (key >= (K - 1) * nc) return;
  // key / ncell and cell / gy through float reciprocals, corrected to the exact quotients
  int p = 0;
#pragma unroll
  for (int q = 1; q < K; ++q) p += (key >= q * nc) ? 1 : 0;
  const int cell = key - p * nc;
  int cx = (int)((float)cell * H.inv_gy);
  cx += ((cx + 1) * gy <= cell) ? 1 : 0;
  cx -= (cx * gy > cell) ? 1 : 0;
  const int cy = cell - cx * gy;
  // half-column test in f32 (0.0014 columns of slack, see P1): left half -> columns cx-1, cx
  // box_key's product: on !W the f32 difference of the two exact f32 values (what the f64
  // difference rounds to), without the f64 subtraction
  const float u = (W ? (float)(st.a.x - H.minx) : (float)st.a.x - (float)H.minx) * H.inv_cellf;
  st.p = p;
  st.cx = cx - ((u - (float)cx) < 0.5f ? 1 : 0);
  st.y0 = max(cy - 1, 0);
  st.y1 = min(cy + 1, gy - 1);
}

// The stencil in picker q's grid as ONE candidate sequence: the position ranges [lo, hi) of its
// two columns st.cx + d (d = 0, 1) joined, so that a box walks a grid in one loop (a wave pays
// the longest lane of the sum, not of each range).  Candidate j (0 <= j < n, stencil order:
// column d = 0, then d = 1, by position) is the box at position j + (j < n0 ? o0 : o1).
// (The second column's offset is kept as its difference d to the first's and added under a
// predicate: a select between two members of a span that is still in memory when the optimiser
// meets it becomes a dynamically indexed load, which moves the spans to scratch.)
struct Span {
  int n0, n, o0, d;
  __device__ __forceinline__ int at(int j) const { return j + o0 + (j >= n0 ? d : 0); }
};

// Position bounds {lo0, hi0, lo1, hi1} of the stencil's two columns in picker q's grid (q < K).
// st.cx lies in [-1, gx - 1]: only the first column can fall left of the grid and only the
// second right of it; such a column reads cell 0 for both of its bounds (empty).  Nothing is
// selected after a load, so the loads of a box's spans are in flight together.
__device__ __forceinline__ void stencil_bounds(const Stencil& st, const FShared& S,
                                               const GridU& H, int q, int (&b)[4]) {
  const int cb = q * H.ncell + st.cx * H.gy;
  const bool ok0 = st.cx >= 0, ok1 = st.cx + 1 < H.gx;
  b[0] = S.cstart[ok0 ? cb + st.y0 : 0];
  b[1] = S.cstart[ok0 ? cb + st.y1 + 1 : 0];
  b[2] = S.cstart[ok1 ? cb + H.gy + st.y0 : 0];
  b[3] = S.cstart[ok1 ? cb + H.gy + st.y1 + 1 : 0];
}
__device__ __forceinline__ Span span_of(const int (&b)[4]) {
  Span g;
  g.n0 = b[1] - b[0];
  g.n = g.n0 + (b[3] - b[2]);
  g.o0 = b[0];
  g.d = b[2] - g.n0 - b[0];
  return g;
}

// The spans of a K = 3 box's (at most two) target grids, all bounds read before any is used.
// Lanes of a wave hold neighbouring boxes of one picker, so the waves of picker 2 skip both
// reads and those of picker 1 the second.
__device__ __forceinline__ void stencil_spans3(const Stencil& st, const FShared& S,
                                               const GridU& H, Span& g0, Span& g1) {
  int b0[4] = {0, 0, 0, 0}, b1[4] = {0, 0, 0, 0};
  if (st.p + 1 < 3) stencil_bounds(st, S, H, st.p + 1, b0);
  if (st.p + 2 < 3) stencil_bounds(st, S, H, st.p + 2, b1);
  g0 = span_of(b0);
  g1 = span_of(b1);
}

// P2 walk of a box's candidates in stencil order (picker, column, position): body(t, kk) with
// the candidate's position t and its ordinal kk.  One flattened loop per target grid (not
// unrolled: a grid's stencil holds a few candidates).  K = 3 leaves its two spans in g0, g1
// for the list write that follows the count.
// first_done() runs once, behind the first target grid (picker st.p + 1), when the box has one:
// the grids are walked in ascending picker order, so the edges counted up to there are the
// first picker segment of the box's list (P4's split).
template <int K, typename F, typename G1>
__device__ __forceinline__ void stencil_walk(const Stencil& st, const FShared& S,
                                             const GridU& H, Span& g0, Span& g1, F&& body,
                                             G1&& first_done) {
  int kk = 0;
  if constexpr (K == 3) {
    stencil_spans3(st, S, H, g0, g1);
#pragma unroll 1
    for (int j = 0; j < g0.n; ++j, ++kk) body(g0.at(j), kk);
    first_done();
#pragma unroll 1
    for (int j = 0; j < g1.n; ++j, ++kk) body(g1.at(j), kk);
  } else {
    for (int q = st.p + 1; q < K; ++q) {
      int b[4];
      stencil_bounds(st, S, H, q, b);
      const Span g = span_of(b);
#pragma unroll 1
      for (int j = 0; j < g.n; ++j, ++kk) body(g.at(j), kk);
      if (q == st.p + 1) first_done();
    }
  }
}

// v_min_f64 / v_max_f64 without the sNaN canonicalisation fmin/fmax carry: grid candidates
// have finite coordinates (non-finite boxes are never in a grid cell), where they equal
// np.min / np.max
__device__ __forceinline__ double min_f64(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double max_f64(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// JI > threshold (get_cliques.py:40-46, 64-65): branch-free overlap in the reference's op
// order, then I > cut, the largest I whose reference quotient does not exceed the threshold
// (JiCut: the reference's decision for every threshold, without the division)
__device__ __forceinline__ bool edge_test(double2 a, double2 b, double B, double cut) {
  double xo = (min_f64(a.x, b.x) + B) - max_f64(a.x, b.x);
  double yo = (min_f64(a.y, b.y) + B) - max_f64(a.y, b.y);
  xo = max_f64(xo, 0.0);
  yo = max_f64(yo, 0.0);
  return xo * yo > cut;
}

// P2's edge decision on two boxes' LDS coordinates (lower picker first), for P4's adjacency
// tests: the integer test of pairs_count_int on the f32 layout, edge_test on the f64 layout
template <bool W>
struct EdgeP {
  using CT = typename std::conditional<W, double2, float2>::type;
  float Bf, Tf;
  double B, cut;
  __device__ __forceinline__ CT pt(const FShared& S, int p) const {
    return reinterpret_cast<const CT*>(S.sxy)[p];
  }
  __device__ __forceinline__ bool edge(CT a, CT b) const {
    if constexpr (W) {
      return edge_test(a, b, B, cut);
    } else {
      const float xo = fmaxf(Bf - fabsf(a.x - b.x), 0.0f);
      const float yo = fmaxf(Bf - fabsf(a.y - b.y), 0.0f);
      return xo * yo > Tf;
    }
  }
};

// P2 count for the box at sorted position ts (thread per box): JI test against every stencil
// candidate of a higher picker; returns the edge count and, for the list write, either the
// targets themselves (at most 2 edges: first << 16 | second, ascending) or the bitmask of edge
// candidates (candidates 0..31 in stencil order; later candidates are re-tested by the write).
// *first_out: the edges into the next picker's grid (every one counted, past candidate 31
// too), i.e. the length of the list's first picker segment.
template <int K, bool W>
__device__ __forceinline__ int pairs_count(const Stencil& st, const FShared& S, const GridU& H,
                                           double B, double cut, float rej, Span& g0, Span& g1,
                                           uint32_t* mask_out,
                                           int* first_out) {
  uint32_t mask = 0, pk = 0;
  int cnt = 0, first = 0;
  // f32 layout: reject in f32 first.  An edge needs |dx| and |dy| < rho B (JiCut); the f32
  // difference of two exact f32 values is within 2^-24 of the true one, so |dx| >= rej =
  // (float)row_min (0.28 % above rho B) as computed can never be an edge.
  const float ax = (float)st.a.x, ay = (float)st.a.y;
  stencil_walk<K>(st, S, H, g0, g1, [&](int t, int kk) {
    bool e;
    if constexpr (W) {
      e = edge_test(st.a, ld_xy<W>(S, t), B, cut);
    } else {
      const float2 bf = reinterpret_cast<const float2*>(S.sxy)[t];
      e = false;
      if (fabsf(ax - bf.x) < rej && fabsf(ay - bf.y) < rej)
        e = edge_test(st.a, make_double2((double)bf.x, (double)bf.y), B, cut);
    }
    if (e) {
      ++cnt;
      mask |= (kk < 32) ? (1u << kk) : 0u;
      pk = (pk << 16) | (uint32_t)t;
    }
  }, [&]() { first = cnt; });
  *mask_out = cnt <= FILL_FAST ? pk : mask;
  *first_out = first;
  return cnt;
}

// P2 count on integer coordinates (f32 layout, see P2): exact f32 overlaps, I > Tf = int_cut
template <int K>
__device__ __forceinline__ int pairs_count_int(const Stencil& st, const FShared& S,
                                               const GridU& H, float Bf, float Tf, Span& g0,
                                               Span& g1, uint32_t* mask_out, int* first_out) {
  uint32_t mask = 0, pk = 0;
  int cnt = 0, first = 0;
  const float ax = (float)st.a.x, ay = (float)st.a.y;
  stencil_walk<K>(st, S, H, g0, g1, [&](int t, int kk) {
    const float2 bf = reinterpret_cast<const float2*>(S.sxy)[t];
    const float xo = fmaxf(Bf - fabsf(ax - bf.x), 0.0f);
    const float yo = fmaxf(Bf - fabsf(ay - bf.y), 0.0f);
    if (xo * yo > Tf) {
      ++cnt;
      mask |= (kk < 32) ? (1u << kk) : 0u;
      pk = (pk << 16) | (uint32_t)t;
    }
  }, [&]() { first = cnt; });
  *mask_out = cnt <= FILL_FAST ? pk : mask;
  *first_out = first;
  return cnt;
}

// P2 list write: the box's forward targets (positions) to d[0..) from the count's bitmask
// (re-testing candidates past the 32nd), right after the count.  Candidates are visited in
// stencil_walk's order (picker, column, position), so the list comes out sorted.  K = 3 (spans
// g0, g1 still held from the count) with at most 32 candidates (every edge has its mask bit):
// one loop over the set bits of the mask; otherwise one loop per target grid (K >= 4 reads the
// grid's bounds again), over the set bits while the grid ends within the mask.
template <int K, bool W>
__device__ __forceinline__ void pairs_fill(const Stencil& st, const FShared& S, const GridU& H,
                                           const Span& g0, const Span& g1, uint32_t mask,
                                           uint16_t* d, double B, double cut) {
  int c = 0, kk = 0;
  auto fill_grid = [&](const Span& g) {
    if (kk + g.n <= 32) {
      uint32_t bits = kk < 32 ? (mask >> kk) : 0u;
      bits &= g.n >= 32 ? ~0u : ((1u << g.n) - 1u);
      while (bits) {
        const int b = __builtin_ctz(bits);
        bits &= bits - 1;
        d[c++] = (uint16_t)g.at(b);
      }
    } else {
      for (int j = 0; j < g.n; ++j) {
        const int idx = kk + j, t = g.at(j);
        const bool e = idx < 32 ? ((mask >> idx) & 1u) != 0
                                : edge_test(st.a, ld_xy<W>(S, t), B, cut);
        if (e) d[c++] = (uint16_t)t;
      }
    }
    kk += g.n;
  };
  if constexpr (K == 3) {
    if (g0.n + g1.n <= 32) {
      // candidate b of the joined sequence g0, g1: one offset and three predicated steps
      const int t1 = g0.n, t2 = g0.n + g1.n0;
      const int d1 = g1.o0 - g0.n - g0.o0 - g0.d;
      while (mask) {
        const int b = __builtin_ctz(mask);
        mask &= mask - 1;
        d[c++] = (uint16_t)(b + g0.o0 + (b >= g0.n0 ? g0.d : 0) + (b >= t1 ? d1 : 0) +
                            (b >= t2 ? g1.d : 0));
      }
    } else {
      fill_grid(g0);
      fill_grid(g1);
    }
  } else {
    for (int q = st.p + 1; q < K; ++q) {
      int b[4];
      stencil_bounds(st, S, H, q, b);
      fill_grid(span_of(b));
    }
  }
}

// per-micrograph results of workgroup thread 0; finished micrographs add their edges to the
// batch total (deferred ones are counted by the pass that finishes them)
__device__ __forceinline__ void put_stats(const FusedArgs& A, int m, int status, int64_t edges,
                                          int nodes, int cc_cnt, int cc_max, int V, int64_t base,
                                          int64_t C, int ties = 0) {
  // entries this workgroup left in the micrograph's tie segment (0: its epilogue did not run)
  A.tie_cnt[m] = ties;
  A.o.status[m] = status;
  A.o.cc_max[m] = cc_max;
  A.o.cc_cnt[m] = cc_cnt;
  A.o.n_nodes[m] = nodes;
  A.o.n_vert[m] = V;
  A.o.n_edges[m] = edges;
  A.o.clique_base[m] = base;
  A.o.clique_cnt[m] = C;
  // a micrograph that needs another pass is counted, so a run's totals alone tell the host
  // (lazy stats); the edges of finished ones are summed after the launch (k_fused_ties).
  // DEFER_WIDE ones are also counted on cursor[5]; with a device-side f64 pass to follow
  // (wide_list) they go to its list and are not a deferral for the host
  if (status == RGC_ST_DEFER_WIDE) {
    const unsigned long long q = atomicAdd(A.cursor + 5, 1ull);
    if (A.wide_list) {
      A.wide_list[q] = m;
      return;
    }
  }
  if (!(status == 0 || status == RGC_ST_NO_CLIQUES || status == RGC_ST_NO_EDGES))
    atomicAdd(A.cursor + 4, 1ull);
}

// Waves per SIMD the register allocator targets.  K = 3 fits 64 VGPRs (4 small spills) for 8
// waves per SIMD = 4 workgroups per CU, which the f32-coordinate LDS layout also allows; larger
// K keep the compiler's choice (their VGPRs, not LDS, bound the occupancy).
constexpr int fused_waves_per_eu(int k, int nt) {
  return nt == 1024 ? 4 : (nt == 768 ? 6 : (nt == 256 ? 8 : (nt == 384 ? 6 : (k <= 3 ? 8 : 1))));
}

// HBM level-tree slots (QG launches): claim a free bit of the slot bitmap (one thread), or -1
// after a bounded search (then the workgroup keeps the LDS queue).  There are twice as many
// slots as workgroups of such a launch can be resident, so the search normally succeeds on
// its first pass; every claimed slot is released by its workgroup before it ends.
// (the two arguments it reads, not the launch's argument block: a reference to that would keep
// a copy of the whole block in scratch wherever this call is not inlined)
__device__ int qg_claim(uint32_t* qg_slots, int qg_nslots) {
  const int nw = qg_nslots >> 5;
  const int w0 = (int)(blockIdx.x % (unsigned)max(nw, 1));
  for (int pass = 0; pass < 4; ++pass) {
    for (int i = 0; i < nw; ++i) {
      const int wd = (w0 + i) % nw;
      uint32_t v = __hip_atomic_load(qg_slots + wd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (int t = 0; t < 32 && v != 0xFFFFFFFFu; ++t) {
        const int b = __builtin_ctz(~v);
        const uint32_t old = atomicOr(qg_slots + wd, 1u << b);
        if (!(old & (1u << b))) return wd * 32 + b;
        v = old | (1u << b);
      }
    }
  }
  return -1;
}

template <int K, bool W, int NT, bool QG>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(fused_waves_per_eu(K, NT))))
void k_fused(FusedArgs A) {
  constexpr int FWG = NT;   // threads of this instance
  constexpr int FNW = NT / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  FusedHdr& H = *reinterpret_cast<FusedHdr*>(smem);
  const FusedLayout L = fused_layout(A.nmax, A.ecap, W);
  FShared S;
  S.sxy = smem + L.off_sxy;
  S.cstart = reinterpret_cast<uint16_t*>(smem + L.off_cstart);
  S.cnt = reinterpret_cast<uint32_t*>(smem + L.off_cnt);
  S.fwd = reinterpret_cast<uint16_t*>(smem + L.off_fwd);
  S.bend = S.fwd + fwd_blocks(A.nmax) * 64;
  S.split = reinterpret_cast<uint16_t*>(smem + L.off_scell);
  S.vscore = reinterpret_cast<double*>(smem + L.off_parent);
  S.vstaged = false;
  S.parent = reinterpret_cast<uint16_t*>(smem + L.off_parent);
  S.citems = reinterpret_cast<uint16_t*>(smem + L.off_citems);
  S.pos = reinterpret_cast<uint16_t*>(smem + L.off_pos);
  S.scell = reinterpret_cast<uint16_t*>(smem + L.off_scell);
  S.vrank = reinterpret_cast<uint16_t*>(smem + L.off_vrank);
  S.flags = reinterpret_cast<uint8_t*>(smem + L.off_flags);
  S.dst = reinterpret_cast<uint16_t*>(smem + L.off_dst);
  S.cbuf = reinterpret_cast<uint16_t*>(smem + L.off_cbuf);
  const int tid = threadIdx.x;
  // (device-side f64 pass: the list's length is known on the device only)
  if (A.mg_count && blockIdx.x >= *A.mg_count) return;
  const int m = A.mg_list ? A.mg_list[blockIdx.x] : (int)blockIdx.x;
  if (blockIdx.x == 0 && tid < 16 && A.cursor_clear) A.cursor_clear[tid] = 0;   // next run's
#ifdef RGC_STAMPS
  // diagnostic build only: per-phase s_memtime stamps of thread 0 (never in the product .so)
#define STAMP(i)                                                                            \
  do {                                                                                      \
    if ((tid & 63) == 0) {                                                                  \
      A.stamps[(int64_t)blockIdx.x * STAMP_SLOTS + 16 + 16 * (i) + (tid >> 6)] =              \
          (i) == 0 ? 0ull : g_bwait[tid >> 6];                                              \
      g_bwait[tid >> 6] = 0;                                                                \
    }                                                                                       \
    raw_barrier();                                                                          \
    if (tid == 0) A.stamps[(int64_t)blockIdx.x * STAMP_SLOTS + (i)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define STAMP(i) \
  do {           \
  } while (0)
#endif
#ifdef RGC_STOP_AFTER
  // ablation build only: stop after phase RGC_STOP_AFTER (outputs incomplete)
#define STOP_AFTER(ph)                            \
  do {                                            \
    if ((ph) == RGC_STOP_AFTER) {                 \
      if (tid == 0) put_stats(A, m, 0, 0, 0, 0, 0, 0, 0, 0); \
      return;                                     \
    }                                             \
  } while (0)
#else
#define STOP_AFTER(ph) \
  do {                 \
  } while (0)
#endif
  STAMP(0);
#ifdef RGC_STAMPS
  // workgroup timeline (s_memrealtime, 100 MHz, chip-wide): start in the low half of slot 13
  const uint32_t rt0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  FCtx<K> c;
  c.B = sdetach(A.B); c.two_b2 = sdetach(A.two_b2); c.flags = sdetach(A.flags);
  c.score = gdetach(A.score);
  c.Bf = uff((float)A.B);
  c.two_b2f = uff((float)A.two_b2);
  c.rows = gdetach(A.rows); c.w = gdetach(A.w); c.conf = gdetach(A.conf);
  c.consensus = gdetach(A.consensus);
  c.members = gdetach(A.members); c.order = gdetach(A.order);
  c.ntie = &H.ntie;
  const gptr<const double> ax = gdetach(A.x);
  const gptr<const double> ay = gdetach(A.y);
  c.S = S;
  c.m = m;
  c.b0 = A.box_off[m * K];
  c.n = A.box_off[m * K + K] - c.b0;
#pragma unroll
  for (int i = 0; i <= K; ++i) c.pb[i] = A.box_off[m * K + i] - c.b0;
  c.idb = A.id_base[m];
  const int n = c.n, b0 = c.b0;

  // ---- P0: load coordinates (the first RB boxes of each thread stay in registers for P1),
  // bounding box (one combined workgroup reduction)
  constexpr int RB = fused_rb(NT);
  constexpr int RQ = fused_rq(NT), RV = fused_rv(NT);
  double rx[RB], ry[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int i = tid + j * FWG;
    rx[j] = i < n ? ax[b0 + i] : 0.0;
    ry[j] = i < n ? ay[b0 + i] : 0.0;
  }
  // fn(i, x, y) for every box of this thread
  auto each_box = [&](auto&& fn) {
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const int i = tid + j * FWG;
      if (i < n) fn(i, rx[j], ry[j]);
    }
    for (int i = tid + RB * FWG; i < n; i += FWG) fn(i, ax[b0 + i], ay[b0 + i]);
  };
  // bounding box on floats for the f32 layout (exact there; a micrograph with inexact
  // coordinates is deferred to the f64 layout, where it is computed in f64)
  using BT = typename std::conditional<W, double, float>::type;
  BT bmnx = INFINITY, bmny = INFINITY, bmxx = -INFINITY, bmxy = -INFINITY;
  // The f32 layout is the INTEGER layout: every finite coordinate an integer below 2^23 and
  // an integer box size 1 <= B <= 2896, so P2's overlaps and P6's overlap products are exact
  // floats (INTP); any other micrograph is deferred to the f64 ("wide") layout, whose kernel
  // carries the f64 arithmetic.  (Real picker BOX files hold integer pixel coordinates.)
  bool inexact = !W && !(A.B >= 1.0 && A.B <= 2896.0 && A.B == floor(A.B));
  each_box([&](int, double xv, double yv) {
    if (isfinite(xv) && isfinite(yv)) {
      bmnx = fmin(bmnx, (BT)xv); bmxx = fmax(bmxx, (BT)xv);
      bmny = fmin(bmny, (BT)yv); bmxy = fmax(bmxy, (BT)yv);
      if (!W)
        inexact |= xv != rint(xv) || yv != rint(yv) || fabs(xv) >= 0x1p23 || fabs(yv) >= 0x1p23;
    }
  });
  if (inexact) bmnx = -INFINITY;   // (impossible otherwise) carried through the min reduction
  // P1's packed bucket counters (the whole cell-start region of the size class), union-find
  // parents, node flags and P2's packed CC-size counters are set up here, so the bounding-box
  // barrier orders them too
  {
    uint32_t* cw = reinterpret_cast<uint32_t*>(S.cstart);
    const int ncw = (fused_cells(A.nmax) + 8) / 2;
    for (int q = tid; q < ncw; q += FWG) cw[q] = 0;
    for (int i = tid; i < n; i += FWG) {
      S.parent[i] = i;
      S.flags[i] = 0;
    }
    uint32_t* ccsz = reinterpret_cast<uint32_t*>(S.vrank);
    for (int q = tid; q < (n + 1) / 2; q += FWG) ccsz[q] = 0;
  }
  {
    BT bv[4] = {bmnx, bmny, -bmxx, -bmxy};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (W) bv[r] = wave_incl_scan(bv[r], [](BT a, BT b) { return fmin(a, b); });
      else bv[r] = wave_incl_min_f32(bv[r]);
    }
    if ((tid & 63) == 63)
#pragma unroll
      for (int r = 0; r < 4; ++r) H.red4[r][tid >> 6] = (double)bv[r];
  }
  STOP_AFTER(0);
  STAMP(1);
  // ---- P1: one grid per picker (x-major cells, K * gx * gy <= 4 nmax + 4 cells in all) and
  // an LDS counting sort of the boxes by (picker, cell).  JI > t implies |dx|, |dy| < rho B,
  // rho = (1 - t) / (1 + t) (t = 0.3: I > (6/13) B^2, (7/13) B = 0.5385 B): with cells >=
  // 2 row_min wide and >= row_min tall (row_min = r B, r >= 1.0028 rho, JiCut; 0.54 B at 0.3)
  // every edge partner lies in the box's own column or the neighbouring column on the side of
  // the box's half of its column (its x is within 0.4986 columns), three rows around its row: a
  // 2x3 stencil, i.e. two contiguous position ranges per grid.  Per-picker grids let a box
  // visit the boxes of higher pickers only.
  // Wave 0 alone reduces the per-wave bounding boxes and plans the grid (wave-uniform work:
  // done by every wave it cost ~8x its VALU); the other waves read the plan from the header
  // after one barrier.  Planned in f32 with hardware reciprocals: exactness is not needed,
  // only cells >= 2 row_min x row_min (0.28 % above what an edge needs, far above f32 rounding;
  // the half-column test has 0.0014 columns of slack), K gx gy within the budget (checked on
  // the integers used), and one inv_cell / inv_celly used by every key.
  __syncthreads();
  if (tid < 64) {
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      v[r] = H.red4[r][0];
#pragma unroll
      for (int w = 1; w < FNW; ++w) v[r] = fmin(v[r], H.red4[r][w]);
    }
    const double mnx = v[0], mny = v[1], mxx = -v[2], mxy = -v[3];
    double cl = A.B, icl = 0.0, icly = 0.0;
    int gx = 0, gy = 0;
    if (mnx <= mxx && A.B > 0.0) {
      const double ex = mxx - mnx, ey = mxy - mny;
      if (!(ex < 0x1p40 && ey < 0x1p40)) {
        cl = INFINITY; gx = 1; gy = 1;
      } else {
        const int budget = (fused_cells(A.nmax) + 4) / K;
        const float fex = (float)ex, fey = (float)ey, rb = __builtin_amdgcn_rcpf((float)budget);
        // row height h, column width 2 h
        float fch = fmaxf((float)A.cut.row_min * 1.000001f,
                          fmaxf(__builtin_sqrtf(0.5f * fex * fey * rb),
                                fmaxf(0.5f * fex, fey) * rb));
        for (;;) {
          const float iry = __builtin_amdgcn_rcpf(fch);
          const int fx = (int)floorf(fex * (0.5f * iry)) + 1, fy = (int)floorf(fey * iry) + 1;
          if (fx <= budget && fy <= budget && fx * fy <= budget) {
            gx = fx; gy = fy;
            break;
          }
          fch *= 1.0625f;
        }
        cl = (double)fch;
        icly = (double)__builtin_amdgcn_rcpf(fch);
        icl = 0.5 * icly;
        // keys use icl / icly: columns must stay >= 2 row_min wide, rows >= row_min tall
        if (icl * (2.0 * A.cut.row_min) > 1.0) icl = 1.0 / (2.0 * A.cut.row_min);
        if (icly * A.cut.row_min > 1.0) icly = 1.0 / A.cut.row_min;
      }
    }
    if (tid == 0) {
      const double ex = mxx - mnx;
      H.minx = mnx; H.miny = mny; H.cell = cl; H.inv_cell = icl; H.inv_celly = icly;
      H.gx = gx; H.gy = gy;
      H.ncell = gx * gy; H.nkey = K * gx * gy;
      H.inv_gy = gy > 0 ? __builtin_amdgcn_rcpf((float)gy) : 0.0f;
      H.xbs = (mnx < mxx && ex < 0x1p60) ? (double)((float)n * __builtin_amdgcn_rcpf((float)ex))
                                         : 0.0;
      // -inf minimum: some coordinate is not an integer below 2^23 (P0), the host relaunches
      // the micrograph with the f64 layout
      H.status = (!W && mnx == -INFINITY) ? RGC_ST_DEFER_WIDE : 0;
      H.C = 0; H.base = 0; H.V = 0; H.ccur = 0; H.ntie = 0; H.E = 0;
      H.tief[0] = H.tief[1] = 0;
      H.qslot = 0;
    }
  }
  __syncthreads();
  if (!W && H.status == RGC_ST_DEFER_WIDE) {
    if (tid == 0) put_stats(A, m, RGC_ST_DEFER_WIDE, 0, 0, 0, 0, 0, 0, 0);
    return;
  }
  const GridU G = grid_u(H);
  const int nk = G.nkey;
  // counting sort by key with packed u16 counters (two keys per LDS word, zeroed in P0).
  // The count's atomic returns: its old value is the box's arrival ordinal within its bucket.
  // Counts go to slot key, so the exclusive scan leaves cstart[q] = start of bucket q for
  // q = 0..nk and the total n in cstart[nk + 1], and nothing advances them afterwards.  Key and
  // ordinal of a register box (the first RB of a thread) stay in one register, key | ordinal
  // << 16 (both < 2^16), from the count to the placement; a box behind them (more than RB * NT
  // boxes) parks its key in pos[i] and its ordinal in citems[i], free until the placement.
  uint32_t* cw = reinterpret_cast<uint32_t*>(S.cstart);
  auto count_box = [&](int i, double xv, double yv) {
    const int q = box_key<W>(G, picker_of<K>(c.pb, i), xv, yv);
    const uint32_t t = atomicAdd(&cw[q >> 1], 1u << (16 * (q & 1)));
    return (uint32_t)q | (((t >> (16 * (q & 1))) & 0xFFFFu) << 16);
  };
  auto park = [&](int i, uint32_t v) {
    S.pos[i] = (uint16_t)(v & 0xFFFFu);
    S.citems[i] = (uint16_t)(v >> 16);
  };
  uint32_t rq[RQ > 0 ? RQ : 1];
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int i = tid + j * FWG;
    if (j < RQ) rq[j] = 0;
    if (i < n) {
      const uint32_t v = count_box(i, rx[j], ry[j]);
      if (j < RQ) rq[j] = v;
      else park(i, v);
    }
  }
  for (int i = tid + RB * FWG; i < n; i += FWG) park(i, count_box(i, ax[b0 + i], ay[b0 + i]));
  __syncthreads();
  block_scan_dpp32<FWG>(S.cstart, nk + 1, H.redi);
  // arrival order into fwd (free until P2): bucket start + ordinal, one load and no atomic;
  // made deterministic by the placement pass
  uint16_t* arrival = S.fwd;
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
    const int i = tid + j * FWG;
    if (i < n) arrival[S.cstart[rq[j] & 0xFFFFu] + (rq[j] >> 16)] = (uint16_t)i;
  }
  for (int i = tid + RQ * FWG; i < n; i += FWG) {
    const int q = S.pos[i], o = S.citems[i];
    arrival[S.cstart[q] + o] = (uint16_t)i;
  }
  __syncthreads();
  // placement: by local index inside each bucket (buckets hold a few boxes).  Written per
  // box, not through each_box: each stage tests i < n on its own and the walk stands outside
  // those tests (a thread without the box walks an empty bucket).  With the whole body under
  // one test the compiler fuses the two bounds into one 32-bit LDS read at a 2-byte-aligned
  // address and the 1024-thread K = 4 instance needs another register.
  // (key(): the register box's key from its register, a later box's from pos[i])
  auto place = [&](int i, auto&& key, auto&& xy) {
    int q = 0, lo = 0, len = 0;
    if (i < n) q = key();
    if (i < n) {
      lo = S.cstart[q];
      len = (int)S.cstart[q + 1] - lo;
    }
    int t = lo;
#pragma nounroll
    for (int u = 0; u < len; ++u) t += (int)arrival[lo + u] < i ? 1 : 0;
    if (i < n) {
      const double2 v = xy();
      S.scell[t] = (uint16_t)q;
      S.citems[t] = (uint16_t)i;
      S.pos[i] = (uint16_t)t;
      st_xy<W>(S, t, v.x, v.y);
    }
  };
#pragma unroll
  for (int j = 0; j < RB; ++j) {
    const int i = tid + j * FWG;
    if (j < RQ) place(i, [&]() { return (int)(rq[j < RQ ? j : 0] & 0xFFFFu); },
                      [&]() { return make_double2(rx[j], ry[j]); });
    else place(i, [&]() { return (int)S.pos[i]; }, [&]() { return make_double2(rx[j], ry[j]); });
  }
  for (int i = tid + RB * FWG; i < n; i += FWG)
    place(i, [&]() { return (int)S.pos[i]; },
          [&]() { return make_double2(ax[b0 + i], ay[b0 + i]); });
  __syncthreads();
  // picker bounds in position space: grid p occupies [pp[p], pp[p+1]); non-finite boxes follow
#pragma unroll
  for (int p = 0; p <= K; ++p) c.pp[p] = ufl(S.cstart[p * G.ncell]);

  STOP_AFTER(1);
  STAMP(2);
  // ---- P2: Jaccard pairs (forward edges to higher pickers): count (JI test, edge bitmask
  // per box) and list write in one pass, lists sorted as written.
  const double B = A.B, two_b2 = A.two_b2;
  // JI > t  <=>  I > cut, the largest f64 I whose reference quotient fl(I / fl(2 B^2 - I))
  // does not exceed t: the quotient is monotone in I, so the host's bisection (JiCut) makes
  // the comparison the reference's decision for every t, without the division.
  // (both taken out of the argument tuple like c.B above: they stay live through P4)
  const double cut = sdetach(A.cut.f64_cut);
  // f32 layout = integer coordinates (|v| < 2^23) and an integer 1 <= B <= 2896: the overlaps B - |dx| and
  // their product (< 2^24) are exact in f32 and JI > t <=> I > int_cut, the same bisection over
  // the integers (t = 0.3: floor(6 B^2 / 13); at I = 6 B^2 / 13 the reference's quotient rounds
  // to 0.3 itself, not above it), so the count pass decides every candidate with six f32
  // operations (pairs_count_int)
  // (the f32 layout is integer-only: P0)
  const float Tf = __int_as_float(sdetach(__float_as_int(A.cut.tf)));
  const EdgeP<W> ep{(float)B, Tf, B, cut};   // (P4's adjacency tests: P2's values)
  // thread per box (sorted position): lanes of a wave hold neighbouring boxes of one picker,
  // so their stencils overlap (similar trip counts, broadcast LDS reads), and the waves of
  // picker K-1 have nothing to do.
  uint32_t* ccsz = reinterpret_cast<uint32_t*>(S.vrank);   // packed u16 CC sizes (P2-P3)
  // One pass per box: a wave-round (one wave, one aligned block of 64 positions) counts its
  // boxes' edges, scans the counts in position order, reserves the block's lists with one LDS
  // atomic on the header's edge cursor and writes every list at once from the targets or the
  // bitmask its lanes still hold (no scan over the workgroup, no second walk of the stencil).
  // Lists of one block are contiguous in position order; blocks lie in arrival order (fwd / bend).
  // A wave-round that would pass ecap writes nothing; the cursor still ends at the true total.
  // The edges' sources for the edge-parallel union are not recorded here: before the total is
  // known they would have to go to a fixed place in dst, where targets of later wave-rounds
  // may land as well; the loop after the barrier writes them behind the E targets.
  // boustrophedon box order: odd rounds walk their FWG positions backwards, so a thread that
  // took a low-picker box (most grids to search) in one round takes a high-picker box (fewest)
  // in the next; K = 3, ~900 boxes: at most 6 instead of 9 column ranges per thread
  {
    for (int r0 = 0, odd = 0; r0 < n; r0 += FWG, odd ^= 1) {
      const int ts = odd ? r0 + FWG - 1 - tid : r0 + tid;
      if (ufl(ts & ~63) >= n) continue;   // (wave-uniform: the block holds no box)
      const bool act = ts < n;
      Stencil st;
      Span g0, g1;
      uint32_t mask = 0;
      int ec = 0, ec1 = 0;   // edges; those to the next picker (the first target grid)
      if (act) {
        stencil_setup<K, W>(st, ts, S, G);
        if constexpr (!W)
          ec = pairs_count_int<K>(st, S, G, (float)B, Tf, g0, g1, &mask, &ec1);
        else ec = pairs_count<K, W>(st, S, G, B, cut, (float)A.cut.row_min, g0, g1, &mask, &ec1);
      }
      const bool top = (ts & 63) == 63;   // the lane that writes the block's end
      // (lanes past the last box store too: fwd[n] is the end of box n - 1's list unless that
      // box closes its block; the slots lie within the fwd_blocks(nmax) * 64 begins)
      // split[ts], the end of the first picker segment of the box's list, is written beside
      // fwd[ts] for every box: begin + ec1 (an empty list or segment: the begin).  split
      // aliases scell, and scell[ts] is read exactly once, by this thread in stencil_setup
      // above, so no other thread can still need the slot.  (Boxes only: scell has n slots.)
      if (__ballot(ec != 0) == 0) {   // (no edge in the block, e.g. the last picker's)
        S.fwd[ts] = 0;
        if (act) S.split[ts] = 0;
        if (top) S.bend[ts >> 6] = 0;
        continue;
      }
      // boxes before this one in the block: lanes below (even rounds) or above (odd rounds)
      const int incl = wave_incl_add32(ec);
      const int total = __builtin_amdgcn_readlane(incl, 63);
      uint32_t rb = 0;
      if ((tid & 63) == 0) rb = (uint32_t)atomicAdd(&H.E, total);
      const int base = ufl((int)rb);
      const int off = base + (odd ? total - incl : incl - ec);
      S.fwd[ts] = (uint16_t)off;
      if (act) S.split[ts] = (uint16_t)(off + ec1);
      if (top) S.bend[ts >> 6] = (uint16_t)(base + total);
      if (base + total > A.ecap || ec == 0) continue;
      uint16_t* d = S.dst + off;
      if (ec <= FILL_FAST) {   // the count kept the targets themselves (ascending)
        d[0] = (uint16_t)(ec == 2 ? mask >> 16 : mask);
        if (ec == 2) d[1] = (uint16_t)mask;
      } else {
        pairs_fill<K, W>(st, S, G, g0, g1, mask, d, B, cut);
      }
      S.flags[ts] = 1;
    }
    __syncthreads();
  }
  const int E = ufl(H.E);
  STAMP(3);   // count + list write (one pass)
  STOP_AFTER(21);

  // the status is the same in every thread
  const int st2 = E == 0 ? RGC_ST_NO_EDGES : (E > A.ecap ? RGC_ST_DEFER : 0);
  if (tid == 0) H.status = st2;
  STAMP(4);   // (the former scan: nothing left but the status)
  STOP_AFTER(22);
  bool cc32 = false;   // the unions ran on u32 parents in cnt
  // QG launches: the workgroup's HBM level-tree slot (claimed here when the edge sources do not
  // fit dst's tail: they go to the slot, dead again by P4, which reuses it for the trees)
  int qslot = -1;
  uint16_t* esrc_g = nullptr;
  if constexpr (QG) {
    if (st2 == 0 && 2 * E > A.ecap && A.qg_base) {
      if (tid == 0) H.qslot = qg_claim(A.qg_slots, A.qg_nslots);
      __syncthreads();
      qslot = ufl(H.qslot);
      if (qslot >= 0) esrc_g = reinterpret_cast<uint16_t*>(A.qg_base + (size_t)qslot * A.qg_bytes);
    }
  }
  if (st2 == 0) {
    // the lists are written (each sorted: position order).  The edges are united one thread
    // per edge (lock-free union-find on u32 parents in cnt, balanced across lanes whatever the
    // degrees), which needs each edge's source: written here from the finished lists, in dst's
    // unused tail when it has room (2 E <= ecap) or in the QG slot in HBM.  With neither: union
    // per box on the u16 parents.
    const bool src_hbm = QG && esrc_g != nullptr;
    const bool src_ok = 2 * E <= A.ecap || src_hbm;
    uint16_t* esrc = S.dst + E;
    // (QG: esrc_g in HBM when dst's tail is short; separate loops keep esrc's LDS accesses
    // ds_* instructions instead of flat ones)
    {
      for (int i = tid; i < n; i += FWG) {
        const int base = S.eb(i);
        const int cnt = S.ee(i) - base;
        if (src_hbm) {
          for (int e = 0; e < cnt; ++e) esrc_g[base + e] = (uint16_t)i;
        } else if (src_ok) {
          for (int e = 0; e < cnt; ++e) esrc[base + e] = (uint16_t)i;
        } else {
          const uint16_t* d = S.dst + base;
          for (int e = 0; e < cnt; ++e) {
            S.flags[d[e]] = 1;
            uf_union_lds(S.parent, (uint32_t)i, (uint32_t)d[e]);
          }
        }
        if (src_ok) S.cnt[i] = (uint32_t)i;
      }
      __syncthreads();
    }
    STAMP(5);   // edge sources (or per-box unions) and identity parents
    STOP_AFTER(23);
    if (src_hbm) {
      // sources from HBM (L2) in batches of 8 loads in flight per thread, then the unions
      constexpr int UB = 8;
      for (int e0 = tid; e0 < E; e0 += UB * FWG) {
        uint32_t sv[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int e = e0 + u * FWG;
          sv[u] = e < E ? esrc_g[e] : 0u;
        }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
          const int e = e0 + u * FWG;
          if (e >= E) break;
          const uint32_t h = S.dst[e];
          S.flags[h] = 1;
          uf_union32(S.cnt, sv[u], h);
        }
      }
      __syncthreads();
    } else if (src_ok) {
      // both endpoints, then both parents, are loaded before the flag store and either find
      for (int e = tid; e < E; e += FWG) {
        const uint32_t a = esrc[e], h = S.dst[e];
        const uint32_t pa = lds_ld(S.cnt + a), ph = lds_ld(S.cnt + h);
        S.flags[h] = 1;
        uf_union32p(S.cnt, a, pa, h, ph);
      }
      __syncthreads();
    }
    cc32 = src_ok;
    if (A.eu) {
      // RGC_F_EDGES test hook: the edge list with the reference's f64 JI (get_cliques.py:40-46)
      if (tid == 0) H.base = (int64_t)atomicAdd(A.cursor + 2, (unsigned long long)E);
      __syncthreads();
      const int64_t eb = H.base;
      if (eb + E <= A.ecap_out) {
        for (int i = tid; i < n; i += FWG) {
          const double2 a = ld_xy<W>(S, i);
          for (int e = S.eb(i), e1 = S.ee(i); e < e1; ++e) {
            const int h = S.dst[e];
            const double2 b = ld_xy<W>(S, h);
            A.eu[eb + e] = b0 + S.citems[i];
            A.ev[eb + e] = b0 + S.citems[h];
            A.eji[eb + e] = jaccard(a.x, a.y, b.x, b.y, B, two_b2);
          }
        }
      }
      __syncthreads();
      if (tid == 0) H.base = 0;
    }
  }
  if (st2 != 0) {
    if (tid == 0) put_stats(A, m, st2, E, 0, 0, 0, 0, 0, 0);
    return;
  }

  STOP_AFTER(2);

  // ---- P3: connected components: the unions ran edge-parallel behind P2's pass (one thread per
  // edge); compress, count sizes
  STAMP(6);   // union (one thread per edge)
  // One loop compresses and takes the stats.  The flag and the parent are loaded together,
  // before the flag is tested (the list split P4 reads came from P2's count).  The size
  // counter's atomic returns: sizes only grow, so the last increment of the largest component
  // returns its final size minus one, and the largest size is the maximum of old + 1 over all
  // increments.  Nodes: the flag is set; roots: the find returned the box itself.
  const bool get_cc = (A.flags & 1) != 0;
  int nodes = 0, cc_max = 0;
  // per-wave partials in redd: no scan of P4 uses it (the one-trip scans red64, the general
  // form redi), so they survive until they are read
  int* const sred = reinterpret_cast<int*>(H.redd);
  {
    // nodes << 16 | roots (both <= n < 2^16) in one 32-bit sum, the largest size in one max;
    // every thread reads the per-wave partials (no thread-0 section and second barrier)
    int nr = 0;
    int mx = 0;
    for (int i = tid; i < n; i += FWG) {
      const int f = S.flags[i];
      uint32_t p = 0;
      if (cc32) p = lds_ld(S.cnt + i);
      if (!f) continue;
      const uint32_t r = cc32 ? uf_find32p(S.cnt, i, p) : uf_find_lds(S.parent, i);
      p16_st(S.parent + i, r);
      const uint32_t old = atomicAdd(&ccsz[r >> 1], 1u << (16 * (r & 1)));
      nr += (1 << 16) + (r == (uint32_t)i ? 1 : 0);
      mx = max(mx, (int)((old >> (16 * (r & 1))) & 0xFFFFu) + 1);
    }
    nr = wave_incl_add32(nr);
    mx = wave_incl_max32(mx);
    if ((tid & 63) == 63) { sred[tid >> 6] = nr; sred[MAXW + (tid >> 6)] = mx; }
  }
  // The finds above walk and compress parent chains through other boxes' entries (cnt, or the
  // u16 parents), so nothing may overwrite an entry while some thread is still in the loop.
  // P4's one-trip root pass writes nothing in front of its scan barrier: it reads fwd / bend,
  // dst and its root's split, all final since P2 (and, with --get_cc, parent behind the
  // barrier below), and the chunk table is first written behind a BFS.  The general root pass
  // and the DFS fallback store per-root counts into cnt, the u32 parents, in front of their
  // first barrier: instances and micrographs that take them keep the barrier here.
  if (!(bfs_one_trip(K, NT) && c.pp[1] <= NT)) __syncthreads();
  auto cc_size = [&](uint32_t r) { return (int)((ccsz[r >> 1] >> (16 * (r & 1))) & 0xFFFF); };
  // the per-wave partials of the stats, once a barrier is behind them
  auto cc_stats = [&]() {
    int t = 0;
    int m2 = 0;
#pragma unroll
    for (int w = 0; w < FNW; ++w) {
      t += sred[w];
      m2 = max(m2, sred[MAXW + w]);
    }
    nodes = t >> 16;
    cc_max = m2;
    if (tid == 0) { H.nodes = nodes; H.cc_cnt = t & 0xFFFF; H.cc_max = cc_max; }
  };
  // --get_cc needs cc_max at once.  Without it the stats are first needed behind P4 (set_order,
  // put_stats): they are summed there, behind the barriers P4 takes anyway (at least one on
  // every path), and this one goes.
  const bool stats_late = !get_cc;
  if (!stats_late) {
    __syncthreads();
    cc_stats();
  }
  // (no barrier: the P4 passes below start with their own before touching the reduction
  // slots, and no array read here is written before it)
  int target = -1;
  if (get_cc) {
    // largest CC; ties -> the component whose first edge comes first in the enumeration
    uint64_t best = ~0ULL;
    for (int i = tid; i < n; i += FWG) {
      const int e0 = S.eb(i), e1 = S.ee(i);
      if (e0 == e1) continue;
      const uint32_t r = S.parent[i];
      if (cc_size(r) != cc_max) continue;
      // the box's first edge in enumeration order: lowest target picker (the first segment
      // of the position-sorted list), smallest file index inside it
      const int pi = picker_of<K>(c.pp, i);
      const int h0 = S.dst[e0];
      const int ph = picker_of<K>(c.pp, h0);
      const int se = lb16(S.dst, e0, e1, picker_end<K>(c.pp, h0));
      int hmin = 1 << 30;
      for (int e = e0; e < se; ++e) hmin = min(hmin, (int)S.citems[S.dst[e]]);
      const uint64_t key = ((uint64_t)pair_index(pi, ph, K) << 48) |
                           ((uint64_t)(S.citems[i] - picker_begin<K>(c.pb, pi)) << 32) |
                           ((uint64_t)(hmin - picker_begin<K>(c.pb, ph)) << 16) | r;
      best = key < best ? key : best;
    }
    // redu is not aliased by red64/redi (only P0's red4 covers it): one barrier
    best = wave_incl_scan(best, [](uint64_t a, uint64_t b) { return a < b ? a : b; });
    if ((tid & 63) == 63) H.redu[tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < FNW; ++w) best = H.redu[w] < best ? H.redu[w] : best;
    target = (int)(best & 0xFFFF);
  }

  STOP_AFTER(3);
  STAMP(7);   // CC stats
  // ---- P4: k-cliques (level-synchronous BFS into the queue region; per-root DFS counts as the
  // fallback when a level does not fit), vertex marking, output reservation
  const int n0 = c.pp[1];   // roots: picker-0 positions
  // queue region: after the E used entries of dst through the cell starts (contiguous: dst
  // immediately precedes the cell starts in the layout)
  const int qoff = (L.off_dst + 2 * H.E + 15) & ~15;
  const int qbytes_lds = L.off_parent - qoff;
  char* q = smem + qoff;
  int qbytes = qbytes_lds;
  if constexpr (QG) {
    // large micrographs: the level trees in an HBM slot (no root chunks to re-walk), the
    // LDS region when no slot is free (P2 may have claimed the slot already for esrc)
    if (qslot < 0) {
      if (tid == 0) H.qslot = A.qg_base ? qg_claim(A.qg_slots, A.qg_nslots) : -1;
      __syncthreads();
      qslot = ufl(H.qslot);
    }
    if (qslot >= 0) {
      q = A.qg_base + (size_t)qslot * (size_t)A.qg_bytes;
      qbytes = A.qg_bytes;
    }
  }
  // wide level-tree entries (members, not parent chains) in the HBM slot
  const bool we = QG && K <= 4 && qslot >= 0;
  // Root chunks: all roots at once when the levels fit the queue region, else consecutive
  // root ranges (halved after a level overflows, doubled after a success).  Chunk i covers
  // roots [rs[i], rs[i+1]) and cliques [cs[i], cs[i+1]) of the micrograph's lexicographic
  // order; the table lives in cnt behind the n0 entries the level-2 counts use.  A chunk's
  // tree is rebuilt in P6 (BFS REWALK), except the last one, still in the queue region.
  uint32_t* const chtab = S.cnt + n0 + 1;
  // (K = 3 keeps one attempt: the rebuild in P6 would push it past its 64-VGPR budget, and
  // its level trees rarely overflow)
  const int maxch = K >= 4 ? min(64, (n + 3 - n0) / 2 - 1) : 1;
  BfsOut<K> bo;
  int nch = 0;
  int64_t C = 0;
  {
    int r0 = 0, len = n0;
    bool ok = maxch >= 1;
    // (chtab[0..1], the table's origin, is written with the first chunk, behind that BFS's
    // barriers: the table lies in cnt, where P3b's finds may still be walking parents)
    while (ok && r0 < n0) {
      len = min(len, n0 - r0);
      if (QG && K <= 4 && qslot >= 0)
        bo = bfs_cliques<K, false, NT, QG && K <= 4>(S, H, q, qbytes, r0, r0 + len, get_cc,
                                                     (uint32_t)target, tid, c.pp, ep);
      else
        bo = bfs_cliques<K, false, NT>(S, H, q, qbytes, r0, r0 + len, get_cc, (uint32_t)target,
                                       tid, c.pp, ep);
      if (bo.C < 0) {
        // shrink to the estimated fit of the overflowing level (demand grows about linearly
        // with the roots), with a small margin; strictly smaller each time
        ok = K >= 4 && len > 1;
        len = max(1, min(len - 1, (int)((float)len * bo.fit * 0.95f)));
        continue;
      }
      if (nch == maxch) { ok = false; break; }
      C += bo.C;
      r0 += len;
      ++nch;
      if (tid == 0) {
        if (nch == 1) { chtab[0] = 0; chtab[1] = 0; }
        chtab[2 * nch] = (uint32_t)r0;
        chtab[2 * nch + 1] = (uint32_t)C;
      }
      // next chunk: as many roots as the tightest level of this one leaves room for
      len = max(len + 1, (int)((float)len * fminf(bo.fit, 2.0f) * 0.95f));
    }
    if (!ok) { nch = 0; C = 0; bo.C = -1; }
  }
  const bool bfs_ok = nch > 0;
  if (bfs_ok) {
    // cliques = level-K tree entries (members by walking parents); their flag words follow
    c.cq_cap = (int)max(bo.C, (int64_t)1);
    c.cq_ord = reinterpret_cast<uint16_t*>(q + bo.lvl[K] + (we ? 8 : 4) * (int)bo.C);
  } else {
    S.cbuf = reinterpret_cast<uint16_t*>(smem + qoff);   // (LDS even when QG)
    c.cq_cap = 0;   // the DFS only counts; P6 re-walks it chunk by chunk
    c.ccur = &H.ccur;
    for (int r = tid; r < n0; r += FWG) {
      uint32_t cntr = 0;
      if (S.eb(r) < S.ee(r) && (!get_cc || S.parent[r] == (uint32_t)target)) {
        int mem[K];
        mem[0] = r;
        c.count = 0;
        FLevel<K, 1, false>::run(c, mem);
        cntr = (uint32_t)c.count;
      }
      S.cnt[r] = cntr;
    }
    __syncthreads();
    C = block_scan_dpp<FWG>(S.cnt, n0, H.red64);
    if (tid == 0) S.cnt[n0] = (uint32_t)C;
    c.cq_cap = qbytes_lds / (2 * K + 2);
    c.cq_ord = S.cbuf + (size_t)c.cq_cap * K;
  }
  c.S.cbuf = S.cbuf;
  if (stats_late) cc_stats();
  c.set_order = 2 * K < nodes;
  STAMP(8);   // cliques
#ifdef RGC_STAMPS
  if (tid == 0) {   // diagnostic build: root chunks of the BFS (0 = DFS fallback) and cliques
    A.stamps[(int64_t)blockIdx.x * STAMP_SLOTS + 14] = (unsigned long long)nch;
    A.stamps[(int64_t)blockIdx.x * STAMP_SLOTS + 15] = (unsigned long long)C;
  }
#endif
  // the output reservation: one returning atomic on the batch cursor per micrograph.  Its
  // result is first needed by P6, so thread 0 only reads it at the end of P5: the round trip
  // (microseconds with every CU's workgroups on the one cursor word) overlaps P5
  unsigned long long resv = 0;
  if (tid == 0) {
    H.C = C;
    if (C == 0) {
      H.status = RGC_ST_NO_CLIQUES;
    } else if (C > 0x7fffffff) {
      H.status = RGC_ST_DEFER;   // P6 indexes a micrograph's cliques in 32 bits
    } else {
      // (a lane-varying zero offset keeps the atomic optimizer's wave-reduction expansion,
      // which consumes the result at once, off this single-lane atomic)
      int vz;
      asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
      resv = atomicAdd(A.cursor + vz, (unsigned long long)C);
    }
  }
  // P5's bucket counters (packed u16 in the dead union-find parents, read for the last time
  // before the barriers of P4's own passes) are zeroed in front of this barrier, so P5 opens
  // without one of its own
  for (int q = tid; q <= (n + 1) / 2; q += FWG) reinterpret_cast<uint32_t*>(S.parent)[q] = 0;
  __syncthreads();

  STOP_AFTER(4);
  STAMP(9);   // scan + reserve
  // ---- P5: row index = rank of each clique vertex by (x, y, id).  Counting sort of the
  // vertices by a fine x bucket (n buckets over the x extent; monotone in x), then rank inside
  // the bucket.  The grid arrays of P1 are dead: parent holds the bucket counters, scell the
  // vertices (sorted positions) in bucket order.
  if (H.status == 0) {
    // bucket counts as packed u16 (two per LDS word; a bucket holds < 2^16 vertices) in the
    // dead union-find parents
    uint16_t* bcnt = S.parent;
    uint32_t* bw = reinterpret_cast<uint32_t*>(S.parent);
    uint16_t* blist = S.scell;
    // f32 layout: coordinates exact as floats, so bucket and (x, y) comparisons run on floats
    // (same order); the bucket map only has to be monotone in x and the same in every pass
    using CT = typename std::conditional<W, double, float>::type;
    using CT2 = typename std::conditional<W, double2, float2>::type;
    auto ld = [&](int t) -> CT2 { return reinterpret_cast<const CT2*>(S.sxy)[t]; };
    const CT minx = (CT)H.minx, xbs = (CT)H.xbs, nlast = (CT)(n - 1);
    auto xbucket = [&](CT xv) { return (int)fmin((xv - minx) * xbs, nlast); };
    // count (flag and x loaded together, before the flag is tested): the atomic returns the
    // vertex's ordinal within its bucket.  Bucket and ordinal of a thread's first RV positions
    // stay in one register across the scan, bucket | ordinal << 16 (NOV: no vertex; a bucket
    // is < n <= 65535, so no vertex packs to it), and the scatter is one load and one store; a
    // position behind them parks its ordinal in vrank and recomputes its bucket.
    constexpr uint32_t NOV = ~0u;
    auto count_vertex = [&](int f, CT x) {
      if (f != 3) return NOV;
      const int q = xbucket(x);
      const uint32_t r = atomicAdd(&bw[q >> 1], 1u << (16 * (q & 1)));
      return (uint32_t)q | (((r >> (16 * (q & 1))) & 0xFFFFu) << 16);
    };
    uint32_t rv[RV > 0 ? RV : 1];
#pragma unroll
    for (int j = 0; j < RV; ++j) {
      const int t = tid + j * FWG;
      int f = 0;
      CT x = 0;
      if (t < n) {
        f = S.flags[t];
        x = ld(t).x;
      }
      rv[j] = count_vertex(f, x);
    }
    for (int t = tid + RV * FWG; t < n; t += FWG) {
      const int f = S.flags[t];
      const CT x = ld(t).x;
      const uint32_t v = count_vertex(f, x);
      if (v != NOV) S.vrank[t] = (uint16_t)(v >> 16);
    }
    __syncthreads();
    const int V = block_scan_dpp32<FWG>(bcnt, n, H.redi);
    if (tid == 0) { H.V = (int)V; bcnt[n] = (uint16_t)V; }
#pragma unroll
    for (int j = 0; j < RV; ++j)
      if (rv[j] != NOV) blist[bcnt[rv[j] & 0xFFFFu] + (rv[j] >> 16)] = (uint16_t)(tid + j * FWG);
    for (int t = tid + RV * FWG; t < n; t += FWG) {
      const int f = S.flags[t];
      const CT x = ld(t).x;
      const int vr = S.vrank[t];
      if (f != 3) continue;
      blist[bcnt[xbucket(x)] + vr] = (uint16_t)t;
    }
    __syncthreads();
    // ranks over the dense bucket-ordered vertex list (every lane holds a vertex; the
    // position loop above skips the non-vertices)
    for (int u0 = tid; u0 < V; u0 += FWG) {
      const int t = blist[u0];
      const int vi = S.citems[t];
      const CT2 v = ld(t);
      const int b = xbucket(v.x);
      const int lo = bcnt[b];
      const int len = (int)bcnt[b + 1] - lo;
      uint32_t rk = lo;
#pragma nounroll
      for (int u = 0; u < len; ++u) {
        const int tu = blist[lo + u];
        const CT2 w = ld(tu);
        const int ui = S.citems[tu];
        rk += (w.x < v.x) || (w.x == v.x && (w.y < v.y || (w.y == v.y && ui < vi)));
      }
      S.vrank[t] = (uint16_t)rk;
    }
    if (tid == 0) H.base = (int64_t)resv;   // (the reservation's round trip ends here)
    __syncthreads();
    // every thread reads the base; an output overflow skips P6 (the host regrows and re-runs)
    const bool overflow = H.base + H.C > A.cap;
    if (overflow && tid == 0) H.status = RGC_ST_OVERFLOW;

    STOP_AFTER(5);
    STAMP(10);  // rank
    if (!overflow) {
    // ---- P6: stage the clique vertices' scores in LDS, then the ILP epilogue + COO rows with
    // one thread per clique (coalesced output stores).  Cliques come from the P4 queue, whose
    // output index is (root's scanned offset + ordinal within the root): the same order as a
    // sequential root-by-root walk.  Micrographs whose cliques overflowed the queue re-walk
    // the DFS per chunk of <= cq_cap cliques.
    // scores of the clique vertices into LDS by row rank when they fit in parent..scell
    c.S.vstaged = 8 * H.V <= L.off_citems - L.off_parent;
    if (c.S.vstaged) {
      // (flag, rank and file index loaded together, before the flag is tested)
      for (int t = tid; t < n; t += FWG) {
        const int f = S.flags[t], vr = S.vrank[t], li = S.citems[t];
        if (f != 3) continue;
        c.S.vscore[vr] = c.score[b0 + li];
      }
      __syncthreads();
    }

    STAMP(11);  // score staging
    // per chunk of queued cliques: main pass (thread per clique).  A set-order micrograph
    // (2 K < nodes: every real one) ends the chunk there: the main pass hands what it cannot
    // decide to k_fused_ties itself.  An insertion-order graph takes a second loop over the
    // cliques the main pass flagged (bit 15 of the slot's ordinal word; the slot's output index
    // is kept in the low bits), behind a barrier and the chunk's H.tief: its f64 order pass.
    // Micrographs whose cliques overflowed the queue re-walk the DFS per chunk of <= cq_cap
    // cliques into the same buffer.
    // chunk bounds and the output base are wave-uniform and 32-bit (C < 2^31, checked at the
    // reservation): they live in SGPRs instead of spilled 64-bit VGPR pairs
    const int Cm = ufl((int)H.C);
    const int cap = ufl(c.cq_cap);
    const int64_t obase = (int64_t)(((uint64_t)(uint32_t)ufl((int)(H.base >> 32)) << 32) |
                                    (uint32_t)ufl((int)H.base));
    // BFS: root chunk by chunk (the last one first: its tree is still in the queue region,
    // the others are rebuilt there); DFS fallback: chunks of <= cap cliques re-walked into cbuf
    const int nit = bfs_ok ? nch : (Cm + cap - 1) / cap;
    BfsOut<K> cur = bo;
    c.tie_seg = gdetach(A.tie_list) + obase * (4 + K);   // (obase + C <= cap = tie_cap)
    const bool second = !c.set_order;   // (workgroup-uniform)
    for (int ci = 0; ci < nit; ++ci) {
      int c0, c1;
      // (last read before the previous chunk's end)
      if (second && tid == 0) H.tief[(ci + 1) & 1] = 0;
      if (bfs_ok) {
        const int ch = ci == 0 ? nch - 1 : ci - 1;
        c0 = ufl((int)chtab[2 * ch + 1]);
        c1 = ufl((int)chtab[2 * ch + 3]);
        if constexpr (K >= 4) {
          if (ci > 0)
            cur = we ? bfs_cliques<K, true, NT, QG && K <= 4>(S, H, q, qbytes, ufl((int)chtab[2 * ch]),
                                       ufl((int)chtab[2 * ch + 2]), get_cc, (uint32_t)target,
                                       tid, c.pp, ep)
                     : bfs_cliques<K, true, NT>(S, H, q, qbytes, ufl((int)chtab[2 * ch]),
                                       ufl((int)chtab[2 * ch + 2]), get_cc, (uint32_t)target,
                                       tid, c.pp, ep);
        }
        c.cq_ord = reinterpret_cast<uint16_t*>(q + cur.lvl[K] + (we ? 8 : 4) * (c1 - c0));
      } else {
        c0 = ci * cap;
        c1 = min(Cm, c0 + cap);
        c.c0 = c0;
        c.c1 = c1;
        for (int r = tid; r < n0; r += FWG) {
          const int64_t lo = S.cnt[r], hi = S.cnt[r + 1];
          if (lo == hi || hi <= c0 || lo >= c1) continue;
          int mem[K];
          mem[0] = r;
          c.out = lo;
          FLevel<K, 1, true>::run(c, mem);
        }
        __syncthreads();
      }
      // members of chunk slot sl: BFS tree walk or the re-walk buffer; the output index of
      // the slot; the order-pass flag of the slot
      auto clique_members = [&](int sl, int (&mem)[K]) -> int64_t {
        if (bfs_ok) {
          if (we) BfsLevel<K, K, NT, QG && K <= 4>::prefix(q, cur.lvl, (uint32_t)sl, mem);
          else BfsLevel<K, K, NT>::prefix(q, cur.lvl, (uint32_t)sl, mem);
        } else {
          const uint16_t* sb = S.cbuf + sl * K;
#pragma unroll
          for (int i = 0; i < K; ++i) mem[i] = sb[i];
        }
        return obase + (c0 + sl);
      };
      auto set_order_flag = [&](int sl) {
        c.cq_ord[sl] |= 0x8000;
      };
      auto order_flag = [&](int sl) -> bool {
        return (c.cq_ord[sl] & 0x8000) != 0;
      };
      bool any = false;
      auto epi = [&](int sl, int (&mem)[K]) {
        const int64_t jo = obase + (c0 + sl);
        bool order;
        if constexpr (!W) order = fused_epilogue_main<K, W, true>(c, jo, mem);
        else order = fused_epilogue_main<K, W, false>(c, jo, mem);
        if (order) {
          set_order_flag(sl);
          any = true;
        }
      };
      if constexpr (QG && K <= 4) {
        if (bfs_ok && we) {
          // wide entries in the HBM slot: the next clique's members are loaded before this
          // one's epilogue runs (an L2 round trip per clique otherwise sits on the chain)
          const uint2* ent = reinterpret_cast<const uint2*>(q + cur.lvl[K]);
          const int cnt = c1 - c0;
          uint2 nx = tid < cnt ? ent[tid] : make_uint2(0u, 0u);
          for (int sl = tid; sl < cnt; sl += FWG) {
            const uint2 v = nx;
            if (sl + FWG < cnt) nx = ent[sl + FWG];
            const int t[4] = {(int)(v.x & 0xFFFF), (int)(v.x >> 16), (int)(v.y & 0xFFFF),
                              (int)(v.y >> 16)};
            int mem[K];
#pragma unroll
            for (int i = 0; i < K; ++i) mem[i] = t[i];
            epi(sl, mem);
          }
        } else {
          for (int sl = tid; sl < c1 - c0; sl += FWG) {
            int mem[K];
            clique_members(sl, mem);
            epi(sl, mem);
          }
        }
      } else {
        for (int sl = tid; sl < c1 - c0; sl += FWG) {
          int mem[K];
          clique_members(sl, mem);
          epi(sl, mem);
        }
      }
      if (second) {
        if (any) H.tief[ci & 1] = 1;
        __syncthreads();
        if (H.tief[ci & 1]) {
          for (int sl = tid; sl < c1 - c0; sl += FWG) {
            if (!order_flag(sl)) continue;
            int mem[K];
            const int64_t jo = clique_members(sl, mem);
            fused_epilogue_order<K, W>(c, jo, mem);
          }
        }
      }
      __syncthreads();
    }
    }   // !overflow
  }
  STAMP(12);
#ifdef RGC_STAMPS
  if (tid == 0)
    A.stamps[(int64_t)blockIdx.x * STAMP_SLOTS + 13] =
        ((unsigned long long)(uint32_t)__builtin_amdgcn_s_memrealtime() << 32) | rt0;
#endif
  if constexpr (QG) {
    if (qslot >= 0) {   // every thread is done with the slot
      __syncthreads();
      if (tid == 0) {
        __threadfence();
        atomicAnd(A.qg_slots + (qslot >> 5), ~(1u << (qslot & 31)));
      }
    }
  }
  if (tid == 0)
    put_stats(A, m, H.status, H.E, H.nodes, H.cc_cnt, H.cc_max, H.V, H.base, H.C, (int)H.ntie);
}

// The cliques the fused launches before it left undecided (fused_tie_handoff): the exact f64
// weighted degrees from the batch coordinates (the reference's JIs, get_cliques.py:182-183),
// the consensus where one member's is the largest, else the first tied member in networkx's
// node order = CPython set order of the (x, y, id) node keys (set(sorted(clique)), pyset.h);
// the --multi_out node order.  Micrograph m's entries are the first tie_cnt[m] slots of the
// tie list from its clique base.  A workgroup takes G consecutive micrographs (one thread each:
// count and base), scans the counts and spreads the (micrograph, entry) pairs over its 256
// threads, so C2's ~3 entries in each of 10k micrographs do not serialise on one lane and C4's
// uneven dozens per micrograph even out; G shrinks with the batch until every workgroup of the
// launch has work.  Each consumed count is cleared: the launch behind a later fused pass, or
// the context's next run, sees only new entries.
template <int K>
__global__ __launch_bounds__(256) void k_fused_ties(FusedArgs A) {
  if (A.esum_n > 0 && blockIdx.x < 16) {
    // edges of the finished micrographs into cursor[1]: 16 workgroups, one atomic each
    __shared__ int64_t red[4];
    int64_t e = 0;
    for (int m = blockIdx.x * 256 + threadIdx.x; m < A.esum_n; m += 16 * 256) {
      const int st = A.o.status[m];
      if (st == 0 || st == RGC_ST_NO_CLIQUES || st == RGC_ST_NO_EDGES) e += A.o.n_edges[m];
    }
    e = block_sum64<256>(e, red);
    if (threadIdx.x == 0 && e) atomicAdd(A.cursor + 1, (unsigned long long)e);
  }
  {
    __shared__ int s_inc[256];
    __shared__ int64_t s_base[256];
    __shared__ int s_wave[4];
    const int tid = threadIdx.x;
    const int G = min(max((A.tie_n + (int)gridDim.x - 1) / (int)gridDim.x, 1), 256);
    const int ngrp = (A.tie_n + G - 1) / G;
    for (int g = (int)blockIdx.x; g < ngrp; g += (int)gridDim.x) {
      const int m = g * G + tid;
      int cnt = 0;
      int64_t base = 0;
      if (tid < G && m < A.tie_n) {
        cnt = A.tie_cnt[m];
        if (cnt > 0) {
          base = A.o.clique_base[m];
          A.tie_cnt[m] = 0;
          // (a segment lies inside the list by construction; never read past it)
          if (cnt > A.o.clique_cnt[m] || base < 0 || base + cnt > A.tie_cap) cnt = 0;
        }
      }
      int inc = wave_incl_scan(cnt, [](int a, int b) { return a + b; });
      __syncthreads();   // the previous trip's reads
      if ((tid & 63) == 63) s_wave[tid >> 6] = inc;
      __syncthreads();
      for (int w = 0; w < (tid >> 6); ++w) inc += s_wave[w];
      s_inc[tid] = inc;
      s_base[tid] = base - (inc - cnt);   // entry index of pair p: s_base + p
      __syncthreads();
      const int total = s_inc[255];
      for (int p = tid; p < total; p += 256) {
        // the pair's micrograph: the first thread whose inclusive count exceeds p
        int lo = 0;
#pragma unroll
        for (int st = 128; st > 0; st >>= 1)
          if (s_inc[lo + st - 1] <= p) lo += st;
        const int32_t* e = A.tie_list + (s_base[lo] + p) * (4 + K);
        const int64_t j = (int64_t)(((uint64_t)(uint32_t)e[1] << 32) | (uint32_t)e[0]);
        const int me = e[2];
        const bool multi = (e[3] & 1) != 0;
        const int64_t idb = A.id_base[me] - (int64_t)A.box_off[me * K];
        int mem[K];
        double xs[K], ys[K], ji[K][K];
        int64_t ids[K];
        const uint64_t ins[K] = {};
#pragma unroll
        for (int i = 0; i < K; ++i) {
          mem[i] = e[4 + i];
          xs[i] = A.x[mem[i]];
          ys[i] = A.y[mem[i]];
          ids[i] = idb + mem[i];
        }
#pragma unroll
        for (int a = 0; a < K; ++a)
#pragma unroll
          for (int b = a + 1; b < K; ++b)
            ji[a][b] = jaccard(xs[a], ys[a], xs[b], ys[b], A.B, A.two_b2);
        uint32_t top;
        int arg = epi_degree_max<K>(ji, &top);
        const bool tie = (top & (top - 1)) != 0;
        if (tie || multi) {
          const uint32_t ord = node_order<K>(mem, xs, ys, ids, true, ins);
          if (tie) arg = epi_tie_arg<K>(top, ord);
          if (multi) {
#pragma unroll
            for (int i = 0; i < K; ++i) A.order[j * K + i] = (uint8_t)((ord >> (4 * i)) & 15);
          }
        }
        int cons = mem[0];
#pragma unroll
        for (int i = 1; i < K; ++i) cons = (arg == i) ? mem[i] : cons;
        A.consensus[j] = cons;
      }
    }
  }
  if (A.host_stats) {
    // the per-micrograph stats to the host, every workgroup a slice (final: the fused launches
    // before this one wrote them; the kernel's end makes the writes visible to the host)
    const int64_t n16 = A.stats_bytes / 16;
    const uint4* src = reinterpret_cast<const uint4*>(A.stats_dev);
    uint4* dst = reinterpret_cast<uint4*>(A.host_stats);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256)
      dst[i] = src[i];
  }
}

int launch_fused_ties(hipStream_t stream, const FusedArgs& A) {
  if (!A.tie_list || !A.tie_cnt || A.tie_cap <= 0) return 0;
  // A workgroup walks its pairs 256 at a time, and a trip costs about what the whole kernel
  // did with one entry per thread (tuple hashing: ~11 us at k = 5), so k >= 4, whose
  // micrographs leave a dozen to dozens of entries each, launches as wide as 1024 workgroups
  // (four micrographs each while the batch allows); k <= 3 (C2: ~3 entries per micrograph)
  // stays at 256, where the wider launch only cost ("Near-ties by clique
  // slot").  RGC_TIES_GRID: a fixed grid, timing experiments only
#ifdef RGC_TIES_GRID
  const int nb = RGC_TIES_GRID;
#else
  const int nb = A.k <= 3 ? 256 : std::min(std::max((A.tie_n + 3) / 4, 256), 1024);
#endif
  const dim3 g(nb), b(256);
  switch (A.k) {
#define RGC_TIES_CASE(KK) \
  case KK: hipLaunchKernelGGL((k_fused_ties<KK>), g, b, 0, stream, A); break;
    RGC_TIES_CASE(2) RGC_TIES_CASE(3) RGC_TIES_CASE(4) RGC_TIES_CASE(5) RGC_TIES_CASE(6)
    RGC_TIES_CASE(7) RGC_TIES_CASE(8)
#undef RGC_TIES_CASE
    default:
      return -1;
  }
  return (int)hipGetLastError();
}

template <int K, bool W, int NT, bool QG = false>
static int launch_fused_t(hipStream_t stream, int n_blocks, int lds_bytes, const FusedArgs& A) {
  static std::atomic<uint64_t> attr_set{0};   // per device
#ifdef RGC_STAMPS
  constexpr int kStaticLds = 256;   // (diagnostic build: g_bwait is static LDS)
#else
  constexpr int kStaticLds = 0;
#endif
  const hipError_t e = set_dyn_lds_once(attr_set, reinterpret_cast<const void*>(&k_fused<K, W, NT, QG>),
                                        160 * 1024 - kStaticLds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((k_fused<K, W, NT, QG>), dim3(n_blocks), dim3(NT), lds_bytes, stream, A);
  return (int)hipGetLastError();
}

template <int K, bool W, int NT, bool QG = false>
static int fused_vgprs_t() {
  hipFuncAttributes at;
  if (hipFuncGetAttributes(&at, reinterpret_cast<const void*>(&k_fused<K, W, NT, QG>)) != hipSuccess)
    return -1;
  return at.numRegs;
}

// workgroup sizes compiled for k (fused_nt_ok) and their dispatch
bool fused_nt_ok(int k, int nt) {
  if (k < 2 || k > 8) return false;
  return nt == 512 || ((nt == 768 || nt == 1024) && k <= 5) ||
         ((nt == 256 || nt == 384) && k <= 3);
}

template <int K, bool W>
static int fused_vgprs_k(int nt) {
  if constexpr (K <= 3) {
    if (nt == 256) return fused_vgprs_t<K, W, 256>();
    if (nt == 384) return fused_vgprs_t<K, W, 384>();
  }
  if constexpr (K <= 5) {
    if (nt == 768) return fused_vgprs_t<K, W, 768>();
    if (nt == 1024) return fused_vgprs_t<K, W, 1024, (K == 4)>();
  }
  return nt == 512 ? fused_vgprs_t<K, W, 512>() : -1;
}

template <int K, bool W>
static int launch_fused_k(hipStream_t stream, int n_blocks, int lds_bytes, const FusedArgs& A,
                          int nt) {
  if constexpr (K <= 3) {
    if (nt == 256) return launch_fused_t<K, W, 256>(stream, n_blocks, lds_bytes, A);
    if (nt == 384) return launch_fused_t<K, W, 384>(stream, n_blocks, lds_bytes, A);
  }
  if constexpr (K <= 5) {
    if (nt == 768) return launch_fused_t<K, W, 768>(stream, n_blocks, lds_bytes, A);
    // 1024 threads (LDS admits one workgroup per CU): K = 4 level trees in HBM slots (K = 5
    // keeps the LDS queue: the flat pointers would push it past 128 VGPRs into scratch)
    if (nt == 1024) return launch_fused_t<K, W, 1024, (K == 4)>(stream, n_blocks, lds_bytes, A);
  }
  return nt == 512 ? launch_fused_t<K, W, 512>(stream, n_blocks, lds_bytes, A) : -1;
}

int fused_vgprs(int k, bool wide, int nt) {
  if (!fused_nt_ok(k, nt)) return -1;
  switch (k) {
#define RGC_VG_CASE(KK) \
  case KK: return wide ? fused_vgprs_k<KK, true>(nt) : fused_vgprs_k<KK, false>(nt);
    RGC_VG_CASE(2) RGC_VG_CASE(3) RGC_VG_CASE(4) RGC_VG_CASE(5) RGC_VG_CASE(6) RGC_VG_CASE(7)
    RGC_VG_CASE(8)
#undef RGC_VG_CASE
    default:
      return -1;
  }
}

int launch_fused(hipStream_t stream, int n_blocks, int lds_bytes, const FusedArgs& A, bool wide,
                 int nt) {
  if (n_blocks <= 0) return 0;
  if (!fused_nt_ok(A.k, nt)) return -1;
  switch (A.k) {
#define RGC_FUSED_CASE(KK)                                                            \
  case KK:                                                                            \
    return wide ? launch_fused_k<KK, true>(stream, n_blocks, lds_bytes, A, nt)        \
                : launch_fused_k<KK, false>(stream, n_blocks, lds_bytes, A, nt);
    RGC_FUSED_CASE(2)
    RGC_FUSED_CASE(3)
    RGC_FUSED_CASE(4)
    RGC_FUSED_CASE(5)
    RGC_FUSED_CASE(6)
    RGC_FUSED_CASE(7)
    RGC_FUSED_CASE(8)
#undef RGC_FUSED_CASE
    default:
      return -1;
  }
  return 0;
}

}  // namespace rgc
