// rgc_ctx.cpp — the context of the C ABI (include/repic_gc.h): one per device / stream, with
// a grow-only device and pinned-host arena and the timing events; the per-thread error
// message; the small entry points that only read the context.
#include <algorithm>
#include <cstring>

#include "pyset.h"
#include "rgc_host.h"

using namespace rgc;

static thread_local std::string g_err;

int fail(const std::string& msg) {
  g_err = msg;
  return -1;
}

int ensure_dev(rgc_ctx* c, int id, size_t bytes, size_t keep) {
  Buf& b = c->d[id];
  if (bytes == 0) bytes = 16;
  if (b.cap >= bytes) return 0;
  size_t cap = std::max(bytes, b.cap + b.cap / 2);
  cap = (cap + 255) & ~(size_t)255;
  void* p = nullptr;
  HIPCHK(hipMalloc(&p, cap));
  if (b.p && keep) {
    HIPCHK(hipMemcpyAsync(p, b.p, std::min(keep, b.cap), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  if (b.p) HIPCHK(hipFree(b.p));
  b.p = p;
  b.cap = cap;
  // the scan tile buffer: word 0 is the one-pass scan's claim counter (every scan leaves it
  // zero), the rest per-tile states tagged with a launch epoch; a new buffer starts all zero
  // (no state of a reused allocation can match a later epoch)
  if (id == D_TILES) {
    HIPCHK(hipMemsetAsync(p, 0, cap, c->stream));
    c->tiles_epoch = scan_epoch_count();
  }
  // the per-micrograph tie counts: zero wherever no fused workgroup has written since the last
  // ties launch, so a new buffer starts all zero
  if (id == D_TIECNT) HIPCHK(hipMemsetAsync(p, 0, cap, c->stream));
  return 0;
}

// Before a run that scans: launch epochs repeat after 2^22 - 1 scans process-wide, so a tile
// buffer whose states may date from SCAN_EPOCH_REFRESH scans ago is zeroed first.
int tiles_refresh(rgc_ctx* c) {
  Buf& b = c->d[D_TILES];
  if (!b.p || scan_epoch_count() - c->tiles_epoch < SCAN_EPOCH_REFRESH) return 0;
  HIPCHK(hipMemsetAsync(b.p, 0, b.cap, c->stream));
  c->tiles_epoch = scan_epoch_count();
  return 0;
}

int ensure_host(rgc_ctx* c, int id, size_t bytes) {
  Buf& b = c->h[id];
  if (bytes == 0) bytes = 16;
  if (b.cap >= bytes) return 0;
  if (b.p) HIPCHK(hipHostFree(b.p));
  size_t cap = std::max(bytes, b.cap + b.cap / 2);
  b.p = nullptr;
  b.cap = 0;
  HIPCHK(hipHostMalloc(&b.p, cap, hipHostMallocDefault));
  b.cap = cap;
  return 0;
}

int mark(rgc_ctx* c, const char* name) {
  if (!c->timing) return 0;
  if (c->n_ev >= (int)c->events.size()) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    c->events.push_back(e);
    c->ev_names.push_back(nullptr);
  }
  c->ev_names[c->n_ev] = name;
  HIPCHK(hipEventRecord(c->events[c->n_ev], c->stream));
  ++c->n_ev;
  return 0;
}

// Grow the per-clique output arrays to `need` cliques, keeping the first `keep` cliques.
int ensure_outputs(rgc_ctx* c, int64_t need, int64_t keep, int k, bool members, bool multi) {
  TRY(ensure_dev(c, D_ROWS, need * k * 4, keep * k * 4));
  TRY(ensure_dev(c, D_W, need * 4, keep * 4));
  TRY(ensure_dev(c, D_CONF, need * 4, keep * 4));
  TRY(ensure_dev(c, D_CONS, need * 4, keep * 4));
  TRY(ensure_dev(c, D_TIES, need * (4 + k) * 4));   // <= one entry per clique
  if (members) TRY(ensure_dev(c, D_MEMBERS, need * k * 4, keep * k * 4));
  if (multi) TRY(ensure_dev(c, D_ORDER, need * k, keep * k));
  return 0;
}

// Grow the RGC_F_EDGES dump arrays to `need` edges, keeping the first `keep`.
int ensure_edges(rgc_ctx* c, int64_t need, int64_t keep) {
  TRY(ensure_dev(c, D_EU, need * 4, keep * 4));
  TRY(ensure_dev(c, D_EV, need * 4, keep * 4));
  TRY(ensure_dev(c, D_EJIOUT, need * 8, keep * 8));
  return 0;
}

int collect_times(rgc_ctx* c, bool keep, bool tail) {
  if (!c->timing) return 0;
  if (!keep) {
    c->times.clear();
    c->time_names.clear();
  }
  for (int i = 0; i + 1 < c->n_ev || (tail && i < c->n_ev); ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, c->events[i], i + 1 < c->n_ev ? c->events[i + 1] : c->ev_tail));
    c->times.push_back(ms);
    c->time_names.push_back(c->ev_names[i]);
  }
  return 0;
}

int section_time(rgc_ctx* c, hipEvent_t e0, hipEvent_t e1, const char* name) {
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  c->times.push_back(ms);
  c->time_names.push_back(name);
  return 0;
}

extern "C" {

int rgc_abi_version(void) { return RGC_ABI_VERSION; }

const char* rgc_last_error(void) { return g_err.c_str(); }

int rgc_test_ji_cutoff(int64_t box_size, double t, int64_t* int_cut, double* f64_lo,
                       double* f64_hi) {
  if (!int_cut || !f64_lo || !f64_hi) return fail("null argument");
  if (box_size < 1 || box_size > (1LL << 26)) return fail("box_size must be in 1..2^26");
  if (!(t >= 0.0 && t < 1.0)) return fail("ji_threshold must be finite and in [0, 1)");
  const rgc::JiCut c = rgc::ji_cut(box_size, t);
  *int_cut = c.int_cut;
  *f64_lo = *f64_hi = c.f64_cut;
  return 0;
}

int rgc_device_count(int* n) {
  HIPCHK(hipGetDeviceCount(n));
  return 0;
}

int rgc_ctx_set_copy_stream(rgc_ctx* c, void* hip_stream) {
  if (!c) return fail("null context");
  if (c->pend) return fail("rgc_ctx_set_copy_stream: a submitted run awaits rgc_wait");
  if (c->copy_set) HIPCHK(hipStreamSynchronize(c->copy_stream));
  c->copy_stream = reinterpret_cast<hipStream_t>(hip_stream);
  c->copy_set = true;
  return 0;
}

int rgc_ctx_create(int device, void* hip_stream, rgc_ctx** out) {
  *out = nullptr;
  HIPCHK(hipSetDevice(device));
  rgc_ctx* c = new rgc_ctx();
  c->device = device;
  if (hip_stream) {
    c->stream = reinterpret_cast<hipStream_t>(hip_stream);
  } else {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      return fail(std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    c->own_stream = true;
  }
  *out = c;
  return 0;
}

void rgc_ctx_destroy(rgc_ctx* c) {
  if (!c) return;
  if (c->worker.joinable()) c->worker.join();
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& b : c->d)
    if (b.p) (void)hipFree(b.p);
  for (auto& b : c->h)
    if (b.p) (void)hipHostFree(b.p);
  for (auto e : c->events) (void)hipEventDestroy(e);
  if (c->ev_tail) (void)hipEventDestroy(c->ev_tail);
  if (c->ev_sub) (void)hipEventDestroy(c->ev_sub);
  if (c->ev_k) (void)hipEventDestroy(c->ev_k);
  if (c->copy_set) (void)hipStreamSynchronize(c->copy_stream);   // (not owned: never destroyed)
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// ABI 7: the host buffers the last run's outputs point into, handed to the caller
struct rgc_host_block {
  std::vector<void*> bufs;
};

int rgc_detach_host(rgc_ctx* c, void** block) {
  if (!c || !block) return fail("null argument");
  *block = nullptr;
  if (c->pend) return fail("rgc_detach_host: a submitted run awaits rgc_wait on this context");
  HIPCHK(hipSetDevice(c->device));
  TRY(rgc_fetch_stats(c));   // a lazy run's per-micrograph block lands in the detached buffer
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->copy_set) HIPCHK(hipStreamSynchronize(c->copy_stream));
  rgc_host_block* b = new rgc_host_block();
  for (auto& h : c->h) {
    if (h.p) b->bufs.push_back(h.p);
    h.p = nullptr;   // the next run allocates fresh pinned buffers
    h.cap = 0;
  }
  c->n_edge_dump = 0;
  *block = b;
  return 0;
}

void rgc_host_block_free(void* block) {
  rgc_host_block* b = static_cast<rgc_host_block*>(block);
  if (!b) return;
  for (void* p : b->bufs) (void)hipHostFree(p);
  delete b;
}

int rgc_kernel_times(rgc_ctx* c, int max_n, float* ms, const char** names) {
  if (!c) return fail("null ctx");
  const int n = std::min<int>(max_n, (int)c->times.size());
  for (int i = 0; i < n; ++i) {
    if (ms) ms[i] = c->times[i];
    if (names) names[i] = c->time_names[i];
  }
  return (int)c->times.size();
}

int64_t rgc_last_edges(rgc_ctx* c, const int32_t** u, const int32_t** v, const double** ji) {
  if (!c) return fail("null ctx");
  if (u) *u = H<int32_t>(c, H_EU);
  if (v) *v = H<int32_t>(c, H_EV);
  if (ji) *ji = H<double>(c, H_EJIOUT);
  return c->n_edge_dump;
}

uint64_t rgc_py_hash_node(double x, double y, int64_t id) { return pyset::hash_node(x, y, id); }

#ifdef RGC_STAMPS
// Diagnostic build only: s_memtime stamps (8 per fused workgroup, launch order) of the
// last rgc_run.
int64_t rgc_diag_stamps(rgc_ctx* c, uint64_t* out, int64_t max_n) {
  const int64_t n = std::min<int64_t>(max_n, (int64_t)c->stamps.size());
  if (out) std::memcpy(out, c->stamps.data(), n * 8);
  return (int64_t)c->stamps.size();
}
#endif

int rgc_py_set_order(const uint64_t* hashes, int n, int8_t* out) {
  if (n < 0 || n > 18) return fail("set_order supports 0..18 keys");
  if (n >= 1 && n <= 8) {   // the register-packed variant the device epilogue uses
    uint32_t p = 0;
    switch (n) {
#define RGC_SO(NN)                                  \
  case NN: {                                        \
    uint64_t h[NN];                                 \
    for (int i = 0; i < NN; ++i) h[i] = hashes[i];  \
    p = pyset::set_order_packed<NN>(h);             \
    break;                                          \
  }
      RGC_SO(1) RGC_SO(2) RGC_SO(3) RGC_SO(4) RGC_SO(5) RGC_SO(6) RGC_SO(7) RGC_SO(8)
#undef RGC_SO
    }
    for (int i = 0; i < n; ++i) out[i] = (int8_t)((p >> (4 * i)) & 15);
    return n;
  }
  return pyset::set_order(hashes, n, out);
}

}  // extern "C"
