// Host-side plumbing every engine's create / destroy path shares: the checkpoint's weight table, the list of device allocations a handle owns,
// the fp32 -> 16-bit conversions of the weight packers, the "on error, free the half-built handle" macro, and what every batch engine's per-call host path
// shares: the config-size refusal, the workspace cursor, the finiteness scan, the per-call table upload and the lazy upload of a handle's tables.
// Nothing here is on a hot path.
#pragma once
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "common.h"

// In a create function, between `new` and `*out = handle`: every fallible call goes through this, so that nothing returns past `fail`
// (a callable taking the error code, freeing what the handle owns and returning the code).
#define ETD_TRY_OR(fail, x)                  \
  do {                                       \
    const int _rc = (x);                     \
    if (_rc != ETD_OK) return fail(_rc);     \
  } while (0)
// a HIP call as an error code (HIP_TRY's message), for ETD_TRY_OR
#define ETD_HIP_RC(x) etd_hip_rc((x), #x, __FILE__, __LINE__)
inline int etd_hip_rc(hipError_t e, const char* what, const char* file, int line) {
  if (e == hipSuccess) return ETD_OK;
  char b[512];
  snprintf(b, sizeof(b), "%s:%d %s -> %s", file, line, what, hipGetErrorString(e));
  g_etd_err = b;
  return ETD_EHIP;
}

// name -> (host pointer, element count) of a checkpoint, as the C ABI passes it
struct WeightTable {
  std::map<std::string, std::pair<const float*, int64_t>> t;
  int null_name = -1;                      // index of the first null entry of `names` (skipped), or -1
  WeightTable(const char* const* names, const float* const* host_ptrs, const int64_t* numels, int n) {
    for (int i = 0; i < n; ++i) {
      if (names[i]) t[names[i]] = {host_ptrs[i], numels[i]};
      else if (null_name < 0) null_name = i;
    }
  }
  // the tensor `k` of exactly `numel` elements, or null with g_etd_err set
  const float* get(const std::string& k, int64_t numel) const {
    auto it = t.find(k);
    if (it == t.end()) { g_etd_err = "missing weight '" + k + "'"; return nullptr; }
    if (it->second.second != numel || !it->second.first) {
      g_etd_err = "weight '" + k + "' has " + std::to_string(it->second.second) + " elements, expected " + std::to_string(numel);
      return nullptr;
    }
    return it->second.first;
  }
};

// every device allocation a handle owns, in allocation order; each carries 256 bytes of slack (kernels read whole vectors / tiles at the end of a buffer)
struct DevPool {
  std::vector<void*> ptrs;
  std::vector<size_t> bytes;               // parallel to ptrs, slack included
  template <typename T> int alloc(T** p, size_t n, bool zero = false) {
    void* q = nullptr;
    const size_t nb = n * sizeof(T) + 256;
    HIP_TRY(hipMalloc(&q, nb));
    ptrs.push_back(q); bytes.push_back(nb);
    if (zero) HIP_TRY(hipMemset(q, 0, nb));
    *p = (T*)q;
    return ETD_OK;
  }
  // allocate + copy n elements from the host (S: the host-side type of the same size, e.g. uint16_t bits of a 16-bit float)
  template <typename T, typename S> int upload(T** dst, const S* src, size_t n) {
    static_assert(sizeof(T) == sizeof(S), "upload: element sizes differ");
    ETD_TRY(alloc(dst, n));
    HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return ETD_OK;
  }
  size_t mark() const { return ptrs.size(); }
  void free_from(size_t m) {               // the allocations made since mark() returned m
    for (size_t i = m; i < ptrs.size(); ++i) (void)hipFree(ptrs[i]);
    ptrs.resize(m); bytes.resize(m);
  }
  void free_all() { free_from(0); }
  // Lazy tables: an engine whose create needs no GPU keeps its tables on the host and every run starts with upload_once(body).  `body` (-> error code) allocates
  // from this pool and runs once; if it fails, what it allocated is freed and the next run tries again.
  bool uploaded = false;
  template <typename F> int upload_once(F body) {
    if (uploaded) return ETD_OK;
    const size_t m0 = mark();
    const int rc = body();
    if (rc != ETD_OK) free_from(m0);
    uploaded = rc == ETD_OK;
    return rc;
  }
  // ... and its destroy: nothing to do for a handle that never ran
  void release_uploaded() {
    if (!uploaded) return;
    (void)hipDeviceSynchronize();          // kernels of this handle may still be in flight
    free_all();
  }
};

// A config struct leads with struct_bytes = the caller's sizeof: any other layout is refused (`who`: the create function's name in the message)
#define ETD_CHECK_CFG(cfg, type, who)                                                                                                                   \
  do {                                                                                                                                                  \
    if ((cfg)->struct_bytes != (int)sizeof(type))                                                                                                       \
      ETD_FAIL(ETD_EINVAL, who ": " #type " is %d bytes here, the caller's is %d -- caller built against another etude_hip.h", (int)sizeof(type), (cfg)->struct_bytes); \
  } while (0)

// Per-call workspaces: every piece starts on a multiple of 256 bytes
inline long long ws_align(long long bytes) { return (bytes + 255) & ~255LL; }
struct WsCursor {
  long long off = 0;                       // the next piece's offset; at the end, the bytes the pieces need
  long long take(long long bytes) { const long long o = off; off += ws_align(bytes); return o; }
};

// A handle's per-call workspace: grown when a call needs more than it holds, never shrunk, 256 bytes of slack like the pool's allocations.  A call that grows it
// waits for its stream first (earlier calls on it may still read the old block).
struct Workspace {
  char* p = nullptr;
  long long bytes = 0;
  int reserve(long long need, hipStream_t st) {
    if (need <= bytes) return ETD_OK;
    HIP_TRY(hipStreamSynchronize(st));
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    HIP_TRY(hipMalloc((void**)&p, (size_t)need + 256));
    bytes = need;
    return ETD_OK;
  }
  void release() {                         // a handle's destroy
    if (!p) return;
    (void)hipDeviceSynchronize();          // kernels of this handle may still be in flight
    (void)hipFree(p);
    p = nullptr; bytes = 0;
  }
};

template <typename T> bool finite_all(const T* p, size_t n) {      // T: float or double
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// A per-call host table to the device on the call's stream.  The wait is the call's one synchronisation: `v` is host memory of this call and must outlive the copy.
template <typename T> int upload_table(hipStream_t st, void* dst, const std::vector<T>& v) {
  HIP_TRY(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  HIP_TRY(hipStreamSynchronize(st));
  return ETD_OK;
}

// fp32 -> 16-bit operand bits, round to nearest even, NaN kept
inline uint16_t f32_to_bf16_bits(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
inline uint16_t f32_to_f16_bits(float f) { const _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }
