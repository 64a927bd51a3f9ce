// pnx_common.h -- shared declarations for the gfx950 kernels behind include/pnx.h
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>
#include <mutex>

#include "../../include/pnx.h"

void pnx_set_error(const char* fmt, ...);

#define PNX_CHECK_HIP(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      pnx_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return PNX_ERR_HIP;                                                                \
    }                                                                                    \
  } while (0)

#define PNX_REQUIRE(cond, code, ...) \
  do {                               \
    if (!(cond)) {                   \
      pnx_set_error(__VA_ARGS__);    \
      return (code);                 \
    }                                \
  } while (0)

#define PNX_LAUNCH_CHECK()                                                         \
  do {                                                                             \
    hipError_t _e = hipGetLastError();                                             \
    if (_e != hipSuccess) {                                                        \
      pnx_set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(_e), __FILE__, __LINE__); \
      return PNX_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

// The opt-in a kernel needs before a launch may ask for more than 64 KiB of dynamic LDS: raises the limit of `Kernel` on the current
// device to at least `bytes`.  The HIP runtime keeps the attribute per kernel and per device, so the largest size granted so far is
// remembered the same way: one table per kernel (= per instantiation of this template), one slot per device.  Once a size is granted
// a call costs hipGetDevice and one atomic load; the slow path is serialised, so two host threads can neither skip the attribute nor
// lower it behind each other's back.
constexpr int kPnxMaxDevices = 16;
inline std::mutex g_pnx_lds_mutex;
template <auto Kernel>
int pnx_lds_optin(size_t bytes) {
  static std::atomic<size_t> granted[kPnxMaxDevices];
  int dev = 0;
  PNX_CHECK_HIP(hipGetDevice(&dev));
  PNX_REQUIRE(dev >= 0 && dev < kPnxMaxDevices, PNX_ERR_UNSUPPORTED, "device index %d", dev);
  if (bytes <= granted[dev].load(std::memory_order_acquire)) return PNX_OK;
  std::lock_guard<std::mutex> lock(g_pnx_lds_mutex);
  if (bytes > granted[dev].load(std::memory_order_relaxed)) {
    PNX_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    granted[dev].store(bytes, std::memory_order_release);
  }
  return PNX_OK;
}

// The bf16 pieces of one operand of the training convolutions, most significant first (host side only).  NP = 1: the bf16 operand itself;
// 2: (hi, lo) of pnx_split_f32; 3: (hi, mid, lo) of pnx_split3_f32.  A constructor with another number of pointers than NP does not compile.
// The piece-to-slot mapping of the kernels is stated HERE and nowhere else.  k_conv3x3_pc, k_conv3x3_s2 and k_dgrad_s2 take their pieces
// positionally: the first slot (x, wfrag, g, wt) is hi, the second (x2, wfrag2, g2, wt2) is slot2() = lo for NP 2 but MID for NP 3, and the
// trailing third (x3, wfrag3, g3, wt3) is slot3() = lo for NP 3, null otherwise.  k_wgrad64 takes them by name (x_lo, dy_lo, x_mid, dy_mid).
template <int NP>
struct PnxPieces {
  static_assert(NP >= 1 && NP <= 3, "1, 2 or 3 pieces");
  const void *hi, *mid = nullptr, *lo = nullptr;
  PnxPieces(const void* h) : hi(h) { static_assert(NP == 1, "one pointer: NP = 1"); }
  PnxPieces(const void* h, const void* l) : hi(h), lo(l) { static_assert(NP == 2, "(hi, lo): NP = 2"); }
  PnxPieces(const void* h, const void* m, const void* l) : hi(h), mid(m), lo(l) { static_assert(NP == 3, "(hi, mid, lo): NP = 3"); }
  const void* slot2() const { return NP == 2 ? lo : mid; }
  const void* slot3() const { return NP == 3 ? lo : nullptr; }
  bool complete() const { return hi && (NP < 2 || lo) && (NP < 3 || mid); }
  uintptr_t bits() const { return (uintptr_t)hi | (uintptr_t)mid | (uintptr_t)lo; }  // for alignment checks
};

static inline size_t pnx_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over the caller's workspace.
struct PnxCarver {
  char* base;
  size_t off;
  explicit PnxCarver(void* p) : base((char*)p), off(0) {}
  template <typename T>
  T* take(size_t count) {
    off = pnx_align_up(off, 256);
    T* r = (T*)(base ? base + off : nullptr);
#ifdef PNX_CARVE_PROBE  // tools/carve_check.cpp, host sanitizers: write the first and the last element of every field
    if (base && count) r[0] = T(), r[count - 1] = T();
#endif
    off += count * sizeof(T);
    return r;
  }
  size_t used() const { return pnx_align_up(off, 256); }
};

// The one check in front of every carve (include/pnx.h: the workspace contract).  PnxCarver aligns offsets, not addresses: the base has to be aligned.
inline int pnx_check_workspace(const void* workspace, size_t workspace_bytes, size_t need, const char* entry) {
  PNX_REQUIRE(workspace != nullptr, PNX_ERR_INVALID, "%s: workspace is NULL (%zu bytes needed)", entry, need);
  PNX_REQUIRE(workspace_bytes >= need, PNX_ERR_WORKSPACE, "%s: workspace too small (%zu < %zu bytes)", entry, workspace_bytes, need);
  PNX_REQUIRE(((uintptr_t)workspace & 255) == 0, PNX_ERR_INVALID, "%s: workspace must be 256-byte aligned (%zu bytes given, %zu needed)", entry,
              workspace_bytes, need);
  return PNX_OK;
}
#define PNX_CHECK_WORKSPACE(workspace, workspace_bytes, need, entry)                             \
  do {                                                                                           \
    if (int _rc = pnx_check_workspace((workspace), (workspace_bytes), (need), (entry))) return _rc; \
  } while (0)

// Device-side copy of pnx_geom plus the padded row length of the occupancy bitmap.
struct PnxGeomDev {
  float minx, miny, minz, vx, vy, vz;
  int gx, gy, gyp;  // gyp = gy rounded up to a multiple of 32 (one bitmap word = 32 consecutive yi of one xi)
  int B;
};

// Two-level exclusive scan granularity: one 256-thread block scans 2048 items.
#define PNX_SCAN_ITEMS 2048
#define PNX_SCAN_SHIFT 11

// fp16x3 layer 1 of pfn_v3.hip: power-of-two pre-scales of the layer-0 output (2^SU) and of W1' (2^SW) that keep the fp16 hi/lo
// parts in the normal range; the product scale 2^-(SU+SW) is applied (exactly) in the epilogue.
#define PNX_PFN_SU 6
#define PNX_PFN_SW 8
