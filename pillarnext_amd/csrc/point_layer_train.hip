// point_layer_train.hip -- one per-point layer of the multi-view reader in TRAINING mode: Linear(bias=False) + BatchNorm1d with batch statistics +
// ReLU [+ the per-cell maximum] (mvf_encoder.py:19-37 PointNet, pillar_encoder.py:35-50 PFNLayer as SingleView stacks it), forward and backward,
// the training twin of pnx_pfn_layer_eval (group.hip).  fp32 throughout, the products on v_mfma_f32_32x32x2_f32 (exact fp32 operands, one
// rounding per product: no bf16 piece anywhere).
//
//   z = x W^T (n, cout)      mean, var = batch statistics of z over the n rows (biased)      xhat = (z - mean) invstd
//   pre = xhat gamma + beta  y = relu(pre)      gmax[g] = max of y over the rows of cell g, argmax[g] = its lowest row (pnx_scatter_max's contract)
//   dz = (dy + dgmax routed to the arg-max row) * (pre > 0)      D1 = sum dz = dbeta      D2 = sum dz xhat = dgamma
//   dxpre = gamma invstd (dz - D1/n - xhat D2/n)      dx = dxpre W      dW = dxpre^T x
//
// No (n, cout) tensor lives between forward and backward: every pass RECOMPUTES z from x and W with the same tile routine, the same k order and
// the same zero padding, so z -- and with it every ReLU gate -- has the same bits in every pass.  Passes (host: pillarnext_amd/ops.py PointLayer):
//   stats           sum z, sum z^2 per channel in fp64 (a product of two fp32 numbers is exact in fp64: what the host subtracts in E[z^2] - E[z]^2
//                   carries no fp32 rounding; tests/pfn_train_ref.py says why fp32 sums cannot meet the masked-BN bars).  Per-workgroup partials,
//                   summed in workgroup order by k_pl_reduce_d into 2 x cout doubles: the small vector the host turns into mean / invstd (and would
//                   all-reduce under SyncBatchNorm; no collective is issued here).
//   forward         y (optional) and / or the per-cell maximum.  The maximum is taken with 64-bit INTEGER atomic max over keys
//                   (bits(y) << 32 | ~row): y >= 0, so its bit pattern orders like the number, and among equal values the lowest row has the largest
//                   key.  A maximum is order-free, so the result does not depend on timing; no floating-point atomic is used.  The key array is the
//                   caller's argmax buffer; k_pl_max_final turns it into gmax / argmax in place (an empty cell: 0 and n).
//   backward_stats  D1, D2 in fp64 the same way.
//   backward        dxpre (n, cout) into the call's workspace (a transient of the backward call), then dx = dxpre W (the same tile routine, B read as
//                   stored) and dW = dxpre^T x: a grid of (cout tile, cin chunk, row split) workgroups, per-split partials summed in split order.
// Determinism: fixed work split (a function of the sizes only), fixed summation orders, integer atomics only; every workspace slot that is read
// has been written by the same call.
//
// Tile routine: a workgroup of 4 waves owns 128 rows x up to 256 columns; wave w rows 32 w .. 32 w + 31, NT <= 8 accumulator tiles of 32 x 32
// (16 registers each).  K runs in chunks of 32 staged through LDS, out-of-range rows / columns / k zero-filled, rows padded to 33 words: the
// operand reads (lane l: row l & 31, k + (l >> 5)) are conflict-free.
// LDS per workgroup: (128 + 256) x 33 x 4 = 50 688 bytes static (A tile 16 896, B tile 33 792); the statistics' cross-wave reduction reuses the B tile.
// No scratch.
#include <type_traits>

#include "pnx_common.h"

namespace {

constexpr int kTM = 128;        // rows of a workgroup tile
constexpr int kKC = 32;         // k per LDS stage
constexpr int kLd = kKC + 1;    // padded LDS row
constexpr int kMaxNT = 8;       // 32-column accumulator tiles per wave
constexpr int kMaxBlocks = 1024;  // workgroups of a row pass (the statistics' partial count)
constexpr int kMaxCin = 576, kMaxCout = 256;
constexpr int kDwBlocks = 768;  // target workgroup count of the dW pass

using f32x16 = __attribute__((ext_vector_type(16))) float;

// acc (128 x NT*32) += A (128 x [k0, k1)) B ([k0, k1) x NT*32)
//   TA = false: A(i, k) = a[i * lda + k]     TA = true: A(i, k) = a[k * lda + i]       i < m_valid, else 0
//   TB = false: B(k, j) = b[j * ldb + k]     TB = true: B(k, j) = b[k * ldb + j]       j < n_valid, else 0
template <int NT, bool TA, bool TB>
__device__ __forceinline__ void gemm_tile(const float* __restrict__ a, int64_t lda, int m_valid, const float* __restrict__ b, int64_t ldb, int n_valid,
                                          int64_t k0, int64_t k1, float* __restrict__ sA, float* __restrict__ sB, f32x16 (&acc)[NT]) {
  const int tid = threadIdx.x, l31 = tid & 31, half = (tid >> 5) & 1, wv = tid >> 6;
  for (int64_t kc = k0; kc < k1; kc += kKC) {
#pragma unroll 4
    for (int e = tid; e < kTM * kKC; e += 256) {
      const int i = TA ? (e & (kTM - 1)) : (e >> 5), k = TA ? (e >> 7) : (e & 31);
      const int64_t kk = kc + k;
      float v = 0.f;
      if (i < m_valid && kk < k1) v = TA ? a[kk * lda + i] : a[(int64_t)i * lda + kk];
      sA[i * kLd + k] = v;
    }
#pragma unroll 4
    for (int e = tid; e < NT * 32 * kKC; e += 256) {
      const int j = TB ? (e % (NT * 32)) : (e >> 5), k = TB ? (e / (NT * 32)) : (e & 31);
      const int64_t kk = kc + k;
      float v = 0.f;
      if (j < n_valid && kk < k1) v = TB ? b[kk * ldb + j] : b[(int64_t)j * ldb + kk];
      sB[j * kLd + k] = v;
    }
    __syncthreads();
    const float* pa = sA + (wv * 32 + l31) * kLd + half;
    const float* pb = sB + l31 * kLd + half;
#pragma unroll
    for (int kk = 0; kk < kKC; kk += 2) {
      const float av = pa[kk];
#pragma unroll
      for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, pb[t * 32 * kLd + kk], acc[t], 0, 0, 0);
    }
    __syncthreads();
  }
}

// row of accumulator register `reg` inside the wave's 32 x 32 tile (lane half h = lane >> 5)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

enum { M_STATS = 0, M_FWD = 1, M_BSTATS = 2, M_BAPPLY = 3 };

struct PlArgs {
  const float* x;
  int64_t ldx, n;
  int cin;
  const float* w;
  int cout;
  const float* prm;  // (6, cout): mean, invstd, gamma, beta, D1 / n, D2 / n
  const int64_t* inv;
  int64_t groups;
  float* y;
  int64_t ldy;
  unsigned long long* keys;
  const float* dy;
  int64_t lddy;
  const float* dgmax;
  const int64_t* argmax;
  float* dxp;
  double* part;  // (gridDim.x, 2, 256)
};

template <int NT, int MODE>
__global__ __launch_bounds__(256) void k_pl_rows(const PlArgs p) {
  __shared__ __align__(16) float smem[(kTM + kMaxNT * 32) * kLd];
  float* sA = smem;
  float* sB = smem + kTM * kLd;
  const int tid = threadIdx.x, l31 = tid & 31, half = (tid >> 5) & 1, wv = tid >> 6;
  const int cout = p.cout;
  float mu[NT], is[NT], ga[NT], be[NT], m1[NT], m2[NT];
  double s1[NT], s2[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int c = t * 32 + l31;
    const bool ok = MODE != M_STATS && c < cout;
    mu[t] = ok ? p.prm[c] : 0.f;
    is[t] = ok ? p.prm[cout + c] : 0.f;
    ga[t] = ok ? p.prm[2 * cout + c] : 0.f;
    be[t] = ok ? p.prm[3 * cout + c] : 0.f;
    m1[t] = ok && MODE == M_BAPPLY ? p.prm[4 * cout + c] : 0.f;
    m2[t] = ok && MODE == M_BAPPLY ? p.prm[5 * cout + c] : 0.f;
    s1[t] = 0.0;
    s2[t] = 0.0;
  }
  const int64_t ntiles = (p.n + kTM - 1) / kTM;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kTM;
    const int m_valid = (int)(p.n - row0 < kTM ? p.n - row0 : kTM);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    gemm_tile<NT, false, false>(p.x + row0 * p.ldx, p.ldx, m_valid, p.w, p.cin, cout, 0, p.cin, sA, sB, acc);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int64_t row = row0 + wv * 32 + acc_row(r, half);
      const bool rok = row < p.n;
      int64_t cell = -1;
      if (MODE != M_STATS && p.inv != nullptr && rok) {
        cell = p.inv[row];
        if (cell < 0 || cell >= p.groups) cell = -1;
      }
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int c = t * 32 + l31;
        const float z = acc[t][r];
        if (MODE == M_STATS) {  // rows >= n and columns >= cout are exact zeros
          const double zd = (double)z;
          s1[t] += zd;
          s2[t] = __builtin_fma(zd, zd, s2[t]);
          continue;
        }
        const float xh = (z - mu[t]) * is[t];
        const float pre = __builtin_fmaf(xh, ga[t], be[t]);
        const bool ok = rok && c < cout;
        if (MODE == M_FWD) {
          const float yv = pre > 0.f ? pre : 0.f;
          if (ok && p.y != nullptr) p.y[row * p.ldy + c] = yv;
          if (ok && p.keys != nullptr && cell >= 0) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(yv) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)row);
            unsigned long long* k = p.keys + cell * cout + c;
            if (*k < key) atomicMax(k, key);  // keys only grow: a stale read can only let a needless atomic through
          }
        } else {
          float dz = 0.f;
          if (ok) {
            if (p.dy != nullptr) dz = p.dy[row * p.lddy + c];
            if (p.dgmax != nullptr && cell >= 0 && p.argmax[cell * cout + c] == row) dz += p.dgmax[cell * cout + c];
            dz = pre > 0.f ? dz : 0.f;
          }
          if (MODE == M_BSTATS) {
            const double dd = (double)dz;
            s1[t] += dd;
            s2[t] = __builtin_fma(dd, (double)xh, s2[t]);
          } else if (ok) {
            p.dxp[row * cout + c] = (ga[t] * is[t]) * ((dz - m1[t]) - xh * m2[t]);
          }
        }
      }
    }
  }
  if (MODE == M_STATS || MODE == M_BSTATS) {
    double* red = reinterpret_cast<double*>(sB);  // [4 waves][2][NT * 32]; every wave has passed the tile routine's last barrier
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const double a = s1[t] + __shfl_xor(s1[t], 32), b = s2[t] + __shfl_xor(s2[t], 32);
      if (half == 0) {
        red[(wv * 2 + 0) * (NT * 32) + t * 32 + l31] = a;
        red[(wv * 2 + 1) * (NT * 32) + t * 32 + l31] = b;
      }
    }
    __syncthreads();
    for (int e = tid; e < 2 * NT * 32; e += 256) {
      const int q = e / (NT * 32), c = e % (NT * 32);
      const double v = ((red[(0 * 2 + q) * (NT * 32) + c] + red[(1 * 2 + q) * (NT * 32) + c]) + red[(2 * 2 + q) * (NT * 32) + c]) + red[(3 * 2 + q) * (NT * 32) + c];
      p.part[((int64_t)blockIdx.x * 2 + q) * 256 + c] = v;
    }
  }
}

// sums[q * cout + c] = the partials of the nblk workgroups in workgroup order
__global__ __launch_bounds__(256) void k_pl_reduce_d(const double* __restrict__ part, int nblk, int cout, double* __restrict__ sums) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * cout) return;
  const int q = e / cout, c = e % cout;
  double s = 0.0;
  for (int b = 0; b < nblk; b++) s += part[((int64_t)b * 2 + q) * 256 + c];
  sums[e] = s;
}

// keys -> gmax / argmax, in place (argmax IS the key array)
__global__ __launch_bounds__(256) void k_pl_max_final(unsigned long long* __restrict__ keys, int64_t total, int64_t n, float* __restrict__ gmax) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const unsigned long long k = keys[i];
  gmax[i] = k == 0ull ? 0.f : __uint_as_float((uint32_t)(k >> 32));
  reinterpret_cast<int64_t*>(keys)[i] = k == 0ull ? n : (int64_t)(0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull));
}

// dx (n, lddx) = dxp (n, cout) W (cout, cin): blockIdx.x walks the row tiles, blockIdx.y the chunks of NT * 32 input columns
template <int NT>
__global__ __launch_bounds__(256) void k_pl_dx(const float* __restrict__ dxp, const float* __restrict__ w, int64_t n, int cin, int cout, float* __restrict__ dx,
                                               int64_t lddx) {
  __shared__ __align__(16) float smem[(kTM + kMaxNT * 32) * kLd];
  const int tid = threadIdx.x, l31 = tid & 31, half = (tid >> 5) & 1, wv = tid >> 6;
  const int j0 = blockIdx.y * NT * 32;
  const int n_valid = cin - j0 < NT * 32 ? cin - j0 : NT * 32;
  const int64_t ntiles = (n + kTM - 1) / kTM;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = tile * kTM;
    const int m_valid = (int)(n - row0 < kTM ? n - row0 : kTM);
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
    gemm_tile<NT, false, true>(dxp + row0 * cout, cout, m_valid, w + j0, cin, n_valid, 0, cout, smem, smem + kTM * kLd, acc);
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int64_t row = row0 + wv * 32 + acc_row(r, half);
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int j = t * 32 + l31;
        if (row < n && j < n_valid) dx[row * lddx + j0 + j] = acc[t][r];
      }
    }
  }
}

// dW partials: part[s][c][j] = sum over the rows of split s of dxp[row][c] x[row][j]; blockIdx = (cout tile of 128, cin chunk of NT * 32, split)
template <int NT>
__global__ __launch_bounds__(256) void k_pl_dw(const float* __restrict__ dxp, const float* __restrict__ x, int64_t ldx, int64_t n, int cin, int cout,
                                               int64_t rows_per_split, float* __restrict__ part) {
  __shared__ __align__(16) float smem[(kTM + kMaxNT * 32) * kLd];
  const int tid = threadIdx.x, l31 = tid & 31, half = (tid >> 5) & 1, wv = tid >> 6;
  const int c0 = blockIdx.x * kTM, j0 = blockIdx.y * NT * 32;
  const int m_valid = cout - c0 < kTM ? cout - c0 : kTM;
  const int n_valid = cin - j0 < NT * 32 ? cin - j0 : NT * 32;
  const int64_t k0 = (int64_t)blockIdx.z * rows_per_split;
  int64_t k1 = k0 + rows_per_split;
  if (k1 > n) k1 = n;
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
  gemm_tile<NT, true, true>(dxp + c0, cout, m_valid, x + j0, ldx, n_valid, k0, k1, smem, smem + kTM * kLd, acc);
  float* o = part + (int64_t)blockIdx.z * cout * cin;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int c = c0 + wv * 32 + acc_row(r, half);
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const int j = t * 32 + l31;
      if (c < cout && j < n_valid) o[(int64_t)c * cin + j0 + j] = acc[t][r];
    }
  }
}

__global__ __launch_bounds__(256) void k_pl_reduce_f(const float* __restrict__ part, int splits, int64_t total, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  double s = 0.0;
  for (int k = 0; k < splits; k++) s += (double)part[(int64_t)k * total + i];
  out[i] = (float)s;
}

// accumulator tiles per wave for `cols` columns in `chunks` equal chunks: 1, 2, 4, 6 or 8
int nt_for(int cols, int& chunks) {
  const int tiles = (cols + 31) / 32;
  chunks = (tiles + kMaxNT - 1) / kMaxNT;
  const int per = (tiles + chunks - 1) / chunks;
  const int nt = per <= 1 ? 1 : per <= 2 ? 2 : per <= 4 ? 4 : per <= 6 ? 6 : 8;
  chunks = (tiles + nt - 1) / nt;
  return nt;
}

template <typename F>
int with_nt(int nt, F&& f) {
  switch (nt) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

int row_blocks(int64_t n) {
  const int64_t t = (n + kTM - 1) / kTM;
  return (int)(t < kMaxBlocks ? (t < 1 ? 1 : t) : kMaxBlocks);
}

struct DwSplit {
  int mt, chunks, nt, splits;
  int64_t rows;
};
DwSplit dw_split(int64_t n, int cin, int cout) {
  DwSplit d;
  d.mt = (cout + kTM - 1) / kTM;
  d.nt = nt_for(cin, d.chunks);
  int64_t s = kDwBlocks / (d.mt * d.chunks);
  const int64_t most = (n + kKC - 1) / kKC;
  if (s > most) s = most;
  if (s < 1) s = 1;
  d.rows = ((n + s - 1) / s + kKC - 1) / kKC * kKC;
  if (d.rows < kKC) d.rows = kKC;
  d.splits = (int)((n + d.rows - 1) / d.rows);
  if (d.splits < 1) d.splits = 1;
  return d;
}

struct PlWs {
  double* part;
  float *dxp, *dwpart;
  size_t bytes;
};
PlWs pl_carve(void* ws, int64_t n, int cin, int cout, bool backward) {
  PlWs w;
  PnxCarver c(ws);
  w.part = c.take<double>((size_t)kMaxBlocks * 2 * 256);
  w.dxp = w.dwpart = nullptr;
  if (backward) {
    w.dxp = c.take<float>((size_t)n * cout + 64);
    w.dwpart = c.take<float>((size_t)dw_split(n, cin, cout).splits * cout * cin + 64);
  }
  w.bytes = c.used();
  return w;
}

// what every entry point checks before any HIP call
int pl_check(const char* who, const float* x, int64_t ldx, int64_t n, int cin, const float* w, int cout) {
  PNX_REQUIRE(n >= 0 && cin >= 1 && cout >= 1, PNX_ERR_INVALID, "%s: bad sizes n=%lld cin=%d cout=%d", who, (long long)n, cin, cout);
  PNX_REQUIRE(cin <= kMaxCin && cout <= kMaxCout, PNX_ERR_UNSUPPORTED, "%s: %d -> %d channels (at most %d -> %d)", who, cin, cout, kMaxCin, kMaxCout);
  PNX_REQUIRE(n < ((int64_t)1 << 31) - kTM, PNX_ERR_UNSUPPORTED, "%s: more than 2^31 rows", who);
  PNX_REQUIRE(ldx >= cin, PNX_ERR_INVALID, "%s: ldx %lld < cin %d", who, (long long)ldx, cin);
  PNX_REQUIRE(w != nullptr && (n == 0 || x != nullptr), PNX_ERR_INVALID, "%s: null pointer (x / W)", who);
  return PNX_OK;
}

template <int MODE>
int launch_rows(const PlArgs& a, int blocks, hipStream_t st) {
  int chunks = 1;
  const int nt = nt_for(a.cout, chunks);
  return with_nt(nt, [&](auto t) -> int {
    k_pl_rows<decltype(t)::value, MODE><<<blocks, 256, 0, st>>>(a);
    PNX_LAUNCH_CHECK();
    return PNX_OK;
  });
}

// the upstream gradient's arguments, shared by the two backward entry points
int grad_check(const char* who, int64_t n, int cout, const float* dy, int64_t lddy, const int64_t* inv, int64_t groups, const float* dgmax, const int64_t* argmax) {
  PNX_REQUIRE(dy != nullptr || dgmax != nullptr, PNX_ERR_INVALID, "%s: neither dy nor dgmax given", who);
  PNX_REQUIRE(dy == nullptr || lddy >= cout, PNX_ERR_INVALID, "%s: lddy %lld < cout %d", who, (long long)lddy, cout);
  PNX_REQUIRE(dgmax == nullptr || (groups >= 0 && argmax != nullptr && (n == 0 || inv != nullptr)), PNX_ERR_INVALID, "%s: dgmax needs inv, argmax and num_groups >= 0", who);
  return PNX_OK;
}

}  // namespace

extern "C" {

size_t pnx_point_layer_workspace_bytes(int64_t n, int32_t cin, int32_t cout, int32_t backward) {
  if (n < 0 || n >= ((int64_t)1 << 31) - kTM || cin < 1 || cin > kMaxCin || cout < 1 || cout > kMaxCout) return 0;
  return pl_carve(nullptr, n, cin, cout, backward != 0).bytes;
}

int pnx_point_layer_stats(const float* x, int32_t ldx, int64_t n, int32_t cin, const float* w, int32_t cout, double* sums, void* workspace,
                          size_t workspace_bytes, pnx_stream_t stream) {
  const char* who = "pnx_point_layer_stats";
  if (int rc = pl_check(who, x, ldx, n, cin, w, cout)) return rc;
  PNX_REQUIRE(sums != nullptr, PNX_ERR_INVALID, "%s: null pointer (sums)", who);
  const PlWs ws = pl_carve(workspace, n, cin, cout, false);
  PNX_CHECK_WORKSPACE(workspace, workspace_bytes, ws.bytes, who);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    PNX_CHECK_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 2 * cout, st));
    return PNX_OK;
  }
  PlArgs a = {};
  a.x = x, a.ldx = ldx, a.n = n, a.cin = cin, a.w = w, a.cout = cout, a.part = ws.part;
  const int blocks = row_blocks(n);
  if (int rc = launch_rows<M_STATS>(a, blocks, st)) return rc;
  k_pl_reduce_d<<<(2 * cout + 255) / 256, 256, 0, st>>>(ws.part, blocks, cout, sums);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_point_layer_forward(const float* x, int32_t ldx, int64_t n, int32_t cin, const float* w, int32_t cout, const float* prm, const int64_t* inv,
                            int64_t num_groups, float* y, int32_t ldy, float* gmax, int64_t* argmax, pnx_stream_t stream) {
  const char* who = "pnx_point_layer_forward";
  if (int rc = pl_check(who, x, ldx, n, cin, w, cout)) return rc;
  PNX_REQUIRE(y != nullptr || gmax != nullptr, PNX_ERR_INVALID, "%s: neither y nor gmax requested", who);
  PNX_REQUIRE(prm != nullptr, PNX_ERR_INVALID, "%s: null pointer (prm)", who);
  PNX_REQUIRE(y == nullptr || ldy >= cout, PNX_ERR_INVALID, "%s: ldy %d < cout %d", who, ldy, cout);
  PNX_REQUIRE(gmax == nullptr || (num_groups >= 0 && argmax != nullptr && (n == 0 || inv != nullptr)), PNX_ERR_INVALID,
              "%s: gmax needs inv, argmax and num_groups >= 0", who);
  PNX_REQUIRE(gmax == nullptr || num_groups < ((int64_t)1 << 31), PNX_ERR_UNSUPPORTED, "%s: more than 2^31 cells", who);
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = gmax ? num_groups * cout : 0;
  if (total > 0) PNX_CHECK_HIP(hipMemsetAsync(argmax, 0, sizeof(int64_t) * (size_t)total, st));
  if (n > 0) {
    PlArgs a = {};
    a.x = x, a.ldx = ldx, a.n = n, a.cin = cin, a.w = w, a.cout = cout, a.prm = prm, a.y = y, a.ldy = ldy;
    if (total > 0) a.inv = inv, a.groups = num_groups, a.keys = reinterpret_cast<unsigned long long*>(argmax);
    if (int rc = launch_rows<M_FWD>(a, row_blocks(n), st)) return rc;
  }
  if (total > 0) {
    k_pl_max_final<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(reinterpret_cast<unsigned long long*>(argmax), total, n, gmax);
    PNX_LAUNCH_CHECK();
  }
  return PNX_OK;
}

int pnx_point_layer_backward_stats(const float* x, int32_t ldx, int64_t n, int32_t cin, const float* w, int32_t cout, const float* prm, const float* dy,
                                   int32_t lddy, const int64_t* inv, int64_t num_groups, const float* dgmax, const int64_t* argmax, double* sums,
                                   void* workspace, size_t workspace_bytes, pnx_stream_t stream) {
  const char* who = "pnx_point_layer_backward_stats";
  if (int rc = pl_check(who, x, ldx, n, cin, w, cout)) return rc;
  if (int rc = grad_check(who, n, cout, dy, lddy, inv, num_groups, dgmax, argmax)) return rc;
  PNX_REQUIRE(prm != nullptr && sums != nullptr, PNX_ERR_INVALID, "%s: null pointer (prm / sums)", who);
  const PlWs ws = pl_carve(workspace, n, cin, cout, false);
  PNX_CHECK_WORKSPACE(workspace, workspace_bytes, ws.bytes, who);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    PNX_CHECK_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 2 * cout, st));
    return PNX_OK;
  }
  PlArgs a = {};
  a.x = x, a.ldx = ldx, a.n = n, a.cin = cin, a.w = w, a.cout = cout, a.prm = prm, a.dy = dy, a.lddy = lddy, a.part = ws.part;
  if (dgmax) a.inv = inv, a.groups = num_groups, a.dgmax = dgmax, a.argmax = argmax;
  const int blocks = row_blocks(n);
  if (int rc = launch_rows<M_BSTATS>(a, blocks, st)) return rc;
  k_pl_reduce_d<<<(2 * cout + 255) / 256, 256, 0, st>>>(ws.part, blocks, cout, sums);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_point_layer_backward(const float* x, int32_t ldx, int64_t n, int32_t cin, const float* w, int32_t cout, const float* prm, const float* dy,
                             int32_t lddy, const int64_t* inv, int64_t num_groups, const float* dgmax, const int64_t* argmax, float* dx, int32_t lddx,
                             float* dw, void* workspace, size_t workspace_bytes, pnx_stream_t stream) {
  const char* who = "pnx_point_layer_backward";
  if (int rc = pl_check(who, x, ldx, n, cin, w, cout)) return rc;
  if (int rc = grad_check(who, n, cout, dy, lddy, inv, num_groups, dgmax, argmax)) return rc;
  PNX_REQUIRE(prm != nullptr && dw != nullptr, PNX_ERR_INVALID, "%s: null pointer (prm / dw)", who);
  PNX_REQUIRE(dx == nullptr || lddx >= cin, PNX_ERR_INVALID, "%s: lddx %d < cin %d", who, lddx, cin);
  const PlWs ws = pl_carve(workspace, n, cin, cout, true);
  PNX_CHECK_WORKSPACE(workspace, workspace_bytes, ws.bytes, who);
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    PNX_CHECK_HIP(hipMemsetAsync(dw, 0, sizeof(float) * (size_t)cout * cin, st));
    return PNX_OK;
  }
  PlArgs a = {};
  a.x = x, a.ldx = ldx, a.n = n, a.cin = cin, a.w = w, a.cout = cout, a.prm = prm, a.dy = dy, a.lddy = lddy, a.dxp = ws.dxp;
  if (dgmax) a.inv = inv, a.groups = num_groups, a.dgmax = dgmax, a.argmax = argmax;
  const int blocks = row_blocks(n);
  if (int rc = launch_rows<M_BAPPLY>(a, blocks, st)) return rc;
  if (dx != nullptr) {
    int chunks = 1;
    const int nt = nt_for(cin, chunks);
    const int rc = with_nt(nt, [&](auto t) -> int {
      k_pl_dx<decltype(t)::value><<<dim3(blocks, chunks), 256, 0, st>>>(ws.dxp, w, n, cin, cout, dx, lddx);
      PNX_LAUNCH_CHECK();
      return PNX_OK;
    });
    if (rc) return rc;
  }
  const DwSplit d = dw_split(n, cin, cout);
  const int rc = with_nt(d.nt, [&](auto t) -> int {
    k_pl_dw<decltype(t)::value><<<dim3(d.mt, d.chunks, d.splits), 256, 0, st>>>(ws.dxp, x, ldx, n, cin, cout, d.rows, ws.dwpart);
    PNX_LAUNCH_CHECK();
    return PNX_OK;
  });
  if (rc) return rc;
  const int64_t total = (int64_t)cout * cin;
  k_pl_reduce_f<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(ws.dwpart, d.splits, total, dw);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

}  // extern "C"
