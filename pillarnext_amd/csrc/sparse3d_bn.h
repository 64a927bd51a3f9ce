// sparse3d_bn.h -- train-mode BatchNorm1d + residual + ReLU over the (n, C) fp32 rows of an active set, forward and backward (included by
// sparse3d.hip after sparse3d_half.h, whose Sp3Half it uses).  The rows are what pnx_sp3_conv_train and pnx_sp3_conv_h_f32 write: unpadded,
// C any value in 1..256.  Four streaming passes, the per-channel arithmetic between them is masked_bn.hip's (pnx_masked_bn_reduce / _finalize /
// _bwd_finalize take any C <= 256):
//   k_sp3_bn_stats      per workgroup [sum d | sum d^2 | rows], d = y - center[c]
//   k_sp3_bn_apply      out = relu?(y * scale + shift (+ residual)) fp32 (n, C), and in the same pass out_h = out rounded once into padded
//                       16-bit rows (n, round_up(C, 8)), pad columns zero -- what the next convolution reads
//   k_sp3_bn_bwd_stats  per workgroup [sum g | sum g xhat], g = gout * [z > 0] with z recomputed as the forward computed it
//   k_sp3_bn_bwd_apply  dy = scale * (g - mean_g - xhat * mean_gx), dresidual = g
// The residual is fp32 (n, C) or padded 16-bit rows (n, round_up(C, 8)).
//
// One thread owns ONE chunk of 8 consecutive channels (q = thread % cpc, cpc = ceil(C / 8) chunks per row) of the rows it walks, so the
// per-channel vectors sit in registers and a row's last chunk carries C - 8 (cpc - 1) live channels (the others are never loaded or stored:
// nothing assumes that C divides the wave).  A workgroup of 256 threads covers rpp = 256 / cpc whole rows per pass (256 - rpp cpc < cpc threads idle),
// consecutive threads read consecutive 32-byte pieces of consecutive rows: 16 bytes per load where C % 4 == 0, 8 where C % 2 == 0, else 4.
//
// The split (sp3_bn_split): tiles = ceil(n / rpp), blocks = min(tiles, 1024), passes = ceil(tiles / blocks).  Workgroup b takes the tiles b,
// b + blocks, b + 2 blocks, ...; its thread (r, q) adds the terms of rows (b + k blocks) rpp + r, k = 0, 1, ..., in that order (at most `passes`
// terms), then thread (0, q) adds the rpp per-thread sums r = 0, 1, ..., rpp - 1 in that order: the longest fp32 chain of a partial is
// passes + rpp terms, each term formed with at most 3 roundings (d, d d; xhat = (y - mean) invstd, g xhat).  The caller adds the `blocks`
// partials in fp64 (pnx_masked_bn_reduce).  No atomics, no dependence on timing: bit-identical run to run.
#pragma once

constexpr int kSp3BnBlocks = 1024;

struct Sp3BnSplit {
  int cpc, rpp, blocks;
  int64_t passes;
};

inline Sp3BnSplit sp3_bn_split(int64_t n, int C) {
  Sp3BnSplit s;
  s.cpc = (C + 7) / 8;
  s.rpp = kBlock / s.cpc;
  const int64_t tiles = (n + s.rpp - 1) / s.rpp;
  s.blocks = (int)(tiles < kSp3BnBlocks ? tiles : kSp3BnBlocks);
  s.passes = s.blocks > 0 ? (tiles + s.blocks - 1) / s.blocks : 0;
  return s;
}

// the partials of one statistics pass: one carve for the size query and the launch
struct Sp3BnWs {
  Sp3BnSplit sp;
  float* part;
  int cols;
  size_t bytes;
};

inline Sp3BnWs sp3_bn_carve(void* base, int64_t n, int C, bool backward) {
  Sp3BnWs w;
  w.sp = sp3_bn_split(n, C);
  w.cols = 2 * C + (backward ? 0 : 1);
  PnxCarver c(base);
  w.part = c.take<float>((size_t)w.sp.blocks * w.cols);
  w.bytes = c.used() < 256 ? 256 : c.used();
  return w;
}

typedef float f32x8 __attribute__((ext_vector_type(8)));

// 8 floats of a chunk with `valid` live ones (a multiple of V), V floats per load; the others read as zero
template <int V>
__device__ __forceinline__ void sp3_bn_ld(const float* __restrict__ p, int valid, float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k += V) {
    if (k < valid) {
      if constexpr (V == 4) {
        const float4 a = *reinterpret_cast<const float4*>(p + k);
        v[k] = a.x, v[k + 1] = a.y, v[k + 2] = a.z, v[k + 3] = a.w;
      } else if constexpr (V == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p + k);
        v[k] = a.x, v[k + 1] = a.y;
      } else {
        v[k] = p[k];
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) v[k + j] = 0.f;
    }
  }
}

template <int V>
__device__ __forceinline__ void sp3_bn_st(float* __restrict__ p, int valid, const float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k += V) {
    if (k >= valid) continue;
    if constexpr (V == 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    else if constexpr (V == 2) *reinterpret_cast<float2*>(p + k) = make_float2(v[k], v[k + 1]);
    else p[k] = v[k];
  }
}

// a per-channel vector's 8 values of the thread's chunk, read once (the chunk never changes along a thread's walk)
__device__ __forceinline__ void sp3_bn_par(const float* __restrict__ p, int c0, int valid, float (&v)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = (p != nullptr && k < valid) ? p[c0 + k] : 0.f;
}

// one 16-byte chunk of a padded 16-bit row as floats (exact)
template <int DT>
__device__ __forceinline__ void sp3_bn_ld_h(const void* __restrict__ rows, int64_t chunk, float (&v)[8]) {
  if constexpr (DT != PNX_F32) {
    const f32x8 f = __builtin_convertvector(static_cast<const typename Sp3Half<DT>::v8*>(rows)[chunk], f32x8);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = f[k];
  }
}

// the residual operand: none, fp32 (n, C) or padded 16-bit rows of type DT
struct Sp3BnRes {
  const float* f;
  const void* h;
};

template <int V, int DT>
__device__ __forceinline__ void sp3_bn_ld_res(const Sp3BnRes& res, int64_t row, int C, int cpc, int q, int valid, float (&r)[8]) {
  if (res.f != nullptr) sp3_bn_ld<V>(res.f + row * C + q * 8, valid, r);
  else if (res.h != nullptr) sp3_bn_ld_h<DT>(res.h, row * cpc + q, r);
}

// sums of NV vectors of 8 channels per thread -> out[NV * C (+ 1: rows)]: thread (0, q) adds the threads (r, q), r = 0 .. rpp - 1, in that order
template <int NV>
__device__ __forceinline__ void sp3_bn_block_reduce(const float (&acc)[NV][8], float cnt, bool with_cnt, int cpc, int rpp, int C, float* __restrict__ out) {
  __shared__ float s_red[kBlock * 8];
  __shared__ float s_cnt[kBlock];
  const int t = threadIdx.x;
  for (int v = 0; v < NV; v++) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) s_red[t * 8 + k] = acc[v][k];
    if (v == 0) s_cnt[t] = cnt;
    __syncthreads();
    if (t < cpc * 8 && t < C) {  // channel t = chunk t / 8, element t % 8
      const int q = t >> 3, k = t & 7;
      float s = 0.f;
      for (int r = 0; r < rpp; r++) s += s_red[(r * cpc + q) * 8 + k];
      out[v * C + t] = s;
    }
    if (v == 0 && with_cnt && t == 0) {
      float s = 0.f;
      for (int r = 0; r < rpp; r++) s += s_cnt[r * cpc];  // the chunk-0 threads counted their rows
      out[NV * C] = s;
    }
  }
}

// Every thread of a statistics kernel reaches the barriers of the reduction: an idle thread (r >= rpp) walks no row and hands in zeros.
template <int V>
__global__ __launch_bounds__(kBlock) void k_sp3_bn_stats(const float* __restrict__ y, int64_t n, int C, int rpp, const float* __restrict__ center,
                                                         float* __restrict__ partials) {
  const int cpc = (C + 7) >> 3, t = threadIdx.x, q = t % cpc, r = t / cpc;
  const int c0 = q * 8, valid = C - c0 < 8 ? C - c0 : 8;
  float ctr[8];
  sp3_bn_par(center, c0, valid, ctr);
  float acc[2][8] = {};
  float cnt = 0.f;
  const int64_t stride = (int64_t)gridDim.x * rpp;
  // two rows of the walk per iteration, their loads requested together; the additions keep the walk's order
  for (int64_t row = r < rpp ? (int64_t)blockIdx.x * rpp + r : n; row < n; row += 2 * stride) {
    float v[2][8];
    const bool two = row + stride < n;
    sp3_bn_ld<V>(y + row * C + c0, valid, v[0]);
    if (two) sp3_bn_ld<V>(y + (row + stride) * C + c0, valid, v[1]);
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (u == 1 && !two) continue;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const float d = k < valid ? v[u][k] - ctr[k] : 0.f;
        acc[0][k] += d, acc[1][k] += d * d;
      }
      if (q == 0) cnt += 1.f;
    }
  }
  sp3_bn_block_reduce<2>(acc, cnt, true, cpc, rpp, C, partials + (size_t)blockIdx.x * (2 * C + 1));
}

template <int V, int DT>
__global__ __launch_bounds__(kBlock) void k_sp3_bn_apply(const float* __restrict__ y, int64_t n, int C, int rpp, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, Sp3BnRes res, int relu, float* __restrict__ out,
                                                         void* __restrict__ out_h) {
  const int cpc = (C + 7) >> 3, t = threadIdx.x, q = t % cpc, r = t / cpc;
  if (r >= rpp) return;  // no barrier below
  const int c0 = q * 8, valid = C - c0 < 8 ? C - c0 : 8;
  float sc[8], sh[8];
  sp3_bn_par(scale, c0, valid, sc), sp3_bn_par(shift, c0, valid, sh);
  const int64_t stride = (int64_t)gridDim.x * rpp;
  for (int64_t row0 = (int64_t)blockIdx.x * rpp + r; row0 < n; row0 += 2 * stride) {
    float v[2][8], rs[2][8] = {};
    const bool two = row0 + stride < n;
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (u == 1 && !two) continue;
      const int64_t row = row0 + u * stride;
      sp3_bn_ld<V>(y + row * C + c0, valid, v[u]);
      sp3_bn_ld_res<V, DT>(res, row, C, cpc, q, valid, rs[u]);
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (u == 1 && !two) continue;
      const int64_t row = row0 + u * stride;
      float o[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const float z = v[u][k] * sc[k] + sh[k] + rs[u][k];
        o[k] = k < valid ? ((relu && !(z > 0.f)) ? 0.f : z) : 0.f;  // pad columns exactly zero
      }
      sp3_bn_st<V>(out + row * C + c0, valid, o);
      if constexpr (DT != PNX_F32) {
        if (out_h != nullptr) {
          const f32x8 f = {o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]};
          static_cast<typename Sp3Half<DT>::v8*>(out_h)[row * cpc + q] = __builtin_convertvector(f, typename Sp3Half<DT>::v8);  // the one rounding (nearest even)
        }
      }
    }
  }
}

// the per-channel vectors of the backward passes for one chunk
struct Sp3BnBwdPar {
  float sc[8], sh[8], mu[8], is[8];
};

// g of one (row, chunk): gout gated by the pre-activation, recomputed with the forward's own operations; xh = (y - mean) * invstd
template <int V, int DT>
__device__ __forceinline__ void sp3_bn_bwd_terms(const float* __restrict__ gout, const float* __restrict__ y, const Sp3BnRes& res, int64_t row, int C, int cpc,
                                                 int q, int valid, const Sp3BnBwdPar& P, int relu, float (&g)[8], float (&xh)[8]) {
  float v[8], rs[8] = {};
  sp3_bn_ld<V>(gout + row * C + q * 8, valid, g);
  sp3_bn_ld<V>(y + row * C + q * 8, valid, v);
  if (relu) sp3_bn_ld_res<V, DT>(res, row, C, cpc, q, valid, rs);  // without the gate the residual is not needed
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const float z = v[k] * P.sc[k] + P.sh[k] + rs[k];
    if (relu && !(z > 0.f)) g[k] = 0.f;
    xh[k] = (v[k] - P.mu[k]) * P.is[k];
  }
}

template <int V, int DT>
__global__ __launch_bounds__(kBlock) void k_sp3_bn_bwd_stats(const float* __restrict__ gout, const float* __restrict__ y, Sp3BnRes res, int64_t n, int C, int rpp,
                                                             const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, int relu, float* __restrict__ partials) {
  const int cpc = (C + 7) >> 3, t = threadIdx.x, q = t % cpc, r = t / cpc;
  const int c0 = q * 8, valid = C - c0 < 8 ? C - c0 : 8;
  Sp3BnBwdPar P;
  sp3_bn_par(scale, c0, valid, P.sc), sp3_bn_par(shift, c0, valid, P.sh), sp3_bn_par(mean, c0, valid, P.mu), sp3_bn_par(invstd, c0, valid, P.is);
  float acc[2][8] = {};
  const int64_t stride = (int64_t)gridDim.x * rpp;
  for (int64_t row = r < rpp ? (int64_t)blockIdx.x * rpp + r : n; row < n; row += 2 * stride) {
    float g[2][8], xh[2][8];
    const bool two = row + stride < n;
    sp3_bn_bwd_terms<V, DT>(gout, y, res, row, C, cpc, q, valid, P, relu, g[0], xh[0]);
    if (two) sp3_bn_bwd_terms<V, DT>(gout, y, res, row + stride, C, cpc, q, valid, P, relu, g[1], xh[1]);
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (u == 1 && !two) continue;
#pragma unroll
      for (int k = 0; k < 8; k++) acc[0][k] += g[u][k], acc[1][k] += g[u][k] * xh[u][k];
    }
  }
  sp3_bn_block_reduce<2>(acc, 0.f, false, cpc, rpp, C, partials + (size_t)blockIdx.x * (2 * C));
}

template <int V, int DT>
__global__ __launch_bounds__(kBlock) void k_sp3_bn_bwd_apply(const float* __restrict__ gout, const float* __restrict__ y, Sp3BnRes res, int64_t n, int C, int rpp,
                                                             const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, int relu, const float* __restrict__ mean_g,
                                                             const float* __restrict__ mean_gx, float* __restrict__ dy, float* __restrict__ dres) {
  const int cpc = (C + 7) >> 3, t = threadIdx.x, q = t % cpc, r = t / cpc;
  if (r >= rpp) return;  // no barrier below
  const int c0 = q * 8, valid = C - c0 < 8 ? C - c0 : 8;
  Sp3BnBwdPar P;
  sp3_bn_par(scale, c0, valid, P.sc), sp3_bn_par(shift, c0, valid, P.sh), sp3_bn_par(mean, c0, valid, P.mu), sp3_bn_par(invstd, c0, valid, P.is);
  float mg[8], mgx[8];
  sp3_bn_par(mean_g, c0, valid, mg), sp3_bn_par(mean_gx, c0, valid, mgx);
  const int64_t stride = (int64_t)gridDim.x * rpp;
  for (int64_t row = (int64_t)blockIdx.x * rpp + r; row < n; row += stride) {
    float g[8], xh[8], d[8];
    sp3_bn_bwd_terms<V, DT>(gout, y, res, row, C, cpc, q, valid, P, relu, g, xh);
#pragma unroll
    for (int k = 0; k < 8; k++) d[k] = P.sc[k] * (g[k] - mg[k] - xh[k] * mgx[k]);
    sp3_bn_st<V>(dy + row * C + c0, valid, d);
    if (dres != nullptr) sp3_bn_st<V>(dres + row * C + c0, valid, g);
  }
}

// the instantiation a call takes: floats per load from the row length, the 16-bit type in play (PNX_F32: none)
#define SP3_BN_DISPATCH(C, DT, GO)                       \
  do {                                                   \
    if ((C) % 4 == 0) {                                  \
      if ((DT) == PNX_BF16) GO(4, PNX_BF16);             \
      else if ((DT) == PNX_F16) GO(4, PNX_F16);          \
      else GO(4, PNX_F32);                               \
    } else if ((C) % 2 == 0) {                           \
      if ((DT) == PNX_BF16) GO(2, PNX_BF16);             \
      else if ((DT) == PNX_F16) GO(2, PNX_F16);          \
      else GO(2, PNX_F32);                               \
    } else {                                             \
      if ((DT) == PNX_BF16) GO(1, PNX_BF16);             \
      else if ((DT) == PNX_F16) GO(1, PNX_F16);          \
      else GO(1, PNX_F32);                               \
    }                                                    \
  } while (0)
