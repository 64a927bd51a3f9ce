// sparse3d.hip -- sparse 3-D convolution for SparseResNet3D (det3d/models/backbones/sparse_resnet3d.py, utils/sparse_conv.py:66-104):
//   pnx_sp3_index_build   key-order occupancy bitmap + popcount word prefix of an active set (the index)
//   pnx_sp3_out_index     index of the output set of SparseConv3d: every input x tap sets the bit of the output it reaches
//   pnx_sp3_index_coords  the set's [b, z, y, x] rows in key (= rank) order
//   pnx_sp3_neighbor_map  (N_out, T) input row per output site and tap, -1 where the neighbour is inactive
//   pnx_sp3_conv          gather-GEMM on the fp32 matrix cores + folded BN shift (+ residual) (+ ReLU)
//   pnx_sp3_dense         rows -> zero-initialised (B, C*D, H, W), channel c*D + d (x.dense().view(B, C*D, H, W), :67-71)
//   pnx_sp3_conv_h, pnx_sp3_dense_h   the same two on bf16 / fp16 rows and the 16-bit matrix cores, inference only (sparse3d_half.h)
// and, for training:
//   pnx_sp3_transpose_map   tmap (N_in, T): tmap[map[o][t]][t] = o, -1 elsewhere -- the data gradient is pnx_sp3_conv_train on dy, tmap and w^T
//   pnx_sp3_wgrad           dw[co][t][ci] = sum_o dy[o][co] * x[map[o][t]][ci]: split-K gather-GEMM, fp32 partials added in a fixed order
//   pnx_sp3_dense_backward  the gather that undoes pnx_sp3_dense
//   pnx_sp3_conv_h_f32, pnx_sp3_wgrad_h   forward / data gradient and weight gradient on bf16 / fp16 operands, fp32 results (sparse3d_half_train.h)
//   pnx_sp3_bn_stats, _apply, _bwd_stats, _bwd_apply   train-mode BatchNorm1d + residual + ReLU over the rows, forward and backward (sparse3d_bn.h)
//
// A site's key is ((b*D + z)*H + y)*W + x (64-bit), one bit of the bitmap; its rank (the row it occupies) is the number of set bits
// below it: blk[word >> PNX_SCAN_SHIFT] + pre[word] + popc(bitmap[word] & below).  Ranks follow [b, z, y, x] lexicographic order, which
// is torch.unique(dim=0)'s order and so the voxel reader's row order.  Neighbour lookup is a bit test and that rank: no hash table.
//
// Convolution: a wave owns 16 output rows and every output channel (NT tiles of 16); K runs tap by tap, Cin in steps of 4, on
// v_mfma_f32_16x16x4_f32 -- exact fp32 products accumulated in k order, so every output row is reduced in one fixed order whatever the
// tiling (a missing neighbour contributes 0 * w, which leaves the sum unchanged), and a tap none of the 16 rows has is skipped.
//
// Weight gradient: per tap a (Cout x Cin) GEMM whose K runs over the output rows.  Both operands are row-major in memory with the channel
// contiguous, and the fp32 MFMA wants exactly that: A = dy^T is A[m = lane & 15][k = lane >> 4] = dy[row k][co m], B = x gathered is
// B[k = lane >> 4][n = lane & 15] = x[map[row k][t]][ci n] -- 16 consecutive lanes read 16 consecutive floats of one row, no transpose.
// Rows are dealt statically: workgroup c owns rows [c R, (c + 1) R) (sp3_wgrad_split), its four waves take the taps wave, wave + 4, ...
// one after the other (the chunk's map, x and dy rows stay in cache across the taps), a wave accumulates MT x NT tiles of 16 x 16 over the
// chunk in row order -- a K step of 16 rows none of which has the tap costs no MFMA -- and writes them to partial c; k_sp3_wgrad_sum adds
// the partials in index order.  No floating-point atomics: the result does not depend on timing.
#include <algorithm>

#include "pnx_common.h"
#include "pnx_scan.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#include "sparse3d_index.h"  // Sp3Grid, Sp3Index, sp3_carve, sp3_grid, sp3_index_args, sp3_key, sp3_rank

// output extent (n + 2 pad - k) / s + 1 per axis; fills o and returns PNX_OK, or an error for a geometry without outputs
int sp3_conv_geom(const Sp3Grid& in, const int32_t* k3, const int32_t* s3, const int32_t* p3, Sp3Grid* out) {
  PNX_REQUIRE(k3 && s3 && p3, PNX_ERR_INVALID, "sparse3d: kernel / stride / padding is NULL");
  const int n[3] = {in.D, in.H, in.W};
  int o[3];
  for (int a = 0; a < 3; a++) {
    PNX_REQUIRE(k3[a] >= 1 && k3[a] <= 3 && s3[a] >= 1 && s3[a] <= 2 && p3[a] >= 0 && p3[a] < k3[a], PNX_ERR_UNSUPPORTED,
                "sparse3d: axis %d kernel %d stride %d padding %d (kernels 1..3, strides 1..2)", a, k3[a], s3[a], p3[a]);
    PNX_REQUIRE(n[a] + 2 * p3[a] >= k3[a], PNX_ERR_INVALID, "sparse3d: axis %d of extent %d is smaller than the kernel", a, n[a]);
    o[a] = (n[a] + 2 * p3[a] - k3[a]) / s3[a] + 1;
  }
  out->B = in.B, out->D = o[0], out->H = o[1], out->W = o[2];
  return PNX_OK;
}

struct Sp3Conv {
  int k[3], s[3], p[3];
};

__device__ __forceinline__ bool sp3_row(const int32_t* __restrict__ coords, int64_t i, const Sp3Grid& g, int (&c)[4]) {
  const int4 v = *reinterpret_cast<const int4*>(coords + 4 * i);
  c[0] = v.x, c[1] = v.y, c[2] = v.z, c[3] = v.w;
  return c[0] >= 0 && c[0] < g.B && c[1] >= 0 && c[1] < g.D && c[2] >= 0 && c[2] < g.H && c[3] >= 0 && c[3] < g.W;
}

// rows with a coordinate outside the grid are skipped here (the module rejects them before calling)
__global__ __launch_bounds__(kBlock) void k_sp3_mark(const int32_t* __restrict__ coords, int64_t n, Sp3Grid g, uint32_t* __restrict__ bitmap) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int c[4];
  if (!sp3_row(coords, i, g, c)) return;
  const int64_t k = sp3_key(g, c[0], c[1], c[2], c[3]);
  atomicOr(&bitmap[k >> 5], 1u << (k & 31));
}

__global__ __launch_bounds__(kBlock) void k_sp3_row_of_rank(const int32_t* __restrict__ coords, int64_t n, Sp3Grid g, const uint32_t* __restrict__ bitmap,
                                                            const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk, int32_t* __restrict__ row_of_rank) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int c[4];
  if (!sp3_row(coords, i, g, c)) return;
  const uint32_t r = sp3_rank(bitmap, pre, blk, sp3_key(g, c[0], c[1], c[2], c[3]));
  if ((int64_t)r < n) row_of_rank[r] = (int32_t)i;
}

// output q exists iff some active input p = q*s - pad + o: for every input and tap, (p + pad - o) divisible by s and inside the output grid
__global__ __launch_bounds__(kBlock) void k_sp3_mark_out(const int32_t* __restrict__ coords, int64_t n, Sp3Grid gi, Sp3Grid go, Sp3Conv cv,
                                                         uint32_t* __restrict__ bitmap) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  int c[4];
  if (!sp3_row(coords, i, gi, c)) return;
  for (int od = 0; od < cv.k[0]; od++) {
    const int z = c[1] + cv.p[0] - od;
    if (z < 0 || z % cv.s[0] != 0 || z / cv.s[0] >= go.D) continue;
    for (int oh = 0; oh < cv.k[1]; oh++) {
      const int yy = c[2] + cv.p[1] - oh;
      if (yy < 0 || yy % cv.s[1] != 0 || yy / cv.s[1] >= go.H) continue;
      for (int ow = 0; ow < cv.k[2]; ow++) {
        const int xx = c[3] + cv.p[2] - ow;
        if (xx < 0 || xx % cv.s[2] != 0 || xx / cv.s[2] >= go.W) continue;
        const int64_t k = sp3_key(go, c[0], z / cv.s[0], yy / cv.s[1], xx / cv.s[2]);
        atomicOr(&bitmap[k >> 5], 1u << (k & 31));
      }
    }
  }
}

// one thread per bitmap word: every set bit writes its [b, z, y, x] row at its rank
__global__ __launch_bounds__(kBlock) void k_sp3_coords(const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                                       int64_t nwords, Sp3Grid g, int32_t* __restrict__ coords, int64_t cap) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= nwords) return;
  uint32_t m = bitmap[w];
  int64_t r = (int64_t)blk[w >> PNX_SCAN_SHIFT] + pre[w];
  const int64_t hw = (int64_t)g.H * g.W, dhw = hw * g.D;
  while (m) {
    const int bit = __ffs(m) - 1;
    m &= m - 1;
    if (r < cap) {
      int64_t k = (w << 5) + bit;
      const int b = (int)(k / dhw);
      k -= (int64_t)b * dhw;
      const int z = (int)(k / hw);
      k -= (int64_t)z * hw;
      *reinterpret_cast<int4*>(coords + 4 * r) = make_int4(b, z, (int)(k / g.W), (int)(k % g.W));
    }
    r++;
  }
}

// map[row][tap] = input row at q*s - pad + o (tap = (od*kh + oh)*kw + ow, spconv's kernel order), -1 where that site is inactive or outside
__global__ __launch_bounds__(kBlock) void k_sp3_nbmap(const int32_t* __restrict__ coords_out, int64_t n_out, Sp3Grid go, Sp3Grid gi, Sp3Conv cv,
                                                      const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ pre,
                                                      const uint32_t* __restrict__ blk, const int32_t* __restrict__ row_of_rank, int T,
                                                      int32_t* __restrict__ map) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_out * T) return;
  const int64_t i = e / T;
  const int t = (int)(e - i * T);
  int c[4];
  int32_t v = -1;
  if (sp3_row(coords_out, i, go, c)) {
    const int o[3] = {t / (cv.k[1] * cv.k[2]), (t / cv.k[2]) % cv.k[1], t % cv.k[2]};
    const int n[3] = {gi.D, gi.H, gi.W};
    int p[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      p[a] = c[1 + a] * cv.s[a] - cv.p[a] + o[a];
      ok = ok && p[a] >= 0 && p[a] < n[a];
    }
    if (ok) {
      const int64_t k = sp3_key(gi, c[0], p[0], p[1], p[2]);
      if ((bitmap[k >> 5] >> (k & 31)) & 1u) {
        const uint32_t r = sp3_rank(bitmap, pre, blk, k);
        v = row_of_rank ? row_of_rank[r] : (int32_t)r;
      }
    }
  }
  map[e] = v;
}

// y[row] = relu?( sum_t sum_c x[map[row][t]][c] * w'[t][c][:] + shift (+ residual[row]) ).  w' is (T, cin4, NT*16): BN scale folded in, zero-padded.
// PERTAP (training): every tap is summed from zero on its own and the taps are added in tap order -- the summation tree of a matmul per tap, whose
// chains are one tap long; a row with t taps otherwise carries a chain t times as long and about sqrt(t) times the rounding error.
template <int NT, bool PERTAP>
__global__ __launch_bounds__(kBlock) void k_sp3_conv(const float* __restrict__ x, int64_t n_in, int cin, const int32_t* __restrict__ map, int64_t n_out, int T,
                                                     const float* __restrict__ wp, const float* __restrict__ shift, const float* __restrict__ res, int relu,
                                                     float* __restrict__ y, int cout) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row0 = ((int64_t)blockIdx.x * (kBlock / 64) + wave) * 16;
  if (row0 >= n_out) return;  // wave-uniform; the kernel has no barrier
  const int r = lane & 15, kk = lane >> 4;
  const int64_t row = row0 + r;
  const int cin4 = (cin + 3) & ~3, ldw = NT * 16;
  f32x4 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; j++) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < T; t++) {
    int32_t nb = row < n_out ? map[row * T + t] : -1;
    if ((int64_t)nb >= n_in) nb = -1;
    if (__ballot(nb >= 0) == 0) continue;  // no row of the tile has this neighbour: no MFMA
    const float* xr = x + (int64_t)(nb < 0 ? 0 : nb) * cin;
    const float* wt = wp + (int64_t)t * cin4 * ldw + r;
    if constexpr (PERTAP) {
      f32x4 tap[NT];
#pragma unroll
      for (int j = 0; j < NT; j++) tap[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < cin; k0 += 4) {
        const int k = k0 + kk;
        const float a = (nb >= 0 && k < cin) ? xr[k] : 0.f;
        const float* wk = wt + (int64_t)k * ldw;
#pragma unroll
        for (int j = 0; j < NT; j++) tap[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wk[j * 16], tap[j], 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < NT; j++) acc[j] += tap[j];
    } else {
      for (int k0 = 0; k0 < cin; k0 += 4) {
        const int k = k0 + kk;
        const float a = (nb >= 0 && k < cin) ? xr[k] : 0.f;
        const float* wk = wt + (int64_t)k * ldw;
#pragma unroll
        for (int j = 0; j < NT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, wk[j * 16], acc[j], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const int col = j * 16 + r;
    if (col >= cout) continue;
    const float sh = shift[col];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int64_t orow = row0 + kk * 4 + i;
      if (orow >= n_out) continue;
      float v = acc[j][i] + sh;
      if (res) v += res[orow * cout + col];
      if (relu && v < 0.f) v = 0.f;
      y[orow * cout + col] = v;
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_sp3_dense(const float* __restrict__ feat, const int32_t* __restrict__ coords, int64_t n, int C, Sp3Grid g,
                                                      float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n * C) return;
  const int64_t i = e / C;
  const int ch = (int)(e - i * C);
  int c[4];
  if (!sp3_row(coords, i, g, c)) return;
  out[((((int64_t)c[0] * C + ch) * g.D + c[1]) * g.H + c[2]) * g.W + c[3]] = feat[e];
}

unsigned sp3_blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

#include "sparse3d_half.h"  // the 16-bit inference form: k_sp3_conv_h, k_sp3_dense_h and their launchers

// tmap[map[o][t]][t] = o: for one input row and tap there is at most one output row (q = (p + pad - o) / s), so no two threads meet
__global__ __launch_bounds__(kBlock) void k_sp3_tmap(const int32_t* __restrict__ map, int64_t n_out, int T, int64_t n_in, int32_t* __restrict__ tmap) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_out * T) return;
  const int64_t o = e / T;
  const int t = (int)(e - o * T);
  const int32_t v = map[e];
  if (v >= 0 && (int64_t)v < n_in) tmap[(int64_t)v * T + t] = (int32_t)o;
}

// partial[c][co][t][ci] = sum over rows o of chunk c, in row order, of dy[o][co] * x[map[o][t]][ci]
template <int MT, int NT>
__global__ __launch_bounds__(kBlock) void k_sp3_wgrad(const float* __restrict__ x, int64_t n_in, int cin, const float* __restrict__ dy, int cout,
                                                      const int32_t* __restrict__ map, int64_t n_out, int T, int R, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kk = lane >> 4;
  const int64_t c = blockIdx.x;
  const int co0 = blockIdx.y * (MT * 16);
  const int64_t row_begin = c * R;
  const int64_t row_end = row_begin + R < n_out ? row_begin + R : n_out;
  for (int t = wave; t < T; t += kBlock / 64) {
    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int j = 0; j < NT; j++) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t row0 = row_begin; row0 < row_end; row0 += 16) {
      int32_t nb[4];
      bool any = false;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int64_t row = row0 + 4 * s + kk;
        int32_t v = row < row_end ? map[row * T + t] : -1;
        if ((int64_t)v >= n_in) v = -1;
        nb[s] = v;
        any = any || v >= 0;
      }
      if (__ballot(any) == 0) continue;  // no row of the K step has this tap: no MFMA
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const bool on = nb[s] >= 0;
        const float* dr = dy + (row0 + 4 * s + kk) * cout + co0 + r;
        const float* xr = x + (int64_t)(on ? nb[s] : 0) * cin + r;
        float a[MT], b[NT];
#pragma unroll
        for (int m = 0; m < MT; m++) a[m] = (on && co0 + m * 16 + r < cout) ? dr[m * 16] : 0.f;
#pragma unroll
        for (int j = 0; j < NT; j++) b[j] = (on && j * 16 + r < cin) ? xr[j * 16] : 0.f;
#pragma unroll
        for (int m = 0; m < MT; m++) {
          if (co0 + m * 16 >= cout) continue;  // uniform: a channel tile past the layer's last
#pragma unroll
          for (int j = 0; j < NT; j++) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m], b[j], acc[m][j], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const int ci = j * 16 + r;
        if (ci >= cin) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int co = co0 + m * 16 + kk * 4 + i;
          if (co < cout) part[(((int64_t)c * cout + co) * T + t) * cin + ci] = acc[m][j][i];
        }
      }
  }
}

// dw[e] = partial[0][e] + partial[1][e] + ... in that order
__global__ __launch_bounds__(kBlock) void k_sp3_wgrad_sum(const float* __restrict__ part, int P, int64_t E, float* __restrict__ dw) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= E) return;
  float v = 0.f;
#pragma unroll 8
  for (int p = 0; p < P; p++) v += part[(int64_t)p * E + e];
  dw[e] = v;
}

__global__ __launch_bounds__(kBlock) void k_sp3_dense_bwd(const float* __restrict__ dout, const int32_t* __restrict__ coords, int64_t n, int C, Sp3Grid g,
                                                          float* __restrict__ dfeat) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n * C) return;
  const int64_t i = e / C;
  const int ch = (int)(e - i * C);
  int c[4];
  dfeat[e] = sp3_row(coords, i, g, c) ? dout[((((int64_t)c[0] * C + ch) * g.D + c[1]) * g.H + c[2]) * g.W + c[3]] : 0.f;
}

// The weight gradient's static split: output-channel tiles per wave (MT), rows per workgroup R (a multiple of 16, 256 .. 4096: about 256
// workgroups, a chunk small enough to stay in cache over the taps) and the number of partials P = ceil(n_out / R).
struct Sp3WgradSplit {
  int mt, groups, R;
  int64_t P;
};

Sp3WgradSplit sp3_wgrad_split(int64_t n_out, int cout) {
  Sp3WgradSplit s;
  const int tiles = (cout + 15) / 16;
  s.mt = tiles <= 3 ? tiles : (tiles % 3 == 0 ? 3 : (tiles % 2 == 0 ? 2 : 3));
  s.groups = (tiles + s.mt - 1) / s.mt;
  const int64_t p0 = 256 / s.groups > 1 ? 256 / s.groups : 1;
  int64_t R = ((n_out + p0 - 1) / p0 + 15) & ~(int64_t)15;
  R = R < 256 ? 256 : (R > 4096 ? 4096 : R);
  s.R = (int)R;
  s.P = n_out > 0 ? (n_out + R - 1) / R : 0;
  return s;
}

template <int MT, int NT>
void sp3_wgrad_launch(dim3 grid, hipStream_t st, const float* x, int64_t n_in, int cin, const float* dy, int cout, const int32_t* map, int64_t n_out, int T,
                      int R, float* part) {
  k_sp3_wgrad<MT, NT><<<grid, kBlock, 0, st>>>(x, n_in, cin, dy, cout, map, n_out, T, R, part);
}

template <int MT>
void sp3_wgrad_nt(int nt, dim3 grid, hipStream_t st, const float* x, int64_t n_in, int cin, const float* dy, int cout, const int32_t* map, int64_t n_out,
                  int T, int R, float* part) {
  switch (nt) {
    case 1: sp3_wgrad_launch<MT, 1>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 2: sp3_wgrad_launch<MT, 2>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 3: sp3_wgrad_launch<MT, 3>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 4: sp3_wgrad_launch<MT, 4>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 5: sp3_wgrad_launch<MT, 5>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 6: sp3_wgrad_launch<MT, 6>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 7: sp3_wgrad_launch<MT, 7>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    case 8: sp3_wgrad_launch<MT, 8>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
    default: sp3_wgrad_launch<MT, 9>(grid, st, x, n_in, cin, dy, cout, map, n_out, T, R, part); break;
  }
}

#include "sparse3d_half_train.h"  // the 16-bit training form: k_sp3_wgrad_h, its split and its partials buffer
#include "sparse3d_bn.h"          // train-mode BatchNorm + residual + ReLU over the rows: k_sp3_bn_*, their split and their partials buffer

// bitmap already marked: word prefix (level 1 + level 2), total set bits -> count
int sp3_scan(const Sp3Index& ix, int32_t* count, hipStream_t st) {
  if (ix.nblk > 0) k_scan_local<SCAN_POPC><<<ix.nblk, kBlock, 0, st>>>(ix.bitmap, ix.nwords, ix.pre, ix.blk);
  k_scan_blocks<<<1, kBlock, 0, st>>>(ix.blk, ix.nblk, count);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

template <int NT>
void sp3_conv_launch(bool per_tap, unsigned nb, hipStream_t st, const float* x, int64_t n_in, int cin, const int32_t* map, int64_t n_out, int T,
                     const float* wp, const float* shift, const float* res, int relu, float* y, int cout) {
  if (per_tap)
    k_sp3_conv<NT, true><<<nb, kBlock, 0, st>>>(x, n_in, cin, map, n_out, T, wp, shift, res, relu, y, cout);
  else
    k_sp3_conv<NT, false><<<nb, kBlock, 0, st>>>(x, n_in, cin, map, n_out, T, wp, shift, res, relu, y, cout);
}

}  // namespace

extern "C" {

size_t pnx_sp3_index_bytes(int32_t batch, const int32_t* grid3_host) {
  Sp3Grid g;
  if (sp3_grid(batch, grid3_host, &g) != PNX_OK) return 0;
  return sp3_carve(nullptr, g).bytes;
}

int pnx_sp3_index_build(const int32_t* coords, int64_t n, int32_t batch, const int32_t* grid3_host, void* index, size_t index_bytes, int32_t* row_of_rank,
                        int32_t* count, pnx_stream_t stream) {
  Sp3Grid g;
  Sp3Index ix;
  int rc = sp3_grid(batch, grid3_host, &g);
  if (rc == PNX_OK) rc = sp3_index_args(g, index, index_bytes, &ix);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), PNX_ERR_INVALID, "pnx_sp3_index_build: %lld rows", (long long)n);
  PNX_REQUIRE(n == 0 || (coords != nullptr && ((uintptr_t)coords & 15) == 0), PNX_ERR_INVALID, "pnx_sp3_index_build: coords NULL or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  PNX_CHECK_HIP(hipMemsetAsync(ix.bitmap, 0, (size_t)ix.nwords * 4, st));
  if (n > 0) k_sp3_mark<<<sp3_blocks(n), kBlock, 0, st>>>(coords, n, g, ix.bitmap);
  rc = sp3_scan(ix, count, st);
  if (rc != PNX_OK) return rc;
  if (row_of_rank && n > 0) {
    k_sp3_row_of_rank<<<sp3_blocks(n), kBlock, 0, st>>>(coords, n, g, ix.bitmap, ix.pre, ix.blk, row_of_rank);
    PNX_LAUNCH_CHECK();
  }
  return PNX_OK;
}

int pnx_sp3_out_grid(int32_t batch, const int32_t* grid_in3_host, const int32_t* kernel3_host, const int32_t* stride3_host, const int32_t* pad3_host,
                     int32_t* grid_out3_host) {
  Sp3Grid gi, go;
  int rc = sp3_grid(batch, grid_in3_host, &gi);
  if (rc == PNX_OK) rc = sp3_conv_geom(gi, kernel3_host, stride3_host, pad3_host, &go);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(grid_out3_host != nullptr, PNX_ERR_INVALID, "pnx_sp3_out_grid: grid_out3_host is NULL");
  grid_out3_host[0] = go.D, grid_out3_host[1] = go.H, grid_out3_host[2] = go.W;
  return PNX_OK;
}

int pnx_sp3_out_index(const int32_t* coords_in, int64_t n_in, int32_t batch, const int32_t* grid_in3_host, const int32_t* kernel3_host,
                      const int32_t* stride3_host, const int32_t* pad3_host, void* index_out, size_t index_out_bytes, int32_t* count, pnx_stream_t stream) {
  Sp3Grid gi, go;
  Sp3Index ix;
  int rc = sp3_grid(batch, grid_in3_host, &gi);
  if (rc == PNX_OK) rc = sp3_conv_geom(gi, kernel3_host, stride3_host, pad3_host, &go);
  if (rc == PNX_OK) rc = sp3_index_args(go, index_out, index_out_bytes, &ix);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(n_in >= 0 && n_in < ((int64_t)1 << 31), PNX_ERR_INVALID, "pnx_sp3_out_index: %lld rows", (long long)n_in);
  PNX_REQUIRE(n_in == 0 || (coords_in != nullptr && ((uintptr_t)coords_in & 15) == 0), PNX_ERR_INVALID,
              "pnx_sp3_out_index: coords NULL or not 16-byte aligned");
  Sp3Conv cv;
  for (int a = 0; a < 3; a++) cv.k[a] = kernel3_host[a], cv.s[a] = stride3_host[a], cv.p[a] = pad3_host[a];
  hipStream_t st = (hipStream_t)stream;
  PNX_CHECK_HIP(hipMemsetAsync(ix.bitmap, 0, (size_t)ix.nwords * 4, st));
  if (n_in > 0) k_sp3_mark_out<<<sp3_blocks(n_in), kBlock, 0, st>>>(coords_in, n_in, gi, go, cv, ix.bitmap);
  return sp3_scan(ix, count, st);
}

int pnx_sp3_index_coords(const void* index, size_t index_bytes, int32_t batch, const int32_t* grid3_host, int32_t* coords, int64_t capacity,
                         pnx_stream_t stream) {
  Sp3Grid g;
  Sp3Index ix;
  int rc = sp3_grid(batch, grid3_host, &g);
  if (rc == PNX_OK) rc = sp3_index_args(g, const_cast<void*>(index), index_bytes, &ix);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(capacity >= 0 && (capacity == 0 || (coords != nullptr && ((uintptr_t)coords & 15) == 0)), PNX_ERR_INVALID,
              "pnx_sp3_index_coords: coords NULL or not 16-byte aligned");
  if (capacity == 0 || ix.nwords == 0) return PNX_OK;
  k_sp3_coords<<<sp3_blocks(ix.nwords), kBlock, 0, (hipStream_t)stream>>>(ix.bitmap, ix.pre, ix.blk, ix.nwords, g, coords, capacity);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_neighbor_map(const int32_t* coords_out, int64_t n_out, const void* index_in, size_t index_in_bytes, int32_t batch, const int32_t* grid_in3_host,
                         const int32_t* row_of_rank_in, const int32_t* kernel3_host, const int32_t* stride3_host, const int32_t* pad3_host, int32_t* map,
                         pnx_stream_t stream) {
  Sp3Grid gi, go;
  Sp3Index ix;
  int rc = sp3_grid(batch, grid_in3_host, &gi);
  if (rc == PNX_OK) rc = sp3_conv_geom(gi, kernel3_host, stride3_host, pad3_host, &go);
  if (rc == PNX_OK) rc = sp3_index_args(gi, const_cast<void*>(index_in), index_in_bytes, &ix);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(n_out >= 0 && n_out < ((int64_t)1 << 31), PNX_ERR_INVALID, "pnx_sp3_neighbor_map: %lld rows", (long long)n_out);
  PNX_REQUIRE(n_out == 0 || (coords_out != nullptr && ((uintptr_t)coords_out & 15) == 0 && map != nullptr), PNX_ERR_INVALID,
              "pnx_sp3_neighbor_map: coords_out / map NULL or coords not 16-byte aligned");
  Sp3Conv cv;
  for (int a = 0; a < 3; a++) cv.k[a] = kernel3_host[a], cv.s[a] = stride3_host[a], cv.p[a] = pad3_host[a];
  const int T = cv.k[0] * cv.k[1] * cv.k[2];
  if (n_out == 0) return PNX_OK;
  k_sp3_nbmap<<<sp3_blocks(n_out * T), kBlock, 0, (hipStream_t)stream>>>(coords_out, n_out, go, gi, cv, ix.bitmap, ix.pre, ix.blk, row_of_rank_in, T, map);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

size_t pnx_sp3_packed_weight_floats(int32_t taps, int32_t cin, int32_t cout) {
  if (taps < 1 || cin < 1 || cout < 1) return 0;
  return (size_t)taps * ((cin + 3) & ~3) * ((cout + 15) & ~15);
}

static int sp3_conv_run(bool per_tap, const float* x, int64_t n_in, int32_t cin, const int32_t* map, int64_t n_out, int32_t taps, const float* w_packed,
                        const float* shift, const float* residual, int32_t relu, float* y, int32_t cout, pnx_stream_t stream) {
  const char* name = per_tap ? "pnx_sp3_conv_train" : "pnx_sp3_conv";
  PNX_REQUIRE(cin >= 1 && cin <= 1024 && cout >= 1 && cout <= 192 && taps >= 1 && taps <= 27, PNX_ERR_UNSUPPORTED,
              "%s: %d -> %d channels over %d taps (cin 1..1024, cout 1..192, taps 1..27)", name, cin, cout, taps);
  PNX_REQUIRE(n_in >= 0 && n_out >= 0 && n_out < ((int64_t)1 << 31), PNX_ERR_INVALID, "%s: %lld -> %lld rows", name, (long long)n_in,
              (long long)n_out);
  if (n_out == 0) return PNX_OK;
  PNX_REQUIRE(map && w_packed && shift && y && (n_in == 0 || x), PNX_ERR_INVALID, "%s: null pointer", name);
  const unsigned nb = (unsigned)((n_out + 63) / 64);
  hipStream_t st = (hipStream_t)stream;
  switch ((cout + 15) / 16) {
    case 1: sp3_conv_launch<1>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 2: sp3_conv_launch<2>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 3: sp3_conv_launch<3>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 4: sp3_conv_launch<4>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 5: sp3_conv_launch<5>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 6: sp3_conv_launch<6>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 7: sp3_conv_launch<7>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 8: sp3_conv_launch<8>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 9: sp3_conv_launch<9>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 10: sp3_conv_launch<10>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    case 11: sp3_conv_launch<11>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
    default: sp3_conv_launch<12>(per_tap, nb, st, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout); break;
  }
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_conv(const float* x, int64_t n_in, int32_t cin, const int32_t* map, int64_t n_out, int32_t taps, const float* w_packed, const float* shift,
                 const float* residual, int32_t relu, float* y, int32_t cout, pnx_stream_t stream) {
  return sp3_conv_run(false, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout, stream);
}

int pnx_sp3_conv_train(const float* x, int64_t n_in, int32_t cin, const int32_t* map, int64_t n_out, int32_t taps, const float* w_packed, const float* shift,
                       const float* residual, int32_t relu, float* y, int32_t cout, pnx_stream_t stream) {
  return sp3_conv_run(true, x, n_in, cin, map, n_out, taps, w_packed, shift, residual, relu, y, cout, stream);
}

int pnx_sp3_dense(const float* feat, const int32_t* coords, int64_t n, int32_t channels, int32_t batch, const int32_t* grid3_host, float* out,
                  pnx_stream_t stream) {
  Sp3Grid g;
  int rc = sp3_grid(batch, grid3_host, &g);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(n >= 0 && channels >= 1, PNX_ERR_INVALID, "pnx_sp3_dense: %lld rows of %d channels", (long long)n, channels);
  const size_t bytes = (size_t)g.B * channels * g.D * g.H * g.W * sizeof(float);
  if (bytes == 0) return PNX_OK;  // a batch of 0 samples
  PNX_REQUIRE(out != nullptr && (n == 0 || (feat && coords && ((uintptr_t)coords & 15) == 0)), PNX_ERR_INVALID, "pnx_sp3_dense: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PNX_CHECK_HIP(hipMemsetAsync(out, 0, bytes, st));
  if (n == 0) return PNX_OK;
  k_sp3_dense<<<sp3_blocks(n * channels), kBlock, 0, st>>>(feat, coords, n, channels, g, out);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

size_t pnx_sp3_packed_weight_halfs(int32_t taps, int32_t cin, int32_t cout) {
  if (taps < 1 || taps > 27 || cin < 1 || cin > 144 || cout < 1 || cout > 144) return 0;
  const int chunks = taps * ((cin + 7) / 8);
  return (size_t)((chunks + 3) / 4) * ((cout + 15) / 16) * 512;
}

int pnx_sp3_conv_h(const void* x, int64_t n_in, int32_t cin, int32_t cin_pad, const int32_t* map, int64_t n_out, int32_t taps, const void* w_packed,
                   const float* shift, const void* residual, int32_t relu, void* y, int32_t cout, int32_t cout_pad, int32_t dtype, pnx_stream_t stream) {
  PNX_REQUIRE(dtype == PNX_BF16 || dtype == PNX_F16, PNX_ERR_UNSUPPORTED, "pnx_sp3_conv_h: dtype %d (PNX_BF16 or PNX_F16)", dtype);
  PNX_REQUIRE(cin >= 1 && cin <= 144 && cout >= 1 && cout <= 144 && taps >= 1 && taps <= 27, PNX_ERR_UNSUPPORTED,
              "pnx_sp3_conv_h: %d -> %d channels over %d taps (channels 1..144, taps 1..27)", cin, cout, taps);
  PNX_REQUIRE(cin_pad == ((cin + 7) & ~7) && cout_pad == ((cout + 7) & ~7), PNX_ERR_INVALID,
              "pnx_sp3_conv_h: padded channel counts %d / %d for %d -> %d channels (each the count rounded up to a multiple of 8)", cin_pad, cout_pad, cin,
              cout);
  PNX_REQUIRE(n_in >= 0 && n_out >= 0 && n_out < ((int64_t)1 << 31), PNX_ERR_INVALID, "pnx_sp3_conv_h: %lld -> %lld rows", (long long)n_in,
              (long long)n_out);
  if (n_out == 0) return PNX_OK;
  PNX_REQUIRE(map && w_packed && shift && y && (n_in == 0 || x), PNX_ERR_INVALID, "pnx_sp3_conv_h: null pointer");
  PNX_REQUIRE((((uintptr_t)x | (uintptr_t)w_packed | (uintptr_t)residual | (uintptr_t)y) & 15) == 0, PNX_ERR_INVALID,
              "pnx_sp3_conv_h: x, w_packed, residual and y must be 16-byte aligned");
  const int cpc = cin_pad / 8, S = (taps * cpc + 3) / 4, nt = (cout + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == PNX_BF16)
    sp3_conv_h_nt<PNX_BF16>(nt, st, x, n_in, cpc, map, n_out, taps, w_packed, S, shift, residual, relu, y, cout, cout_pad);
  else
    sp3_conv_h_nt<PNX_F16>(nt, st, x, n_in, cpc, map, n_out, taps, w_packed, S, shift, residual, relu, y, cout, cout_pad);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_dense_h(const void* feat, int32_t dtype, const int32_t* coords, int64_t n, int32_t channels, int32_t channels_pad, int32_t batch,
                    const int32_t* grid3_host, float* out, pnx_stream_t stream) {
  Sp3Grid g;
  int rc = sp3_grid(batch, grid3_host, &g);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(dtype == PNX_BF16 || dtype == PNX_F16, PNX_ERR_UNSUPPORTED, "pnx_sp3_dense_h: dtype %d (PNX_BF16 or PNX_F16)", dtype);
  PNX_REQUIRE(n >= 0 && channels >= 1 && channels_pad == ((channels + 7) & ~7), PNX_ERR_INVALID,
              "pnx_sp3_dense_h: %lld rows of %d channels padded to %d (the count rounded up to a multiple of 8)", (long long)n, channels, channels_pad);
  const size_t bytes = (size_t)g.B * channels * g.D * g.H * g.W * sizeof(float);
  if (bytes == 0) return PNX_OK;  // a batch of 0 samples
  PNX_REQUIRE(out != nullptr && (n == 0 || (feat && coords && ((uintptr_t)coords & 15) == 0)), PNX_ERR_INVALID, "pnx_sp3_dense_h: null pointer");
  hipStream_t st = (hipStream_t)stream;
  PNX_CHECK_HIP(hipMemsetAsync(out, 0, bytes, st));
  if (n == 0) return PNX_OK;
  if (dtype == PNX_BF16)
    k_sp3_dense_h<PNX_BF16><<<sp3_blocks(n * channels), kBlock, 0, st>>>(feat, coords, n, channels, channels_pad, g, out);
  else
    k_sp3_dense_h<PNX_F16><<<sp3_blocks(n * channels), kBlock, 0, st>>>(feat, coords, n, channels, channels_pad, g, out);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_transpose_map(const int32_t* map, int64_t n_out, int32_t taps, int64_t n_in, int32_t* tmap, pnx_stream_t stream) {
  PNX_REQUIRE(taps >= 1 && taps <= 27 && n_out >= 0 && n_out < ((int64_t)1 << 31) && n_in >= 0 && n_in < ((int64_t)1 << 31), PNX_ERR_INVALID,
              "pnx_sp3_transpose_map: %lld -> %lld rows over %d taps", (long long)n_in, (long long)n_out, taps);
  PNX_REQUIRE((n_in == 0 || tmap != nullptr) && (n_out == 0 || map != nullptr), PNX_ERR_INVALID, "pnx_sp3_transpose_map: null pointer");
  if (n_in == 0) return PNX_OK;
  hipStream_t st = (hipStream_t)stream;
  PNX_CHECK_HIP(hipMemsetAsync(tmap, 0xff, (size_t)n_in * taps * sizeof(int32_t), st));  // every entry -1
  if (n_out == 0) return PNX_OK;
  k_sp3_tmap<<<sp3_blocks(n_out * taps), kBlock, 0, st>>>(map, n_out, taps, n_in, tmap);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

size_t pnx_sp3_wgrad_workspace_bytes(int64_t n_out, int32_t taps, int32_t cin, int32_t cout) {
  if (n_out < 0 || n_out >= ((int64_t)1 << 31) || taps < 1 || taps > 27 || cin < 1 || cin > 144 || cout < 1 || cout > 144) return 0;
  const size_t bytes = (size_t)sp3_wgrad_split(n_out, cout).P * taps * cin * cout * sizeof(float);
  return bytes < 256 ? 256 : bytes;
}

int pnx_sp3_wgrad(const float* x, int64_t n_in, int32_t cin, const float* dy, int32_t cout, const int32_t* map, int64_t n_out, int32_t taps, float* dw,
                  void* workspace, size_t workspace_bytes, pnx_stream_t stream) {
  PNX_REQUIRE(cin >= 1 && cin <= 144 && cout >= 1 && cout <= 144 && taps >= 1 && taps <= 27, PNX_ERR_UNSUPPORTED,
              "pnx_sp3_wgrad: %d -> %d channels over %d taps (channels 1..144, taps 1..27)", cin, cout, taps);
  PNX_REQUIRE(n_in >= 0 && n_out >= 0 && n_out < ((int64_t)1 << 31), PNX_ERR_INVALID, "pnx_sp3_wgrad: %lld -> %lld rows", (long long)n_in, (long long)n_out);
  PNX_REQUIRE(dw != nullptr, PNX_ERR_INVALID, "pnx_sp3_wgrad: dw is NULL");
  hipStream_t st = (hipStream_t)stream;
  const int64_t E = (int64_t)cout * taps * cin;
  if (n_out == 0 || n_in == 0) {
    PNX_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)E * sizeof(float), st));
    return PNX_OK;
  }
  PNX_REQUIRE(x && dy && map && workspace, PNX_ERR_INVALID, "pnx_sp3_wgrad: null pointer");
  PNX_CHECK_WORKSPACE(workspace, workspace_bytes, pnx_sp3_wgrad_workspace_bytes(n_out, taps, cin, cout), "pnx_sp3_wgrad");
  const Sp3WgradSplit sp = sp3_wgrad_split(n_out, cout);
  const dim3 grid((unsigned)sp.P, (unsigned)sp.groups);
  const int nt = (cin + 15) / 16;
  float* part = static_cast<float*>(workspace);
  switch (sp.mt) {
    case 1: sp3_wgrad_nt<1>(nt, grid, st, x, n_in, cin, dy, cout, map, n_out, taps, sp.R, part); break;
    case 2: sp3_wgrad_nt<2>(nt, grid, st, x, n_in, cin, dy, cout, map, n_out, taps, sp.R, part); break;
    default: sp3_wgrad_nt<3>(nt, grid, st, x, n_in, cin, dy, cout, map, n_out, taps, sp.R, part); break;
  }
  PNX_LAUNCH_CHECK();
  k_sp3_wgrad_sum<<<sp3_blocks(E), kBlock, 0, st>>>(part, (int)sp.P, E, dw);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

// the argument checks pnx_sp3_conv_h_f32 and pnx_sp3_wgrad_h share
static int sp3_half_train_args(const char* name, int32_t dtype, int32_t cin, int32_t cin_pad, int32_t cout, int32_t cout_pad, int32_t taps, int64_t n_in,
                               int64_t n_out) {
  PNX_REQUIRE(dtype == PNX_BF16 || dtype == PNX_F16, PNX_ERR_UNSUPPORTED, "%s: dtype %d (PNX_BF16 or PNX_F16)", name, dtype);
  PNX_REQUIRE(cin >= 1 && cin <= 144 && cout >= 1 && cout <= 144 && taps >= 1 && taps <= 27, PNX_ERR_UNSUPPORTED,
              "%s: %d -> %d channels over %d taps (channels 1..144, taps 1..27)", name, cin, cout, taps);
  PNX_REQUIRE(cin_pad == ((cin + 7) & ~7) && cout_pad == ((cout + 7) & ~7), PNX_ERR_INVALID,
              "%s: padded channel counts %d / %d for %d -> %d channels (each the count rounded up to a multiple of 8)", name, cin_pad, cout_pad, cin, cout);
  PNX_REQUIRE(n_in >= 0 && n_in < ((int64_t)1 << 31) && n_out >= 0 && n_out < ((int64_t)1 << 31), PNX_ERR_INVALID, "%s: %lld -> %lld rows", name,
              (long long)n_in, (long long)n_out);
  return PNX_OK;
}

int pnx_sp3_conv_h_f32(const void* x, int64_t n_in, int32_t cin, int32_t cin_pad, const int32_t* map, int64_t n_out, int32_t taps, const void* w_packed,
                       float* y, int32_t cout, int32_t dtype, pnx_stream_t stream) {
  const int cout_pad = (cout + 7) & ~7;
  if (const int rc = sp3_half_train_args("pnx_sp3_conv_h_f32", dtype, cin, cin_pad, cout, cout_pad, taps, n_in, n_out); rc != PNX_OK) return rc;
  if (n_out == 0) return PNX_OK;
  PNX_REQUIRE(map && w_packed && y && (n_in == 0 || x), PNX_ERR_INVALID, "pnx_sp3_conv_h_f32: null pointer");
  PNX_REQUIRE((((uintptr_t)x | (uintptr_t)w_packed) & 15) == 0 && ((uintptr_t)y & 3) == 0, PNX_ERR_INVALID,
              "pnx_sp3_conv_h_f32: x and w_packed must be 16-byte aligned, y 4-byte aligned");
  const int cpc = cin_pad / 8, S = (taps * cpc + 3) / 4, nt = (cout + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == PNX_BF16)
    sp3_conv_h_nt<PNX_BF16, true>(nt, st, x, n_in, cpc, map, n_out, taps, w_packed, S, nullptr, nullptr, 0, y, cout, cout_pad);
  else
    sp3_conv_h_nt<PNX_F16, true>(nt, st, x, n_in, cpc, map, n_out, taps, w_packed, S, nullptr, nullptr, 0, y, cout, cout_pad);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

size_t pnx_sp3_wgrad_h_partials_bytes(int64_t n_out, int32_t taps, int32_t cin, int32_t cout) {
  if (n_out < 0 || n_out >= ((int64_t)1 << 31) || taps < 1 || taps > 27 || cin < 1 || cin > 144 || cout < 1 || cout > 144) return 0;
  return sp3_wgrad_h_carve(nullptr, n_out, taps, cin, cout).bytes;
}

int pnx_sp3_wgrad_h(const void* x, int64_t n_in, int32_t cin, int32_t cin_pad, const void* dy, int32_t cout, int32_t cout_pad, const int32_t* map,
                    int64_t n_out, int32_t taps, float* dw, int32_t dtype, void* partials, size_t partials_bytes, pnx_stream_t stream) {
  if (const int rc = sp3_half_train_args("pnx_sp3_wgrad_h", dtype, cin, cin_pad, cout, cout_pad, taps, n_in, n_out); rc != PNX_OK) return rc;
  PNX_REQUIRE(dw != nullptr, PNX_ERR_INVALID, "pnx_sp3_wgrad_h: dw is NULL");
  hipStream_t st = (hipStream_t)stream;
  const int64_t E = (int64_t)cout * taps * cin;
  if (n_out == 0 || n_in == 0) {
    PNX_CHECK_HIP(hipMemsetAsync(dw, 0, (size_t)E * sizeof(float), st));
    return PNX_OK;
  }
  PNX_REQUIRE(x && dy && map, PNX_ERR_INVALID, "pnx_sp3_wgrad_h: null pointer");
  PNX_REQUIRE((((uintptr_t)x | (uintptr_t)dy) & 15) == 0, PNX_ERR_INVALID, "pnx_sp3_wgrad_h: x and dy must be 16-byte aligned");
  const Sp3WgradHWs ws = sp3_wgrad_h_carve(partials, n_out, taps, cin, cout);
  PNX_CHECK_WORKSPACE(partials, partials_bytes, ws.bytes, "pnx_sp3_wgrad_h");
  const dim3 grid((unsigned)ws.sp.P, (unsigned)ws.sp.groups);
  const int nt = (cin + 15) / 16;
  if (dtype == PNX_BF16)
    sp3_wgrad_h_mt<PNX_BF16>(ws.sp.mt, nt, grid, st, x, n_in, cin, cin_pad / 8, dy, cout, cout_pad / 8, map, n_out, taps, ws.sp.R, ws.part);
  else
    sp3_wgrad_h_mt<PNX_F16>(ws.sp.mt, nt, grid, st, x, n_in, cin, cin_pad / 8, dy, cout, cout_pad / 8, map, n_out, taps, ws.sp.R, ws.part);
  PNX_LAUNCH_CHECK();
  k_sp3_wgrad_sum<<<sp3_blocks(E), kBlock, 0, st>>>(ws.part, (int)ws.sp.P, E, dw);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

// the argument checks the four pnx_sp3_bn_* passes share; *dt = the 16-bit type in play (PNX_F32: none)
static int sp3_bn_args(const char* name, int64_t n, int32_t channels, const void* residual, int32_t residual_dtype, const void* out_h, int32_t dtype,
                       int32_t* dt) {
  PNX_REQUIRE(channels >= 1 && channels <= 256, PNX_ERR_UNSUPPORTED, "%s: %d channels (1..256)", name, channels);
  PNX_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), PNX_ERR_INVALID, "%s: %lld rows", name, (long long)n);
  const bool res_h = residual != nullptr && residual_dtype != PNX_F32;
  PNX_REQUIRE(residual == nullptr || residual_dtype == PNX_F32 || residual_dtype == PNX_BF16 || residual_dtype == PNX_F16, PNX_ERR_UNSUPPORTED,
              "%s: residual dtype %d (PNX_F32, PNX_BF16 or PNX_F16)", name, residual_dtype);
  PNX_REQUIRE(out_h == nullptr || dtype == PNX_BF16 || dtype == PNX_F16, PNX_ERR_UNSUPPORTED, "%s: out_h dtype %d (PNX_BF16 or PNX_F16)", name, dtype);
  PNX_REQUIRE(!(res_h && out_h != nullptr) || residual_dtype == dtype, PNX_ERR_INVALID, "%s: 16-bit residual and out_h must have one dtype", name);
  PNX_REQUIRE(((uintptr_t)residual & 15) == 0 && ((uintptr_t)out_h & 15) == 0, PNX_ERR_INVALID, "%s: rows must be 16-byte aligned", name);
  *dt = res_h ? residual_dtype : (out_h != nullptr ? dtype : PNX_F32);
  return PNX_OK;
}

int pnx_sp3_bn_split(int64_t n, int32_t channels, int32_t* split3_host) {
  PNX_REQUIRE(split3_host && channels >= 1 && channels <= 256 && n >= 0 && n < ((int64_t)1 << 31), PNX_ERR_INVALID,
              "pnx_sp3_bn_split: %lld rows of %d channels (rows < 2^31, channels 1..256)", (long long)n, channels);
  const Sp3BnSplit s = sp3_bn_split(n, channels);
  split3_host[0] = s.blocks, split3_host[1] = s.rpp, split3_host[2] = (int32_t)s.passes;
  return PNX_OK;
}

size_t pnx_sp3_bn_partials_bytes(int64_t n, int32_t channels, int32_t backward) {
  if (n < 0 || n >= ((int64_t)1 << 31) || channels < 1 || channels > 256) return 0;
  return sp3_bn_carve(nullptr, n, channels, backward != 0).bytes;
}

int pnx_sp3_bn_stats(const float* y, int64_t n, int32_t channels, const float* center, float* partials, size_t partials_bytes, pnx_stream_t stream) {
  int32_t dt;
  if (const int rc = sp3_bn_args("pnx_sp3_bn_stats", n, channels, nullptr, PNX_F32, nullptr, PNX_F32, &dt); rc != PNX_OK) return rc;
  const Sp3BnWs ws = sp3_bn_carve(partials, n, channels, false);
  PNX_CHECK_WORKSPACE(partials, partials_bytes, ws.bytes, "pnx_sp3_bn_stats");
  if (n == 0) return PNX_OK;
  PNX_REQUIRE(y && ((uintptr_t)y & 15) == 0, PNX_ERR_INVALID, "pnx_sp3_bn_stats: y is NULL or not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
#define GO(V, DT) k_sp3_bn_stats<V><<<(unsigned)ws.sp.blocks, kBlock, 0, st>>>(y, n, channels, ws.sp.rpp, center, ws.part)
  SP3_BN_DISPATCH(channels, PNX_F32, GO);
#undef GO
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_bn_apply(const float* y, int64_t n, int32_t channels, const float* scale, const float* shift, const void* residual, int32_t residual_dtype,
                     int32_t relu, float* out, void* out_h, int32_t dtype, pnx_stream_t stream) {
  int32_t dt;
  if (const int rc = sp3_bn_args("pnx_sp3_bn_apply", n, channels, residual, residual_dtype, out_h, dtype, &dt); rc != PNX_OK) return rc;
  if (n == 0) return PNX_OK;
  PNX_REQUIRE(y && scale && shift && out && (((uintptr_t)y | (uintptr_t)out) & 15) == 0, PNX_ERR_INVALID,
              "pnx_sp3_bn_apply: null pointer, or rows not 16-byte aligned");
  const Sp3BnSplit sp = sp3_bn_split(n, channels);
  const Sp3BnRes res = {residual_dtype == PNX_F32 ? (const float*)residual : nullptr, residual_dtype == PNX_F32 ? nullptr : residual};
  hipStream_t st = (hipStream_t)stream;
#define GO(V, DT) k_sp3_bn_apply<V, DT><<<(unsigned)sp.blocks, kBlock, 0, st>>>(y, n, channels, sp.rpp, scale, shift, res, relu, out, out_h)
  SP3_BN_DISPATCH(channels, dt, GO);
#undef GO
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_bn_bwd_stats(const float* gout, const float* y, const void* residual, int32_t residual_dtype, int64_t n, int32_t channels, const float* scale,
                         const float* shift, const float* mean, const float* invstd, int32_t relu, float* partials, size_t partials_bytes,
                         pnx_stream_t stream) {
  int32_t dt;
  if (const int rc = sp3_bn_args("pnx_sp3_bn_bwd_stats", n, channels, residual, residual_dtype, nullptr, PNX_F32, &dt); rc != PNX_OK) return rc;
  const Sp3BnWs ws = sp3_bn_carve(partials, n, channels, true);
  PNX_CHECK_WORKSPACE(partials, partials_bytes, ws.bytes, "pnx_sp3_bn_bwd_stats");
  if (n == 0) return PNX_OK;
  PNX_REQUIRE(gout && y && scale && shift && mean && invstd && (((uintptr_t)y | (uintptr_t)gout) & 15) == 0, PNX_ERR_INVALID,
              "pnx_sp3_bn_bwd_stats: null pointer, or rows not 16-byte aligned");
  const Sp3BnRes res = {residual_dtype == PNX_F32 ? (const float*)residual : nullptr, residual_dtype == PNX_F32 ? nullptr : residual};
  hipStream_t st = (hipStream_t)stream;
#define GO(V, DT) \
  k_sp3_bn_bwd_stats<V, DT><<<(unsigned)ws.sp.blocks, kBlock, 0, st>>>(gout, y, res, n, channels, ws.sp.rpp, scale, shift, mean, invstd, relu, ws.part)
  SP3_BN_DISPATCH(channels, dt, GO);
#undef GO
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_bn_bwd_apply(const float* gout, const float* y, const void* residual, int32_t residual_dtype, int64_t n, int32_t channels, const float* scale,
                         const float* shift, const float* mean, const float* invstd, int32_t relu, const float* mean_g, const float* mean_gx, float* dy,
                         float* dresidual, pnx_stream_t stream) {
  int32_t dt;
  if (const int rc = sp3_bn_args("pnx_sp3_bn_bwd_apply", n, channels, residual, residual_dtype, nullptr, PNX_F32, &dt); rc != PNX_OK) return rc;
  if (n == 0) return PNX_OK;
  PNX_REQUIRE(gout && y && scale && shift && mean && invstd && mean_g && mean_gx && dy, PNX_ERR_INVALID, "pnx_sp3_bn_bwd_apply: null pointer");
  PNX_REQUIRE((((uintptr_t)y | (uintptr_t)gout | (uintptr_t)dy | (uintptr_t)dresidual) & 15) == 0, PNX_ERR_INVALID,
              "pnx_sp3_bn_bwd_apply: rows must be 16-byte aligned");
  const Sp3BnSplit sp = sp3_bn_split(n, channels);
  const Sp3BnRes res = {residual_dtype == PNX_F32 ? (const float*)residual : nullptr, residual_dtype == PNX_F32 ? nullptr : residual};
  hipStream_t st = (hipStream_t)stream;
#define GO(V, DT)                                                                                                                                   \
  k_sp3_bn_bwd_apply<V, DT><<<(unsigned)sp.blocks, kBlock, 0, st>>>(gout, y, res, n, channels, sp.rpp, scale, shift, mean, invstd, relu, mean_g, mean_gx, dy, \
                                                                    dresidual)
  SP3_BN_DISPATCH(channels, dt, GO);
#undef GO
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_sp3_dense_backward(const float* dout, const int32_t* coords, int64_t n, int32_t channels, int32_t batch, const int32_t* grid3_host, float* dfeat,
                           pnx_stream_t stream) {
  Sp3Grid g;
  int rc = sp3_grid(batch, grid3_host, &g);
  if (rc != PNX_OK) return rc;
  PNX_REQUIRE(n >= 0 && channels >= 1, PNX_ERR_INVALID, "pnx_sp3_dense_backward: %lld rows of %d channels", (long long)n, channels);
  if (n == 0) return PNX_OK;
  PNX_REQUIRE(dout && dfeat && coords && ((uintptr_t)coords & 15) == 0, PNX_ERR_INVALID, "pnx_sp3_dense_backward: null pointer or coords not 16-byte aligned");
  k_sp3_dense_bwd<<<sp3_blocks(n * channels), kBlock, 0, (hipStream_t)stream>>>(dout, coords, n, channels, g, dfeat);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

}  // extern "C"
