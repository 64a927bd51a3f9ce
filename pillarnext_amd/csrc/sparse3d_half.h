// sparse3d_half.h -- the 16-bit inference form of the sparse 3-D convolution (included by sparse3d.hip, after its Sp3Grid / sp3_row):
//   k_sp3_conv_h   gather-GEMM on v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulators, + folded BN shift (+ residual) (+ ReLU), one rounding
//   k_sp3_dense_h  padded 16-bit rows -> the fp32 (B, C*D, H, W) map
//
// Rows are stored in the 16-bit type with the channel count padded to a multiple of 8 (cpad), pad columns exactly zero, so a row is a
// whole number of 16-byte chunks.  K is flattened over (tap, padded channel) and cut into chunks of 8: chunk q = tap * cpc + c8 with
// cpc = cpad / 8.  A K step of 32 is four chunks; lane l of the wave (r = l & 15, kk = l >> 4) owns chunk 4 s + kk of output row r, which
// is ONE 16-byte load from ONE neighbour row -- at cpad 16 a step covers two taps, at cpad 8 four.  That fragment (row l & 15,
// k = 8 (l >> 4) + j) is the instruction's A layout and, the two operand layouts being mirror images, its B layout as well: the kernel
// feeds the weights as A and the rows as B, so the accumulator comes out transposed -- lane l holds output row l & 15 and the four
// CONSECUTIVE channels 16 j + 4 kk + i -- and the epilogue reads the residual and stores the result 8 bytes at a time.
//
// Weights: the host packs them once (ops.sp3_pack_weight_h) in fragment order [step][channel tile j][lane][8], value
// w'[tap][8 c8 + e][16 j + (lane & 15)] for chunk 4 step + (lane >> 4), zero past the last chunk / channel: one 16-byte load per lane and
// MFMA.  Where the whole layer fits 64 KiB they are staged in LDS once per workgroup, which then walks row tiles persistently; otherwise
// they stream from L2.  The staging barrier is the kernel's only one and no wave returns before it.
//
// A map entry that is negative or >= n_in contributes zero: the operand is zeroed and no address is formed from it.  A K step none of the
// wave's 16 rows has a neighbour in costs no MFMA and no weight load (wave-uniform __ballot).
#pragma once

template <int DT>
struct Sp3Half;
template <>
struct Sp3Half<PNX_BF16> {
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  typedef __bf16 v4 __attribute__((ext_vector_type(4)));
  typedef __bf16 el;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};
template <>
struct Sp3Half<PNX_F16> {
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  typedef _Float16 v4 __attribute__((ext_vector_type(4)));
  typedef _Float16 el;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};

constexpr int kSp3HalfUnroll = 4;          // K steps whose map entries and rows are fetched together
constexpr size_t kSp3HalfLdsMax = 65536;   // weights up to this size are staged in LDS (no opt-in needed)

// x (n_in, 8 cpc), y / res (n_out, cout_pad), wf (S, NT, 64, 8) in the 16-bit type DT; S = ceil(T cpc / 4) K steps; ntiles = ceil(n_out / 64).
// F32 (training, sparse3d_half_train.h): y is (n_out, cout) fp32 and receives the accumulators as they are -- no shift, residual, ReLU or rounding.
template <int DT, int NT, bool LDS, bool F32 = false>
__global__ __launch_bounds__(kBlock) void k_sp3_conv_h(const void* __restrict__ x_, int64_t n_in, int cpc, const int32_t* __restrict__ map, int64_t n_out, int T,
                                                       const void* __restrict__ wf_, int S, const float* __restrict__ shift, const void* __restrict__ res_,
                                                       int relu, void* __restrict__ y_, int cout, int cout_pad, int64_t ntiles) {
  extern __shared__ __align__(16) unsigned char sp3_half_lds[];
  using H = Sp3Half<DT>;
  using v8 = typename H::v8;
  using v4 = typename H::v4;
  using el = typename H::el;
  constexpr int U = kSp3HalfUnroll;
  const el* x = static_cast<const el*>(x_);
  const el* res = static_cast<const el*>(res_);
  el* y = static_cast<el*>(y_);
  const v8* wf = static_cast<const v8*>(wf_);
  if constexpr (LDS) {
    v8* l = reinterpret_cast<v8*>(sp3_half_lds);
    for (int i = threadIdx.x; i < S * NT * 64; i += kBlock) l[i] = wf[i];
    __syncthreads();  // the only barrier; every wave of the workgroup reaches it (no return above, none below it matters)
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kk = lane >> 4;
  const int Q = T * cpc, in_ld = cpc * 8;
  const uint32_t magic = 65536u / (uint32_t)cpc + 1u;  // q / cpc == (q * magic) >> 16 for q * cpc < 65536 (q < 27 * 18, cpc <= 18)
  const v8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (tile * (kBlock / 64) + wave) * 16;
    if (row0 >= n_out) continue;  // wave-uniform; the barrier is behind us
    const int64_t row = row0 + r;
    const bool live = row < n_out;
    const int32_t* mrow = map + (live ? row : 0) * T;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < S; s0 += U) {
      int32_t nb[U];
      int c8[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int q = 4 * (s0 + u) + kk;
        const int tap = (int)(((uint32_t)q * magic) >> 16);
        c8[u] = q - tap * cpc;
        int32_t v = (live && q < Q) ? mrow[tap] : -1;  // q < Q: tap < T
        if ((int64_t)v >= n_in) v = -1;
        nb[u] = v;
      }
      v8 b[U];
#pragma unroll
      for (int u = 0; u < U; u++) b[u] = nb[u] >= 0 ? *reinterpret_cast<const v8*>(x + (int64_t)nb[u] * in_ld + c8[u] * 8) : zero8;
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (__ballot(nb[u] >= 0) == 0) continue;  // no row of the tile has a neighbour in this K step (steps past S included): no MFMA
        const int f = ((s0 + u) * NT) * 64 + lane;
#pragma unroll
        for (int j = 0; j < NT; j++) {
          v8 a;
          if constexpr (LDS)
            a = reinterpret_cast<const v8*>(sp3_half_lds)[f + j * 64];
          else
            a = wf[f + j * 64];
          acc[j] = H::mfma(a, b[u], acc[j]);
        }
      }
    }
    if (!live) continue;
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const int c0 = j * 16 + kk * 4;  // acc[j][i] = output row r, channel c0 + i
      if (c0 >= cout_pad) continue;    // cout_pad is a multiple of 8: a group of four is inside the padded row or outside it
      f32x4 v = acc[j];
      if constexpr (F32) {
        float* yf = static_cast<float*>(y_) + row * cout + c0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (c0 + i < cout) yf[i] = v[i];
        continue;
      }
#pragma unroll
      for (int i = 0; i < 4; i++) v[i] += c0 + i < cout ? shift[c0 + i] : 0.f;
      if (res) {
        const f32x4 rv = __builtin_convertvector(*reinterpret_cast<const v4*>(res + row * cout_pad + c0), f32x4);
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] += rv[i];
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        if (relu && v[i] < 0.f) v[i] = 0.f;
        if (c0 + i >= cout) v[i] = 0.f;  // pad columns are exactly zero
      }
      *reinterpret_cast<v4*>(y + row * cout_pad + c0) = __builtin_convertvector(v, v4);  // the one rounding (nearest even)
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kBlock) void k_sp3_dense_h(const void* __restrict__ feat_, const int32_t* __restrict__ coords, int64_t n, int C, int cpad,
                                                        Sp3Grid g, float* __restrict__ out) {
  const typename Sp3Half<DT>::el* feat = static_cast<const typename Sp3Half<DT>::el*>(feat_);
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n * C) return;
  const int64_t i = e / C;
  const int ch = (int)(e - i * C);
  int c[4];
  if (!sp3_row(coords, i, g, c)) return;
  out[((((int64_t)c[0] * C + ch) * g.D + c[1]) * g.H + c[2]) * g.W + c[3]] = (float)feat[i * cpad + ch];
}

// workgroups of the persistent (LDS) form: as many as stay resident -- by LDS (160 KiB per CU) and by waves (8 workgroups of 4 per CU)
inline int sp3_half_cus() {
  static std::atomic<int> cus[kPnxMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kPnxMaxDevices) return 256;
  int n = cus[dev].load(std::memory_order_relaxed);
  if (n == 0) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

template <int DT, int NT, bool F32 = false>
void sp3_conv_h_launch(hipStream_t st, const void* x, int64_t n_in, int cpc, const int32_t* map, int64_t n_out, int T, const void* wf, int S,
                       const float* shift, const void* res, int relu, void* y, int cout, int cout_pad) {
  const int64_t ntiles = (n_out + 63) / 64;
  const size_t wbytes = (size_t)S * NT * 1024;
  if (wbytes <= kSp3HalfLdsMax) {
    const int64_t per_cu = std::min<int64_t>(8, (160 * 1024) / (int64_t)wbytes);
    const int64_t nb = std::min<int64_t>(ntiles, per_cu * sp3_half_cus());
    k_sp3_conv_h<DT, NT, true, F32><<<(unsigned)nb, kBlock, wbytes, st>>>(x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad, ntiles);
  } else {
    k_sp3_conv_h<DT, NT, false, F32><<<(unsigned)ntiles, kBlock, 0, st>>>(x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad, ntiles);
  }
}

template <int DT, bool F32 = false>
void sp3_conv_h_nt(int nt, hipStream_t st, const void* x, int64_t n_in, int cpc, const int32_t* map, int64_t n_out, int T, const void* wf, int S,
                   const float* shift, const void* res, int relu, void* y, int cout, int cout_pad) {
  switch (nt) {
    case 1: sp3_conv_h_launch<DT, 1, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 2: sp3_conv_h_launch<DT, 2, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 3: sp3_conv_h_launch<DT, 3, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 4: sp3_conv_h_launch<DT, 4, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 5: sp3_conv_h_launch<DT, 5, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 6: sp3_conv_h_launch<DT, 6, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 7: sp3_conv_h_launch<DT, 7, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    case 8: sp3_conv_h_launch<DT, 8, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
    default: sp3_conv_h_launch<DT, 9, F32>(st, x, n_in, cpc, map, n_out, T, wf, S, shift, res, relu, y, cout, cout_pad); break;
  }
}
