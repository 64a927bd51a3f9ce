// sparse3d_half_train.h -- the 16-bit training form of the sparse 3-D convolution (included by sparse3d.hip, after sparse3d_half.h and the fp32
// weight gradient, whose k_sp3_wgrad_sum it shares):
//   forward and data gradient   k_sp3_conv_h<.., F32 = true> (sparse3d_half.h): the 16-bit gather-GEMM whose fp32 accumulators are the result
//   k_sp3_wgrad_h               dw[co][t][ci] = sum_o dy[o][co] * x[map[o][t]][ci] on v_mfma_f32_16x16x32_{bf16,f16}, fp32 partials
//
// Weight gradient: per tap a (Cout x Cin) GEMM whose K runs over the output rows, 32 per MFMA.  Both operands are row-major with the channel
// contiguous while the MFMA wants K on the lane's eight elements, so each K step stages its 32 dy rows and the 32 x rows the tap gathers in LDS
// (16-byte copies) and reads the fragments back with ds_read_b64_tr_b16: a 16-lane group hands in a [4 rows][16 channels] block and every lane
// gets the 4 rows of ONE channel.  Lane group g takes rows 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3 of the step as its k = 8 g .. 8 g + 7
// -- A and B use the same assignment, so the permutation of K inside a step cancels -- and the LDS row stride is an odd multiple of 32 bytes,
// which puts the 8 rows a 32-lane half reads on 8 different bank groups.  The transposing read wants every lane active and 8-byte aligned
// addresses: a row past the chunk's end, a missing neighbour (map < 0 or >= n_in) and the channels past the padded row are ZERO ROWS / COLUMNS
// in LDS, never a masked lane, and no address is formed from such a map entry.
//
// Rows are dealt statically as in the fp32 kernel: workgroup c owns rows [c R, (c + 1) R) (sp3_wgrad_h_split, R a multiple of 32), its four
// waves take the taps wave, wave + 4, ..., each with its own LDS slab (no workgroup barrier).  A wave walks its chunk in passes: a pass carries
// the accumulators (MT x NT tiles of 16 x 16 each) of as many of its taps as fit its registers at two waves per SIMD (sp3_wgh_taps) -- all 7
// for layers up to 32 x 32 channels, 3 at 48 x 48, 1 at 144 x 144 -- with the K steps as the outer loop and those taps as the inner one, so a step's map entries and dy
// rows are fetched once per pass instead of once per tap and the x rows of the pass's taps are in flight together.  dy is staged as it is (one
// slab serves every tap of the pass); the gathered x rows carry the zeros.  A (tap, K step) none of whose 32 rows has the tap costs no LDS
// traffic and no MFMA, a step none of the pass's taps needs is skipped before anything is loaded.  Whatever the pass width, every element is
// accumulated over the chunk's rows in step order and written to partial c; k_sp3_wgrad_sum adds the partials in index order.  No
// floating-point atomics.
#pragma once

// one 16 x 32 operand fragment: channels 16 tile .. 16 tile + 15 of the staged 32-row slab; `lane_base` = slab + (4 g + q) * stride + 8 p
// for lane 16 g + 4 q + p.  Element e < 4 is row 4 g + e, element 4 + e row 16 + 4 g + e of the slab.
template <int DT, int STRIDE>
__device__ __forceinline__ typename Sp3Half<DT>::v8 sp3_tr_frag(const unsigned char* lane_base, int tile) {
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lane_base + tile * 32));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lane_base + tile * 32 + 16 * STRIDE));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(typename Sp3Half<DT>::v8, v);
}

// taps a wave carries through one pass over its chunk: as many as keep the accumulators (4 MT NT registers a tap) and the x rows in flight
// (4 NT a tap) within about 176 registers, so that two waves per SIMD stay resident without scratch; 7 = all of a wave's taps at 27
constexpr int sp3_wgh_taps(int mt, int nt) { return 176 / (4 * nt * (mt + 1)) >= 7 ? 7 : (176 / (4 * nt * (mt + 1)) >= 1 ? 176 / (4 * nt * (mt + 1)) : 1); }

// x (n_in, 8 cpc_in), dy (n_out, 8 cpc_out) in the 16-bit type DT; partial[c][co][t][ci] = sum over the rows o of chunk c of dy[o][co] * x[map[o][t]][ci]
template <int DT, int MT, int NT>
__global__ __launch_bounds__(kBlock, 2) void k_sp3_wgrad_h(const void* __restrict__ x_, int64_t n_in, int cin, int cpc_in, const void* __restrict__ dy_, int cout,
                                                        int cpc_out, const int32_t* __restrict__ map, int64_t n_out, int T, int R, float* __restrict__ part) {
  using H = Sp3Half<DT>;
  using v8 = typename H::v8;
  constexpr int TW = sp3_wgh_taps(MT, NT);
  constexpr int SX = 32 * (NT | 1), SY = 32 * (MT | 1);  // LDS row strides in bytes: odd multiples of 32
  constexpr int WAVE_LDS = 32 * (SX + SY);
  __shared__ __align__(16) unsigned char lds[(kBlock / 64) * WAVE_LDS];
  const v8* x = static_cast<const v8*>(x_);
  const v8* dy = static_cast<const v8*>(dy_);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, kk = lane >> 4;
  unsigned char* lx = lds + wave * WAVE_LDS;
  unsigned char* ly = lx + 32 * SX;
  const unsigned char* fx = lx + (4 * kk + (r >> 2)) * SX + (r & 3) * 8;
  const unsigned char* fy = ly + (4 * kk + (r >> 2)) * SY + (r & 3) * 8;
  const int srow = lane >> 1, sch = lane & 1;  // staging: two lanes per row, one takes the even 16-byte chunks, one the odd
  const int64_t c = blockIdx.x;
  const int co0 = blockIdx.y * (MT * 16);
  const int64_t row_begin = c * R;
  const int64_t row_end = row_begin + R < n_out ? row_begin + R : n_out;
  const v8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int t0 = wave; t0 < T; t0 += TW * (kBlock / 64)) {  // a pass: the wave's taps t0, t0 + 4, ... (TW of them)
    f32x4 acc[TW][MT][NT];
#pragma unroll
    for (int i = 0; i < TW; i++)
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int j = 0; j < NT; j++) acc[i][m][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t row0 = row_begin; row0 < row_end; row0 += 32) {
      const int64_t row = row0 + srow;
      const bool live = row < row_end;
      int32_t nb[TW];
      bool any = false;
#pragma unroll
      for (int i = 0; i < TW; i++) {
        const int t = t0 + i * (kBlock / 64);
        int32_t v = (live && t < T) ? map[row * T + t] : -1;
        if ((int64_t)v >= n_in) v = -1;
        nb[i] = v;
        any = any || v >= 0;
      }
      if (__ballot(any) == 0) continue;  // wave-uniform: none of the pass's taps has a neighbour in this step -- nothing staged, no MFMA
      v8 xv[TW][NT];  // the x rows of all the pass's taps in flight together; a missing neighbour is a zero row and forms no address
#pragma unroll
      for (int i = 0; i < TW; i++) {
        const v8* xr = x + (int64_t)(nb[i] >= 0 ? nb[i] : 0) * cpc_in;
#pragma unroll
        for (int j = 0; j < NT; j++) xv[i][j] = (nb[i] >= 0 && 2 * j + sch < cpc_in) ? xr[2 * j + sch] : zero8;
      }
      const v8* dr = dy + (live ? row : 0) * cpc_out + co0 / 8;
#pragma unroll
      for (int i = 0; i < MT; i++) {  // the same trip count in every lane
        const int ch = 2 * i + sch;
        *reinterpret_cast<v8*>(ly + srow * SY + ch * 16) = (live && co0 / 8 + ch < cpc_out) ? dr[ch] : zero8;
      }
      __builtin_amdgcn_wave_barrier();  // the slab is the wave's own: its LDS accesses execute in order, this only pins the compiler's
      v8 a[MT];
#pragma unroll
      for (int m = 0; m < MT; m++) a[m] = sp3_tr_frag<DT, SY>(fy, m);
#pragma unroll
      for (int i = 0; i < TW; i++) {
        if (__ballot(nb[i] >= 0) == 0) continue;  // wave-uniform (taps past T included): no row of the step has this tap
#pragma unroll
        for (int j = 0; j < NT; j++) *reinterpret_cast<v8*>(lx + srow * SX + (2 * j + sch) * 16) = xv[i][j];
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const v8 b = sp3_tr_frag<DT, SX>(fx, j);
#pragma unroll
          for (int m = 0; m < MT; m++) {
            if (co0 + m * 16 >= cout) continue;  // uniform: a channel tile past the layer's last
            acc[i][m][j] = H::mfma(a[m], b, acc[i][m][j]);
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int i = 0; i < TW; i++) {
      const int t = t0 + i * (kBlock / 64);
      if (t >= T) continue;
#pragma unroll
      for (int m = 0; m < MT; m++)
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const int ci = j * 16 + r;
          if (ci >= cin) continue;
#pragma unroll
          for (int e = 0; e < 4; e++) {
            const int co = co0 + m * 16 + kk * 4 + e;
            if (co < cout) part[(((int64_t)c * cout + co) * T + t) * cin + ci] = acc[i][m][j][e];
          }
        }
    }
  }
}

// The static split: output-channel tiles per wave (MT, as the fp32 kernel), rows per workgroup R (a multiple of the K step of 32, 256 .. 4096)
// and the number of partials P = ceil(n_out / R).
struct Sp3WgradHSplit {
  int mt, groups, R;
  int64_t P;
};

inline Sp3WgradHSplit sp3_wgrad_h_split(int64_t n_out, int cout) {
  Sp3WgradHSplit s;
  const int tiles = (cout + 15) / 16;
  s.mt = tiles <= 3 ? tiles : (tiles % 3 == 0 ? 3 : (tiles % 2 == 0 ? 2 : 3));
  s.groups = (tiles + s.mt - 1) / s.mt;
  const int64_t p0 = 256 / s.groups > 1 ? 256 / s.groups : 1;
  int64_t R = ((n_out + p0 - 1) / p0 + 31) & ~(int64_t)31;
  R = R < 256 ? 256 : (R > 4096 ? 4096 : R);
  s.R = (int)R;
  s.P = n_out > 0 ? (n_out + R - 1) / R : 0;
  return s;
}

// the partials buffer: one carve for the size query and the launch
struct Sp3WgradHWs {
  Sp3WgradHSplit sp;
  float* part;
  size_t bytes;
};

inline Sp3WgradHWs sp3_wgrad_h_carve(void* base, int64_t n_out, int taps, int cin, int cout) {
  Sp3WgradHWs w;
  w.sp = sp3_wgrad_h_split(n_out, cout);
  PnxCarver c(base);
  w.part = c.take<float>((size_t)w.sp.P * taps * cin * cout);
  w.bytes = c.used() < 256 ? 256 : c.used();
  return w;
}

template <int DT, int MT, int NT>
void sp3_wgrad_h_launch(dim3 grid, hipStream_t st, const void* x, int64_t n_in, int cin, int cpc_in, const void* dy, int cout, int cpc_out, const int32_t* map,
                        int64_t n_out, int T, int R, float* part) {
  k_sp3_wgrad_h<DT, MT, NT><<<grid, kBlock, 0, st>>>(x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part);
}

template <int DT, int MT>
void sp3_wgrad_h_nt(int nt, dim3 grid, hipStream_t st, const void* x, int64_t n_in, int cin, int cpc_in, const void* dy, int cout, int cpc_out,
                    const int32_t* map, int64_t n_out, int T, int R, float* part) {
  switch (nt) {
    case 1: sp3_wgrad_h_launch<DT, MT, 1>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 2: sp3_wgrad_h_launch<DT, MT, 2>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 3: sp3_wgrad_h_launch<DT, MT, 3>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 4: sp3_wgrad_h_launch<DT, MT, 4>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 5: sp3_wgrad_h_launch<DT, MT, 5>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 6: sp3_wgrad_h_launch<DT, MT, 6>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 7: sp3_wgrad_h_launch<DT, MT, 7>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 8: sp3_wgrad_h_launch<DT, MT, 8>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    default: sp3_wgrad_h_launch<DT, MT, 9>(grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
  }
}

template <int DT>
void sp3_wgrad_h_mt(int mt, int nt, dim3 grid, hipStream_t st, const void* x, int64_t n_in, int cin, int cpc_in, const void* dy, int cout, int cpc_out,
                    const int32_t* map, int64_t n_out, int T, int R, float* part) {
  switch (mt) {
    case 1: sp3_wgrad_h_nt<DT, 1>(nt, grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    case 2: sp3_wgrad_h_nt<DT, 2>(nt, grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
    default: sp3_wgrad_h_nt<DT, 3>(nt, grid, st, x, n_in, cin, cpc_in, dy, cout, cpc_out, map, n_out, T, R, part); break;
  }
}
