// sephead.h -- the dense SepHead kernels (included by conv3x3.hip after conv_s2.h): the deblock's transposed convolution k_deconv2x2_64 and the
// block-diagonal closing convolution k_sephead_out with launch_sephead.  The lazy head (candidate cells only) is sephead_lazy.h.
#pragma once

// ---- ConvTranspose2d(64, 64, kernel 2, stride 2) + folded BN + ReLU: the deblock of every SepHead (det3d/models/heads/centerhead.py:17-21).
// Kernel == stride, so the four output parities (ky, kx) are four independent 1x1 convolutions of the input pixel: per 32 input
// pixels 4 x (2 output-channel tiles x 4 k-steps) MFMAs and four 128-byte output lines per pixel, written as complete lines (the
// epilogue of conv_tile.h with a pixel stride of two).  Weights (32 KB, fragment order) stay in registers of the persistent waves.
__global__ __launch_bounds__(256, 2) void k_deconv2x2_64(const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag, const float* __restrict__ bias,
                                                      uint16_t* __restrict__ y, int B, int H, int W, int relu) {
  constexpr int C = 64;
  const int lane = threadIdx.x & 63, px = lane & 31, kb = lane >> 5;
  uint4 w[4][4][2];  // [parity][k-step][output-channel tile]
#pragma unroll
  for (int p = 0; p < 4; p++)
#pragma unroll
    for (int ks = 0; ks < 4; ks++)
#pragma unroll
      for (int m = 0; m < 2; m++) w[p][ks][m] = wfrag[((p * 4 + ks) * 2 + m) * 64 + lane];
  v16f bq[2];
#pragma unroll
  for (int m = 0; m < 2; m++) bq[m] = bias_tile(bias, m * 32, kb);
  const int segs = (W + 31) >> 5;
  const int64_t n_seg = (int64_t)B * H * segs;
  const int Wo = 2 * W;
  for (int64_t sg = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); sg < n_seg; sg += (int64_t)gridDim.x * 4) {
    const int sx = (int)(sg % segs);
    const int64_t row = sg / segs;  // b * H + y
    const int x0 = sx * 32, n_valid = W - x0;
    const bool in = x0 + px < W;
    const uint16_t* src = x + (row * W + (in ? x0 + px : x0)) * C + 8 * kb;
    uint4 q[4];
#pragma unroll
    for (int ks = 0; ks < 4; ks++) q[ks] = in ? *reinterpret_cast<const uint4*>(src + ks * 16) : make_uint4(0, 0, 0, 0);
    const int b = (int)(row / H), yy = (int)(row - (int64_t)b * H);
#pragma unroll
    for (int p = 0; p < 4; p++) {
      v16f acc[2] = {bq[0], bq[1]};
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        const el8 bfr = __builtin_bit_cast(el8, q[ks]);
#pragma unroll
        for (int m = 0; m < 2; m++) acc[m] = PNX_MFMA32(__builtin_bit_cast(el8, w[p][ks][m]), bfr, acc[m]);
      }
      uint4 D[4];
#pragma unroll
      for (int m = 0; m < 2; m++) {
        uint4 pk[2];
        pack_tile(acc[m], true, relu, pk);
        D[2 * m] = pk[0], D[2 * m + 1] = pk[1];
      }
      transpose_row64(D, lane);
      uint16_t* orow = y + ((((int64_t)b * 2 * H + 2 * yy + (p >> 1)) * Wo) + 2 * x0 + (p & 1)) * C;
      store_row64<2 * C>(D, orow, n_valid, lane);  // output pixel of input pixel P: 2 P + kx -> a pixel stride of 2 x 64 channels
    }
  }
}

// ---- final convolution of the merged SepHead branches (det3d/models/heads/centerhead.py:12-59: Conv2d(64, k_j, 3) of every
// branch j of a task).  The first (merged) convolution leaves NBR x 64 channels per pixel; branch j reads only its own 64, so
// the stacked weight (sum k_j <= 16 outputs x NBR*64 inputs) is block diagonal.  HBM-bound by its input (768 B per pixel at
// NBR = 6 against 32 B of output): the 64-channel slabs are staged through LDS one after the other (each pixel is read from
// HBM/L2 once instead of 9 times) and accumulated on v_mfma_f32_16x16x32_bf16 with M = the 16 output channels, N = 16 pixels;
// the D fragment (lane = pixel n + 16 q: channels 4q..4q+3) stores 8 bytes per lane, 512 contiguous bytes per instruction.
// wfrag: [branch][tap][kc][lane = q*16 + o][8]: W[o][branch*64 + kc*32 + q*8 + e][ky][kx] (ops.py::sephead_pack_weights).
typedef float v4f __attribute__((ext_vector_type(4)));
template <int NBR, int TH>
__global__ __launch_bounds__(256) void k_sephead_out(const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag, const float* __restrict__ bias,
                                                     uint16_t* __restrict__ y, int B, int H, int W) {
  constexpr int CIN = NBR * 64, HW_ = LDS_HW, RW = TH / 4;  // RW rows per wave
  __shared__ uint4 s_in[(TH + 2) * LDS_HW * 8];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 15, q = lane >> 4;
  const float4 bq = *reinterpret_cast<const float4*>(bias + 4 * q);
  const int tiles_x = (W + 31) >> 5, tiles_y = (H + TH - 1) / TH;
  const int64_t n_tiles = (int64_t)B * tiles_y * tiles_x;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int tx = (int)(tile % tiles_x);
    const int ty = (int)((tile / tiles_x) % tiles_y);
    const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
    const int x0 = tx * 32, y0 = ty * TH;
    v4f acc[RW][2];
#pragma unroll
    for (int r = 0; r < RW; r++)
#pragma unroll
      for (int h = 0; h < 2; h++) acc[r][h] = v4f{bq.x, bq.y, bq.z, bq.w};
#pragma unroll 1
    for (int j = 0; j < NBR; j++) {
      __syncthreads();  // everybody is done reading the previous slab
      stage_tile64<CIN, TH>(s_in, x, b, H, W, j * 64, y0, x0, (1u << (TH + 2)) - 1u);
      __syncthreads();
      const uint4* wj = wfrag + (size_t)j * 18 * 64 + lane;
      uint4 wn[2] = {wj[0], wj[64]};
#pragma unroll 1
      for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3, dx = tap - 3 * dy;  // halo coordinates: +1 already included
        const uint4 wc[2] = {wn[0], wn[1]};
        if (tap < 8) wn[0] = wj[(tap + 1) * 128], wn[1] = wj[(tap + 1) * 128 + 64];
#pragma unroll
        for (int kc = 0; kc < 2; kc++) {
          uint4 bf[RW][2];
#pragma unroll
          for (int r = 0; r < RW; r++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
              const int c = 16 * h + n + dx;
              bf[r][h] = s_in[((wv * RW + r + dy) * HW_ + c) * 8 + ((kc * 4 + q) ^ lds_swz(c))];
            }
#pragma unroll
          for (int r = 0; r < RW; r++)
#pragma unroll
            for (int h = 0; h < 2; h++)
              acc[r][h] = PNX_MFMA16(__builtin_bit_cast(el8, wc[kc]), __builtin_bit_cast(el8, bf[r][h]), acc[r][h]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < RW; r++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int oy = y0 + wv * RW + r, ox = x0 + 16 * h + n;
        if (oy < H && ox < W) {
          uint2 p;
          p.x = pack_el(acc[r][h][0], acc[r][h][1]);
          p.y = pack_el(acc[r][h][2], acc[r][h][3]);
          *reinterpret_cast<uint2*>(y + (((int64_t)b * H + oy) * W + ox) * 16 + 4 * q) = p;
        }
      }
  }
}

template <int NBR>
int launch_sephead(const void* x, const void* wfrag, const float* bias, void* y, int B, int H, int W, hipStream_t st) {
  constexpr int TH = 8;  // 8-row tiles: 43.5 KiB of LDS, 3 workgroups per CU (4 and 16 rows measured slower in round 2)
  int64_t nb = (int64_t)B * ((H + TH - 1) / TH) * ((W + 31) / 32);
  if (nb > 768) nb = 768;  // resident workgroups
  k_sephead_out<NBR, TH><<<(unsigned)nb, 256, 0, st>>>((const uint16_t*)x, (const uint4*)wfrag, bias, (uint16_t*)y, B, H, W);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}
