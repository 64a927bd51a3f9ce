// sephead_lazy.h -- k_sephead_lazy and its arguments (included by conv3x3.hip after the entry points of the other kernels; the entry point
// pnx_sephead_lazy follows the include there).
//
// Lazy SepHead (models.FusedPillarNeXt): the five regression branches of a task (reg, height, dim, rot, vel: conv3x3 64 -> 64 + BN +
// ReLU, then conv3x3 64 -> k each; det3d/models/heads/centerhead.py:12-59) evaluated ONLY at the candidate cells the decoder selected
// (<= pre_max per sample and class, centerhead.py:341-363) instead of at every cell: 5/6 of the head's convolution work and its
// 384-channel intermediate (9.6 GB of HBM traffic per 8-frame step) shrink to ~8 % of the cells.
// One launch covers every task.  One workgroup (8 waves) = 32 consecutive candidates of one (sample, class) list.  The 5 x 5 x 64 input
// patch of every candidate is staged in LDS (swizzled 16-byte chunks); the first convolution is an implicit GEMM on
// v_mfma_f32_32x32x16_bf16 with M = 320 output channels (10 tiles), N = 32 candidates x 9 neighbour positions = 288 pixels (9 tiles),
// K = 9 taps x 64 channels, dealt to the waves as 15 items (branch = 2 M tiles) x (3 N tiles); its outputs are rounded to bf16 like the
// dense kernel's intermediate and contracted on the spot with the second convolution's weights of their branch (the intermediate never
// exists); per-(pixel, branch) partial sums go through LDS and are added in a fixed order: deterministic.
// The kLz* sizes are shared with the entry point and stand in conv3x3.hip, right before the include.
#pragma once

struct LazyTaskDev {
  const uint16_t* up;
  const uint4* wfrag;
  const float *b1, *w2c, *b2;
  int h, w;
};
struct LazyArgs {
  LazyTaskDev t[kLzMaxTasks];
  signed char class_task[kLzMaxClasses];
  int nc_total, pre_max, bps;
};

__global__ __launch_bounds__(512) void k_sephead_lazy(const LazyArgs A, const int64_t* __restrict__ local, const int32_t* __restrict__ seg_len,
                                                      float* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char s_lz[];
  uint4* s_patch = reinterpret_cast<uint4*>(s_lz);                                    // [cand][cell 25][chunk 8 ^ swz]
  float* s_w2 = reinterpret_cast<float*>(s_patch + kLzPatch);                         // [M tile 10][pos 9][channel 32][3]
  float* s_part = s_w2 + kLzW2;                                                       // [pixel 288][branch 5][3]
  int* s_cell = reinterpret_cast<int*>(s_part + kLzN * 5 * 3);                        // [cand]: b*H*W + cell, or -1
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, px = lane & 31, kb = lane >> 5;
  const int seg = blockIdx.x / A.bps, c0 = (blockIdx.x - seg * A.bps) * kLzG;
  const int len = seg_len[seg];
  const int rows = min(kLzG, A.pre_max - c0);
  float* const outp = out + ((int64_t)seg * A.pre_max + c0) * 10;
  if (c0 >= len) {  // behind the end of the list: zero rows, no work
    for (int i = t; i < rows * 10; i += 512) outp[i] = 0.f;
    return;
  }
  const LazyTaskDev T = A.t[A.class_task[seg % A.nc_total]];
  CT_DECL
  const int H = T.h, W = T.w, HW = H * W;
  if (t < kLzG) s_cell[t] = (c0 + t < len) ? (int)local[(int64_t)seg * A.pre_max + c0 + t] : -1;
  for (int e = t; e < kLzW2 / 4; e += 512) reinterpret_cast<float4*>(s_w2)[e] = reinterpret_cast<const float4*>(T.w2c)[e];
  __syncthreads();
  CT_TOCK(0)
  // ---- stage the 5 x 5 patches (zeros outside the map / for the slots behind the end of the list): all of a thread's 16-byte
  // gathers are in flight before the first LDS write (one after the other they cost a memory latency each)
  {
    constexpr int NP = (kLzPatch + 511) / 512;
    uint4 v[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) {
      const int e = t + k * 512;
      const int q = e & 7, cell = (e >> 3) % 25, c = min(e / 200, kLzG - 1);
      const int lc = s_cell[c];
      v[k] = make_uint4(0, 0, 0, 0);
      if (lc >= 0 && e < kLzPatch) {
        const int b = lc / HW, rem = lc - b * HW;
        const int y = rem / W + cell / 5 - 2, x = rem % W + cell % 5 - 2;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W)
          v[k] = *reinterpret_cast<const uint4*>(T.up + (((int64_t)b * H + y) * W + x) * 64 + q * 8);
      }
    }
#pragma unroll
    for (int k = 0; k < NP; k++) {
      const int e = t + k * 512;
      const int q = e & 7, cell = (e >> 3) % 25, c = e / 200;
      if (e < kLzPatch) s_patch[(c * 25 + cell) * 8 + (q ^ (cell & 7))] = v[k];
    }
  }
  CT_TOCK(1)
  __syncthreads();
  CT_TOCK(2)
#pragma unroll 1
  for (int item = wv; item < 15; item += 8) {
    const int br = item / 3, g0 = (item - br * 3) * 3;
    int pb[3], wc[3], posv[3];
    bool inside[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int pix = (g0 + j) * 32 + px;
      const int cand = pix / 9, pos = pix - cand * 9;
      posv[j] = pos;
      wc[j] = (pos / 3) * 5 + (pos % 3);  // top-left cell of this pixel's 3 x 3 window inside the 5 x 5 patch
      pb[j] = cand * 25 * 8;
      const int lc = s_cell[cand];
      inside[j] = lc >= 0;
      if (inside[j]) {
        const int rem = lc % HW;
        const int y = rem / W + pos / 3 - 1, x = rem % W + pos % 3 - 1;
        inside[j] = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
      }
    }
    float ps[3][3] = {};
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
      const int mt = 2 * br + half;
      v16f acc[3];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const float bq = T.b1[mt * 32 + 8 * (i >> 2) + 4 * kb + (i & 3)];
#pragma unroll
        for (int j = 0; j < 3; j++) acc[j][i] = bq;
      }
      // Weight fragments (L2): kLzAhead taps ahead in straight-line code.  A tap is 12 MFMAs (~400 cycles) per wave; with one tap of lookahead
      // in a rolled loop the k-steps ran at the latency of their fragment loads (the kernel took 620 us for 2.6 M MFMAs = 110 us of pipe time).
      const uint4* wp = T.wfrag + mt * 64 + lane;
      uint4 wq[9][4];
#pragma unroll
      for (int tp = 0; tp < kLzAhead; tp++)
#pragma unroll
        for (int ks = 0; ks < 4; ks++) wq[tp][ks] = wp[(tp * 4 + ks) * 640];
#pragma unroll
      for (int tap = 0; tap < 9; tap++) {
        if (tap + kLzAhead < 9) {
          const uint4* wpt = wp;
          asm volatile("" : "+v"(wpt));  // the loads of a later tap are not hoisted to the top (144 live registers)
#pragma unroll
          for (int ks = 0; ks < 4; ks++) wq[tap + kLzAhead][ks] = wpt[((tap + kLzAhead) * 4 + ks) * 640];
        }
        const int toff = (tap / 3) * 5 + (tap % 3);
        int cwj[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
          cwj[j] = wc[j] + toff;
          asm volatile("" : "+v"(cwj[j]));  // recomputed per tap: hoisted out of the loops, the 108 LDS addresses of an item spill
        }
#pragma unroll
        for (int ks = 0; ks < 4; ks++) {
#pragma unroll
          for (int j = 0; j < 3; j++) {
            const int cw = cwj[j];
            const uint4 bq4 = s_patch[pb[j] + cw * 8 + ((ks * 2 + kb) ^ (cw & 7))];
            acc[j] = PNX_MFMA32(__builtin_bit_cast(el8, wq[tap][ks]), __builtin_bit_cast(el8, bq4), acc[j]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);  // keeps the fragment loads where they are: kLzAhead taps ahead, not all at the top (registers)
      }
      CT_TOCK(3)
      // ---- ReLU, bf16 rounding (the dense kernel's intermediate), contraction with the second convolution
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const float* w2p = s_w2 + ((mt * 9 + posv[j]) * 32 + 4 * kb) * 3;
#pragma unroll
        for (int i = 0; i < 16; i++) {
          const float tv = inside[j] ? round_el(fmaxf(acc[j][i], 0.f)) : 0.f;
          const float* w = w2p + (8 * (i >> 2) + (i & 3)) * 3;
          ps[j][0] = __builtin_fmaf(tv, w[0], ps[j][0]);
          ps[j][1] = __builtin_fmaf(tv, w[1], ps[j][1]);
          ps[j][2] = __builtin_fmaf(tv, w[2], ps[j][2]);
        }
      }
      CT_TOCK(4)
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int pix = (g0 + j) * 32 + px;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const float v = ps[j][q] + __shfl_xor(ps[j][q], 32);  // the other half of the wave holds the other 16 channels of each tile
        if (kb == 0) s_part[(pix * 5 + br) * 3 + q] = v;
      }
    }
  }
  CT_TOCK(5)
  __syncthreads();
  CT_TOCK(6)
  // ---- out[cand][o] = b2[o] + sum over the 9 positions of the output's branch, in a fixed order; rounded to bf16
  for (int e = t; e < rows * 10; e += 512) {
    const int cand = e / 10, o = e - cand * 10;
    const int br = o < 2 ? 0 : (o < 3 ? 1 : (o < 6 ? 2 : (o < 8 ? 3 : 4)));
    const int q = o - (br == 0 ? 0 : (br == 1 ? 2 : (br == 2 ? 3 : (br == 3 ? 6 : 8))));
    float s = 0.f;
    if (s_cell[cand] >= 0) {
      s = T.b2[o];
      for (int pos = 0; pos < 9; pos++) s += s_part[((cand * 9 + pos) * 5 + br) * 3 + q];
      s = round_el(s);
    }
    outp[e] = s;
  }
  CT_TOCK(7)
  CT_FLUSH
}

constexpr size_t kLzLds = (size_t)kLzPatch * 16 + (size_t)kLzW2 * 4 + (size_t)kLzN * 5 * 3 * 4 + kLzG * 4;
static_assert(kLzLds <= 160 * 1024, "k_sephead_lazy: LDS budget");
