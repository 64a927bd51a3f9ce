// conv_s2.h -- the stride-2 kernel k_conv3x3_s2 with its staging (stage_tile64_s2), its per-wave body (conv_rows_s2) and launch_s2 (included by
// conv3x3.hip after conv_rows.h).  Serves the bf16 / fp16 inference entry and, with 2 or 3 bf16 pieces per operand, the fp32 training entries.
#pragma once

// ---- stride 2 (the entry convolution of backbone stages 1-3: 64 -> 128, 128 -> 256, 256 -> 256; sparse_resnet.py:50-68, SparseConv2d).
// Output tile 4 rows x 32 pixels; its 9 x 65 input halo of one 64-channel slab is staged de-interleaved (even columns, then odd
// columns) so that the tap loop (conv_taps.h) reads consecutive slots.  74.9 KB of LDS: 2 workgroups per CU.
constexpr int S2_TH = 4;
constexpr int S2_ROWS = 2 * S2_TH + 1;
constexpr int S2_NSTAGE = S2_ROWS * S2_RS * 8;

// Halo rows iy0 + r (r = 0..8, `need` bit r), input columns ix0 + c (c = 0..64) of channels [ch0, ch0 + 64): slot c/2 of the even
// plane for odd c (= even input column 2 x0 + ...: ix0 = 2 x0 - 1 is odd), slot 32 + c/2 of the odd plane for even c.  Thread t
// owns 16-byte chunk t & 7 of plane slot t >> 3; as in stage_tile64 the rows go global -> LDS directly and the XOR swizzle is
// applied on the source side.  Slot 64 (c = 64) keeps the register path.
template <int CSTRIDE>
__device__ __forceinline__ void stage_tile64_s2(uint4* __restrict__ s_in, const uint16_t* __restrict__ x, int b, int H, int W, int ch0, int iy0,
                                                int ix0, uint32_t need) {
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque: keeps the per-thread staging addresses out of the tile loop's live ranges
  const int slot = tid & 7, col = tid >> 3, wbase = (tid >> 6) * 8;
  const uint16_t* xb = x + (int64_t)b * H * W * CSTRIDE + ch0;
#pragma unroll
  for (int pl = 0; pl < 2; pl++) {        // pl 0: even plane (c = 2 col + 1), pl 1: odd plane (c = 2 col)
    const int ls = pl * 32 + col;         // LDS slot of this thread's column
    const int ix = ix0 + 2 * col + (1 - pl);
    const bool col_ok = (unsigned)ix < (unsigned)W;
    const int chunk = slot ^ lds_swz(ls);
#pragma unroll
    for (int r = 0; r < S2_ROWS; r++) {
      if (!((need >> r) & 1u)) continue;  // wave-uniform
      const int iy = iy0 + r;
      if ((unsigned)iy < (unsigned)H && col_ok) {
        __builtin_amdgcn_global_load_lds((gptr_t)(xb + ((int64_t)iy * W + ix) * CSTRIDE + chunk * 8),
                                         (lptr_t)(s_in + (r * S2_RS + pl * 32 + wbase) * 8), 16, 0, 0);
      } else {
        s_in[(r * S2_RS + ls) * 8 + slot] = make_uint4(0, 0, 0, 0);
      }
    }
  }
  if (tid < S2_ROWS * 8) {  // slot 64: input column ix0 + 64
    const int re = tid >> 3, ce = tid & 7;
    if ((need >> re) & 1u) {
      const int iy = iy0 + re, ix = ix0 + 64;
      uint4 qe = make_uint4(0, 0, 0, 0);
      if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) qe = *reinterpret_cast<const uint4*>(xb + ((int64_t)iy * W + ix) * CSTRIDE + ce * 8);
      s_in[(re * S2_RS + 64) * 8 + (ce ^ lds_swz(64))] = qe;
    }
  }
}

// NP = bf16 pieces per operand, as in conv_pc.h::pc_rows: x / x2 / x3 and wfrag / wfrag2 / wfrag3 = hi / lo (NP 2) or hi / mid / lo (NP 3).
template <int NR, int CIN, int COUT, int MB, int NP = 1>
__device__ __forceinline__ void conv_rows_s2(uint4* __restrict__ s_in, const uint16_t* __restrict__ x, const uint16_t* __restrict__ x2,
                                             const uint16_t* __restrict__ x3, const uint4* __restrict__ wfrag, const uint4* __restrict__ wfrag2,
                                             const uint4* __restrict__ wfrag3, const float* __restrict__ bias, const int (&rbase)[4], const uint32_t (&rmask)[4],
                                             uint16_t* const (&yrow)[4], int b, int H, int W, int iy0, int ix0, int n_valid, uint32_t need, int mg,
                                             int relu, int px, int kb, int lane) {
  constexpr int NS = CIN / 64, NRA = NR > 0 ? NR : 1;
  constexpr bool X3 = NP == 2, F32 = NP > 1;
  v16f acc[NRA][MB];
  if (NR > 0) {
#pragma unroll
    for (int m = 0; m < MB; m++) {
      v16f bq;
      if (F32 && bias == nullptr) {
#pragma unroll
        for (int i = 0; i < 16; i++) bq[i] = 0.f;
      } else {
        bq = bias_tile(bias, (mg + m) * 32, kb);
      }
#pragma unroll
      for (int j = 0; j < NR; j++) acc[j][m] = bq;
    }
  }
  // X3 (fp32 product of bf16 pairs, see conv_pc.h): the NS slabs of the high halves (taps with W_hi and with W_lo), then those of the low halves (W_hi).
  // NP 3: the NS slabs of x_lo (W_hi), of x_mid (W_mid, W_hi), of x_hi (W_lo, W_mid, W_hi) -- the caller staged slab 0 of x_lo.
#pragma unroll 1
  for (int sq = 0; sq < NS * NP; sq++) {
    const int sl = F32 ? sq % NS : sq;
    if (sq) {
      __syncthreads();  // previous slab consumed
      const uint16_t* xs = X3 && sq >= NS ? x2 : x;
      if constexpr (NP == 3) xs = sq < NS ? x3 : sq < 2 * NS ? x2 : x;
      stage_tile64_s2<CIN>(s_in, xs, b, H, W, 64 * sl, iy0, ix0, need);
      __syncthreads();
    }
    if (NR > 0) {
      if constexpr (NP == 3) {
        const int q = sq / NS;  // piece 2 - q of x: W pieces q .. 0
#pragma unroll 1
        for (int k = q; k >= 0; k--)
          conv_taps<NRA, COUT / 32, CIN / 16, 2, MB>(acc, s_in, k == 0 ? wfrag : k == 1 ? wfrag2 : wfrag3, rbase, mg, px, kb, lane, 4 * sl);
      } else {
        conv_taps<NRA, COUT / 32, CIN / 16, 2, MB>(acc, s_in, wfrag, rbase, mg, px, kb, lane, 4 * sl);
        if constexpr (X3) {
          if (sq < NS) conv_taps<NRA, COUT / 32, CIN / 16, 2, MB>(acc, s_in, wfrag2, rbase, mg, px, kb, lane, 4 * sl);
        }
      }
    }
  }
  if (NR > 0) {
#pragma unroll
    for (int j = 0; j < NR; j++) {
      const bool act = (rmask[j] >> px) & 1u;
      if constexpr (F32) {
#pragma unroll
        for (int m = 0; m < MB; m++) store_tile_f32<COUT>(acc[j][m], act, reinterpret_cast<float*>(yrow[j]) + (mg + m) * 32, n_valid, px, kb);
      } else if constexpr (MB == 2) {
        uint4 D[4];
#pragma unroll
        for (int m = 0; m < 2; m++) {
          uint4 pk[2];
          pack_tile(acc[j][m], act, relu, pk);
          D[2 * m] = pk[0], D[2 * m + 1] = pk[1];
        }
        transpose_row64(D, lane);
        store_row64<COUT>(D, yrow[j] + mg * 32, n_valid, lane);
      } else {  // one 32-channel tile per wave: complete 64-byte half lines
        uint4 pk[2];
        pack_tile(acc[j][0], act, relu, pk);
        transpose_row32(pk, lane);
        store_row32<COUT>(pk, yrow[j] + mg * 32, n_valid, lane);
      }
    }
  }
}

// H, W: input; Ho, Wo: output.  The 4 waves are COUT/64 groups of 64 output channels x 4/(COUT/64) row groups.
template <int CIN, int COUT, int NP = 1>
__global__ __launch_bounds__(256, 2) void k_conv3x3_s2(const uint16_t* __restrict__ x, const uint16_t* __restrict__ x2, const uint4* __restrict__ wfrag,
                                                    const uint4* __restrict__ wfrag2, const float* __restrict__ bias,
                                                    const uint8_t* __restrict__ mask, uint16_t* __restrict__ y, int B, int H, int W, int Ho, int Wo,
                                                    int relu, RowDirty row_dirty, int slot, const uint16_t* __restrict__ x3 = nullptr,
                                                    const uint4* __restrict__ wfrag3 = nullptr) {
  static_assert(CIN % 64 == 0 && (COUT == 128 || COUT == 256), "64-channel input slabs; 4 groups of 32 or of 64 output channels");
  // Round 6: with 128 output channels the waves were 2 row groups x 2 groups of 64 channels, i.e. at most TWO rows per wave -- one 1 KiB weight fragment from
  // L1 per two MFMAs, which is all of the L1's bandwidth at full MFMA rate (the 759 us outlier of profiles/r06_bench_steady_trace.md).  Now every shape has one
  // row group: four rows per wave, four channel groups of COUT / 4.
  constexpr int TH = S2_TH, MB = COUT / 128, NCG = 4, NRG = 1, NRMAX = TH / NRG;
  constexpr int YS = NP > 1 ? 2 : 1;  // output element in units of uint16_t (NP > 1: fp32)
  extern __shared__ uint4 s_in[];  // S2_NSTAGE
  __shared__ uint32_t s_rowmask2[2 * TH];
  __shared__ unsigned int s_next[2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int px = lane & 31, kb = lane >> 5;
  const int rg = wv % NRG, mg = MB * (wv / NRG);
  static_assert(NCG * NRG == 4, "four waves");
  const int tiles_x = (Wo + 31) >> 5, tiles_y = (Ho + TH - 1) / TH;
  const int64_t n_tiles = (int64_t)B * tiles_y * tiles_x;
  int64_t next = 0;
  int it = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile = next, it++) {
    sched_draw(s_next, it, slot);
    uint32_t* const s_rowmask = s_rowmask2 + (it & 1) * TH;
    const int tx = (int)(tile % tiles_x);
    const int ty = (int)((tile / tiles_x) % tiles_y);
    const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
    const int x0 = tx * 32, y0 = ty * TH;
    const int ox = x0 + px;
    uint32_t was = 0xffffffffu, bal;  // written mask of this wave's row segment before the launch (pnx.h: row_dirty), its active pixels now
    {  // active sites: wave wv looks at output row wv of the tile
      const int oy = y0 + wv;
      const bool a = ox < Wo && oy < Ho && (mask == nullptr || mask[((int64_t)b * Ho + oy) * Wo + ox] != 0);
      if (oy < Ho) was = (uint32_t)__builtin_amdgcn_readfirstlane((int)rd_load(row_dirty, ((int64_t)b * Ho + oy) * tiles_x + tx));
      bal = (uint32_t)__ballot(a);
      if (lane == 0) s_rowmask[wv] = bal;
    }
    __syncthreads();  // row masks visible; everybody is done reading the previous tile's s_in
    next = sched_next(s_next, it, slot, tile);
    const uint32_t my_rm = s_rowmask[lane & 3];
    const uint32_t am = (uint32_t)__ballot(my_rm != 0) & 0xfu;
    {  // a row without any active site: zero-fill the pixels that may hold data; an active row is stored whole, so its written mask is its row mask
      const int oy = y0 + wv;
      const bool active = (am >> wv) & 1u;
      if (!active && ((rd_held(row_dirty, was) >> px) & 1u) && oy < Ho && ox < Wo) {
        uint4* dst = reinterpret_cast<uint4*>(y + (((int64_t)b * Ho + oy) * Wo + ox) * COUT * YS);
#pragma unroll 1
        for (int ch = kb; ch < COUT * YS / 8; ch += 2) dst[ch] = make_uint4(0, 0, 0, 0);
      }
      if (oy < Ho && lane == 0) rd_store(row_dirty, ((int64_t)b * Ho + oy) * tiles_x + tx, was, bal);
    }
    if (am == 0) continue;  // uniform over the workgroup
    int nr = 0;
    int rbase[4], rrow[4];
    {  // the active rows, dealt round-robin to the row groups
      uint32_t rest = am;
      for (int k = 0; k < rg && rest; k++) rest &= rest - 1;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool has = j < NRMAX && rest != 0;
        rrow[j] = has ? __builtin_ctz(rest) : 0;  // dummy rows point at row 0
        nr += has ? 1 : 0;
        for (int k = 0; k < NRG && rest; k++) rest &= rest - 1;
      }
    }
    nr = __builtin_amdgcn_readfirstlane(nr);
    uint32_t rmask[4];
    uint16_t* yrow[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      rrow[j] = __builtin_amdgcn_readfirstlane(rrow[j]);
      rbase[j] = 2 * rrow[j] * S2_RS * 8;
      rmask[j] = j < nr ? __builtin_amdgcn_readfirstlane(s_rowmask[rrow[j]]) : 0u;
      yrow[j] = y + (((int64_t)b * Ho + (y0 + rrow[j])) * Wo + x0) * COUT * YS;
    }
    uint32_t need = 0;  // halo rows some active output row reads: rows 2r, 2r+1, 2r+2
#pragma unroll
    for (int r = 0; r < TH; r++)
      if ((am >> r) & 1u) need |= 7u << (2 * r);
    const int iy0 = 2 * y0 - 1, ix0 = 2 * x0 - 1;
    stage_tile64_s2<CIN>(s_in, NP == 3 ? x3 : x, b, H, W, 0, iy0, ix0, need);  // NP 3: the low pieces come first
    __syncthreads();
#define PNX_ROWS_S2(N_) conv_rows_s2<(N_ <= NRMAX ? N_ : NRMAX), CIN, COUT, MB, NP>(s_in, x, x2, x3, wfrag, wfrag2, wfrag3, bias, rbase, rmask, yrow, b, H, W, iy0, ix0, Wo - x0, need, mg, relu, px, kb, lane)
    switch (nr) {  // wave-uniform; every case runs the same barriers
      case 0: PNX_ROWS_S2(0); break;
      case 1: PNX_ROWS_S2(1); break;
      case 2: PNX_ROWS_S2(2); break;
      case 3: PNX_ROWS_S2(3); break;
      default: PNX_ROWS_S2(4); break;
    }
#undef PNX_ROWS_S2
  }
  sched_done(slot);
}

template <int CIN, int COUT, int NP>
int launch_s2(PnxPieces<NP> x, PnxPieces<NP> wfrag, const float* bias, const uint8_t* mask, void* y, int B, int H, int W, int Ho, int Wo, int relu,
              RowDirty row_dirty, hipStream_t st) {
  const int slot = mask != nullptr ? next_sched_slot() : -1;
  int64_t nb = (int64_t)B * ((Ho + S2_TH - 1) / S2_TH) * ((Wo + 31) / 32);
  if (nb > 512) nb = 512;  // resident workgroups: 2 per CU (LDS and registers)
  constexpr auto kern = k_conv3x3_s2<CIN, COUT, NP>;
  constexpr int lds = S2_NSTAGE * 16;
  if (const int rc = pnx_lds_optin<kern>(lds); rc != PNX_OK) return rc;
  kern<<<(unsigned)nb, 256, lds, st>>>((const uint16_t*)x.hi, (const uint16_t*)x.slot2(), (const uint4*)wfrag.hi, (const uint4*)wfrag.slot2(), bias, mask,
                                       (uint16_t*)y, B, H, W, Ho, Wo, relu, row_dirty, slot, (const uint16_t*)x.slot3(), (const uint4*)wfrag.slot3());
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}
