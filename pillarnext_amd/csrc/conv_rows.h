// conv_rows.h -- the row-split stride-1 kernels (included by conv3x3.hip after conv_taps.h): k_conv3x3_lds (64 input channels: conv_rows) and
// k_conv3x3_ldsx (128 -> 128, 256 -> 256, 256 -> 64: conv_rows_x, and its packed-pixel form conv_pix_x) with launch_ldsx.  launch_lds stands in
// conv3x3.hip.  Since round 6 these are the cross-checks of k_conv3x3_pc at 64 -> 64 and the default everywhere else.
#pragma once

// k_conv3x3_lds: stride 1, 64 input channels, with the INPUT tile staged in LDS: a workgroup owns 16 x 32 output pixels; the 18 x 34 halo tile of 64
// input channels (128 B per pixel) is loaded once with coalesced 16-byte loads (all loads of a batch in flight before the first
// ds_write), XOR-swizzled so that each 16-lane service group of a ds_read_b128 B-fragment read covers all 64 banks, and then
// serves all 9 taps of all 4 waves -- the direct kernel (k_conv3x3, conv3x3.hip) re-reads every pixel line 9 times through L1/L2 (measured:
// 4.8 GB of L2->L1 traffic per 1440x1440 frame).  Sparsity: the 16 row segments of a tile that hold at least one active site
// are dealt round-robin to the 4 waves (row indices live in SGPRs), each wave runs a branch-free tap loop specialised on its
// row count NR = 1..4 (LDS reads pipeline ahead of the MFMAs), halo rows no active row needs are not staged, and rows without
// an active site are zero-filled without touching the MFMA pipe.  Weights (fragment order, 1 KiB per wave-load, shared by every
// wave on the chip) come straight from L1/L2, one tap ahead of their use.  CIN > 64 is processed as successive 64-channel
// slabs; COUT > 64 as successive 64-channel passes over the same staged tile (the merged SepHead convolution 64 -> 384 stages
// its input once and reuses it six times).

// Everything a wave does for its NR active rows once the tile is staged: per 64-channel pass, accumulators = bias (+ residual),
// the taps, and the epilogue.  No barrier inside.
template <int NR, int COUT, bool HAS_RES>
__device__ __forceinline__ void conv_rows(const uint4* __restrict__ s_in, const uint4* __restrict__ wfrag, const float* __restrict__ bias,
                                          const uint16_t* const (&rrow_res)[4], uint32_t res_off, const int (&rbase)[4], const uint32_t (&rmask)[4],
                                          uint16_t* const (&yrow)[4], int n_valid, int relu, int px, int kb, int lane) {
  constexpr int MTALL = COUT / 32;
#pragma unroll 1
  for (int mg = 0; mg < MTALL; mg += 2) {  // 64 output channels per pass over the staged tile
    v16f acc[NR][2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const v16f bq = bias_tile(bias, (mg + m) * 32, kb);
#pragma unroll
      for (int j = 0; j < NR; j++) acc[j][m] = bq;
    }
    // The residual (HAS_RES: one 64-channel pass by construction) joins in the epilogue: the lines of row 0 are requested here and arrive under the
    // tap loop (16 registers), the lines of row j + 1 are requested before row j is packed and stored -- a load is never issued BEHIND a store it
    // then has to wait for (gfx9 vmcnt is in-order), and nothing is held across the staging of the tile.  (The round 2-4 form, the residual starting
    // the accumulators, held 64 registers across the staging: 212 B/lane of scratch; profiles/r05_conv_ab.txt.  Removed, see git history.)
    uint4 rq[2][2];
    if (HAS_RES) load_residual_u(rq, rrow_res[0], res_off, rmask[0] >> px & 1u);
    conv_taps<NR, MTALL, 4, 1, 2, COUT == 64 ? 2 : TAPS_WD>(acc, s_in, wfrag, rbase, mg, px, kb, lane);  // 64 -> 64 (the cross-check of k_conv3x3_pc): a two-deep weight ring keeps it at 0 scratch
#pragma unroll
    for (int j = 0; j < NR; j++) {
      const bool act = (rmask[j] >> px) & 1u;
      uint4 rc[2][2];
      if (HAS_RES) {
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
          for (int t = 0; t < 2; t++) rc[m][t] = rq[m][t];
        if (j + 1 < NR) load_residual_u(rq, rrow_res[j + 1], res_off, rmask[j + 1] >> px & 1u);
      }
      uint4 D[4];
#pragma unroll
      for (int m = 0; m < 2; m++) {
        uint4 pk[2];
        pack_tile(acc[j][m], act, relu, pk, HAS_RES ? rc[m] : nullptr);
        D[2 * m] = pk[0], D[2 * m + 1] = pk[1];
      }
      transpose_row64(D, lane);
      store_row64<COUT>(D, yrow[j] + mg * 32, n_valid, lane);
    }
  }
}

template <int COUT, bool HAS_RES>
__global__ __launch_bounds__(256, 2) void k_conv3x3_lds(const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag,
                                                     const float* __restrict__ bias, const uint16_t* __restrict__ res,
                                                     const uint8_t* __restrict__ mask, uint16_t* __restrict__ y, int B, int H, int W,
                                                     int relu, RowDirty row_dirty, int slot, const int32_t* __restrict__ tlist,
                                                      const int32_t* __restrict__ tcount) {
  constexpr int CIN = 64;
  constexpr int TH = LDS_TH, HW_ = LDS_HW;
  static_assert(!HAS_RES || COUT == 64, "the residual is folded into the accumulators of a single 64-channel pass");
  __shared__ uint4 s_in[LDS_NSTAGE];
  __shared__ uint32_t s_rowmask2[2 * TH];  // double-buffered by iteration parity: an empty tile has a single barrier (see s_next)
  __shared__ unsigned int s_next[2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int px = lane & 31, kb = lane >> 5;
  const int tiles_x = (W + 31) >> 5, tiles_y = (H + TH - 1) / TH;
  const int64_t n_tiles = tlist != nullptr ? (int64_t)__builtin_amdgcn_readfirstlane(*tcount) : (int64_t)B * tiles_y * tiles_x;
  // requests the mask bytes / written masks (pnx.h: row_dirty) of the rows this wave looks at in tile t (t < 0: none)
  auto load_mask = [&](int64_t t, bool (&a)[4], int (&wz)[4]) {
#pragma unroll
    for (int j = 0; j < 4; j++) a[j] = false, wz[j] = -1;
    if (t < 0) return;
    const int tx = (int)(t % tiles_x);
    const int ty = (int)((t / tiles_x) % tiles_y);
    const int b = (int)(t / ((int64_t)tiles_x * tiles_y));
    const int ox = tx * 32 + px;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int oy = ty * TH + wv * 4 + j;
      a[j] = ox < W && oy < H && (mask == nullptr || mask[((int64_t)b * H + oy) * W + ox] != 0);
      if (oy < H) wz[j] = (int)rd_load(row_dirty, ((int64_t)b * H + oy) * tiles_x + tx);
    }
  };
  int64_t idxB = (int64_t)blockIdx.x + gridDim.x, idxC = 0;
  int64_t tileA = tile_at(tlist, blockIdx.x, n_tiles), tileB = tile_at(tlist, idxB, n_tiles), tileC = -1;
  bool aP[4], aN[4];
  int wasP[4], wasN[4];
  load_mask(tileA, aP, wasP);
#pragma unroll
  for (int j = 0; j < 4; j++) aN[j] = false, wasN[j] = -1;
  CT_DECL
  int it = 0;
  for (; tileA >= 0; tileA = tileB, tileB = tileC, idxB = idxC, it++) {
    const int64_t tile = (int64_t)__builtin_amdgcn_readfirstlane((int)tileA);  // uniform by construction: everything derived from it (origins, row pointers) lives in scalar registers
    sched_draw(s_next, it, slot);
    uint32_t* const s_rowmask = s_rowmask2 + (it & 1) * TH;
    const int tx = (int)(tile % tiles_x);
    const int ty = (int)((tile / tiles_x) % tiles_y);
    const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
    const int x0 = tx * 32, y0 = ty * TH;
    const int ox = x0 + px;
    CT_TOCK(7)
    uint32_t was[4], bal[4];  // written mask of the row segment before this launch, its active pixels now
#pragma unroll
    for (int j = 0; j < 4; j++) {  // active sites: one 32-bit column mask per row of the tile, from the bytes requested one tile ago
      was[j] = (uint32_t)__builtin_amdgcn_readfirstlane(wasP[j]);
      bal[j] = (uint32_t)__ballot(aP[j]);
      if (lane == 0) s_rowmask[wv * 4 + j] = bal[j];
    }
    __syncthreads();  // row masks visible; everybody is done reading the previous tile's s_in
    idxC = sched_next2(s_next, it, slot, idxB);
    tileC = tile_at(tlist, idxC, n_tiles);
    load_mask(tileB, aN, wasN);  // consumed at the top of the next iteration
#pragma unroll
    for (int j = 0; j < 4; j++) aP[j] = aN[j], wasP[j] = wasN[j];
    CT_TOCK(0)
    const uint32_t my_rm = s_rowmask[lane & 15];
    const uint32_t am = (uint32_t)__ballot(my_rm != 0) & 0xffffu;  // rows with an active site (wave-uniform, same in all waves)
    // ---- rows without any active site: zero-fill the pixels that may hold data (natural rows of this wave); active rows are stored whole
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int rr = wv * 4 + j, oy = y0 + rr;
      const bool active = (am >> rr) & 1u;
      if (!active && ((rd_held(row_dirty, was[j]) >> px) & 1u) && oy < H && ox < W) {
        uint4* dst = reinterpret_cast<uint4*>(y + (((int64_t)b * H + oy) * W + ox) * COUT);
#pragma unroll 1
        for (int ch = kb; ch < COUT / 8; ch += 2) dst[ch] = make_uint4(0, 0, 0, 0);
      }
      if (oy < H && lane == 0) rd_store(row_dirty, ((int64_t)b * H + oy) * tiles_x + tx, was[j], bal[j]);
    }
    if (am == 0) continue;  // uniform over the workgroup
    // ---- the active rows, dealt round-robin to the waves (wave wv takes the active rows number wv, wv+4, ...)
    int nr = 0;
    int rbase[4], rrow[4];
    {
      uint32_t rest = am;
      for (int k = 0; k < wv && rest; k++) rest &= rest - 1;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const bool has = rest != 0;
        rrow[j] = has ? __builtin_ctz(rest) : 0;  // dummy rows point at row 0
        nr += has ? 1 : 0;
        for (int k = 0; k < 4 && rest; k++) rest &= rest - 1;
      }
    }
    nr = __builtin_amdgcn_readfirstlane(nr);
    uint32_t rmask[4];
    uint16_t* yrow[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      rrow[j] = __builtin_amdgcn_readfirstlane(rrow[j]);
      rbase[j] = rrow[j] * HW_ * 8;
      rmask[j] = j < nr ? __builtin_amdgcn_readfirstlane(s_rowmask[rrow[j]]) : 0u;
      yrow[j] = y + (((int64_t)b * H + (y0 + rrow[j])) * W + x0) * COUT;
    }
    const uint32_t need = am | (am << 1) | (am << 2);  // halo rows some active row reads
    CT_TOCK(1)
    // ---- residual lines of this lane's pixel in the wave's rows (requested inside conv_rows)
    const uint16_t* rres[4];  // wave-uniform: pixel 0 of the row segment
#pragma unroll
    for (int j = 0; j < 4; j++) rres[j] = HAS_RES ? res + (((int64_t)b * H + (y0 + rrow[j])) * W + x0) * COUT : nullptr;
    const uint32_t res_off = (uint32_t)(px * COUT + 8 * kb) * 2u;
    stage_tile64<CIN>(s_in, x, b, H, W, 0, y0, x0, need);
    CT_TOCK(2)
    __syncthreads();
    CT_TOCK(3)
    const int n_valid = W - x0;
    switch (nr) {  // wave-uniform
      case 1: conv_rows<1, COUT, HAS_RES>(s_in, wfrag, bias, rres, res_off, rbase, rmask, yrow, n_valid, relu, px, kb, lane); break;
      case 2: conv_rows<2, COUT, HAS_RES>(s_in, wfrag, bias, rres, res_off, rbase, rmask, yrow, n_valid, relu, px, kb, lane); break;
      case 3: conv_rows<3, COUT, HAS_RES>(s_in, wfrag, bias, rres, res_off, rbase, rmask, yrow, n_valid, relu, px, kb, lane); break;
      case 4: conv_rows<4, COUT, HAS_RES>(s_in, wfrag, bias, rres, res_off, rbase, rmask, yrow, n_valid, relu, px, kb, lane); break;
      default: break;
    }
    CT_TOCK(4)
  }
  sched_done(slot);
  CT_FLUSH
}

// ---- CIN -> COUT channels in multiples of 64 / 128, stride 1: 8 x 32 pixel tiles, 64-channel input slabs through one LDS buffer
constexpr int L128_TH = 8;
constexpr int L128_NSTAGE = (L128_TH + 2) * LDS_HW * 8;

int next_sched_slot() {
  static unsigned int n = 0;  // one host thread per process drives the launches (pnx.h: not thread-safe)
  return (int)(n++ & 63u);
}

// 128 -> 128 (stage 1) and 256 -> 256 (stages 2 and 3 of the backbone, sparse_resnet.py:50-68).  Per tile, COUT/128 passes (the 4
// waves = 2 row groups x 2 groups of 64 output channels, 4 rows x 64 channels of accumulators each) over CIN/64 input slabs that
// go through the one 43.5 KiB LDS buffer under live accumulators, so 2 workgroups share a CU.  Every (pass, slab) step is
// bracketed by the same two barriers in every wave, whatever its row count (s_barrier counts arrivals, not program counters).
// The residual of a pass is loaded right before it is added: holding the lines from the top of the tile (as the 64-channel
// kernel does) cost 64-128 VGPRs and ~90 spilled registers here -- measured on the stage-1 LiDAR mask, 128 -> 128 with residual:
// 653 us with early loads, 567 us with late ones.
// Depth of the weight-fragment ring with a residual: the row-0 lines are in flight under the last slab's taps (16 registers), and two pairs fewer in
// the ring than TAPS_WD keep the kernel at 256 registers without spilling the tile loop's state (profiles/r06_conv_pc_ab.txt (12)).
constexpr int LDSX_RES_WD = 2;
template <int NR, int CIN, int COUT, bool HAS_RES>
__device__ __forceinline__ void conv_rows_x(uint4* __restrict__ s_in, const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag,
                                            const float* __restrict__ bias, const uint16_t* __restrict__ res, const int (&rrow)[4],
                                            const int (&rbase)[4], const uint32_t (&rmask)[4], uint16_t* const (&yrow)[4], int b, int H, int W,
                                            int y0, int x0, uint32_t need, int mg0, int relu, int px, int kb, int lane, int hsel) {
  constexpr int NS = CIN / 64, NRA = NR > 0 ? NR : 1;
  const int ox = x0 + px;
  {  // ONE pass of 128 output channels per call (round 6: a work unit is (tile, pass), see k_conv3x3_ldsx); slab 0 of the tile is already staged
    const int h = hsel;
    const int mg = mg0 + 4 * h;
    v16f acc[NRA][2];
    if (NR > 0) {
#pragma unroll
      for (int m = 0; m < 2; m++) {
        const v16f bq = bias_tile(bias, (mg + m) * 32, kb);
#pragma unroll
        for (int j = 0; j < NR; j++) acc[j][m] = bq;
      }
    }
    // residual of this pass: row 0's lines are requested before the LAST input slab's taps and arrive under them, row j + 1's before row j is packed
    // (see conv_rows); nothing is held across a barrier-bracketed slab change
    const uint16_t* rres[NRA];  // wave-uniform: pixel 0 of the row segment, first channel of this wave's 64-channel group
    const uint32_t res_off = (uint32_t)(px * COUT + 8 * kb) * 2u;
    uint4 rq[2][2];
    if (NR > 0 && HAS_RES) {
#pragma unroll
      for (int j = 0; j < NR; j++) rres[j] = res + (((int64_t)b * H + (y0 + rrow[j])) * W + x0) * COUT + mg * 32;
    }
#pragma unroll 1
    for (int sl = 0; sl < NS; sl++) {
      if (sl) {
        __syncthreads();  // previous slab consumed
        stage_tile64<CIN, L128_TH>(s_in, x, b, H, W, 64 * sl, y0, x0, need);
        __syncthreads();
      }
      if (NR > 0 && HAS_RES && sl == NS - 1) load_residual_u(rq, rres[0], res_off, rmask[0] >> px & 1u);
      if (NR > 0) conv_taps<NRA, COUT / 32, CIN / 16, 1, 2, HAS_RES ? LDSX_RES_WD : TAPS_WD>(acc, s_in, wfrag, rbase, mg, px, kb, lane, 4 * sl);
    }
    if (NR > 0) {
      const int n_valid = W - x0;
#pragma unroll
      for (int j = 0; j < NR; j++) {
        const bool act = (rmask[j] >> px) & 1u;
        uint4 rc[2][2];
        if (HAS_RES) {
#pragma unroll
          for (int m = 0; m < 2; m++)
#pragma unroll
            for (int t = 0; t < 2; t++) rc[m][t] = rq[m][t];
          if (j + 1 < NR) load_residual_u(rq, rres[j + 1], res_off, rmask[j + 1] >> px & 1u);
        }
        uint4 D[4];
#pragma unroll
        for (int m = 0; m < 2; m++) {
          uint4 pk[2];
          pack_tile(acc[j][m], act, relu, pk, HAS_RES ? rc[m] : nullptr);
          D[2 * m] = pk[0], D[2 * m + 1] = pk[1];
        }
        transpose_row64(D, lane);
        store_row64<COUT>(D, yrow[j] + mg * 32, n_valid, lane);
      }
    }
  }
}

// ---- packed-pixel form (PNX_CONV_PACK, default on with a mask): the active pixels of a tile, listed in row-major order (s_list: pix_code per
// entry), are cut into groups of 32 and the groups -- not the row segments -- are dealt round-robin to the 2 row groups.  On the LiDAR masks about
// half the pixels of an active row segment are inactive; packing never makes more groups than there are active rows (ceil(P / 32) <= rows), and
// on a tile whose rows are all half-empty it halves the MFMA work.  Per output element the k-steps and MFMAs are those of the row form (same
// accumulator start, same (dx, chunk, dy) order, same epilogue arithmetic): the output is bit-identical.  Only the addressing changes: a lane's B
// fragments come from its own listed pixel (conv_taps<PIX>), and stores / residual loads are a uniform tile-origin pointer + a 32-bit per-lane
// pixel offset.  Inactive pixels of active rows are zeroed separately (zero_inactive_pixels), so nothing else of the output contract changes.
__device__ __forceinline__ int pix_code(int row, int col) { return (row << 5) | col; }
// byte offset of pixel `code` from the tile origin, channel 0, in an NHWC tensor of CSTRIDE channels and row pitch W pixels
template <int CSTRIDE>
__device__ __forceinline__ uint32_t pix_off(int code, int W) { return (uint32_t)(((code >> 5) * W + (code & 31)) * CSTRIDE) * 2u; }

// store_row64 for a pixel group: store d of lane L is chunk L & 7 of listed pixel 8 d + (L >> 3), whose code lanes 0..31 hold (code of lane px = its
// pixel px of the group); pixels >= n_valid are not stored.  Every store instruction still writes 8 complete 128-byte lines.  Called by all 64 lanes.
template <int CSTRIDE>
__device__ __forceinline__ void store_pix64(const uint4 (&D)[4], uint16_t* __restrict__ tile, int code, int n_valid, int W, int lane) {
  int l = lane;
  asm volatile("" : "+v"(l));  // opaque: keeps the per-lane permute addresses from being hoisted out of the tile loop (and spilled)
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const int P = 8 * d + (l >> 3);
    const int pc = __builtin_amdgcn_ds_bpermute(P << 2, code);
    if (P < n_valid) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(tile) + pix_off<CSTRIDE>(pc, W) + (uint32_t)((l & 7) * 16)) = D[d];
  }
}

// conv_rows_x on NR pixel groups: byte j of `codes` = pix_code of this lane's pixel in group j (lanes px >= n_g[j] carry code 0 and are neither loaded
// nor stored: one register for all groups keeps the kernel at 256 VGPRs without scratch), ytile / rtile = output / residual at the tile origin
// (wave-uniform).  One pass of 128 output channels, the same barriers as conv_rows_x.
template <int NR, int CIN, int COUT, bool HAS_RES>
__device__ __forceinline__ void conv_pix_x(uint4* __restrict__ s_in, const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag,
                                           const float* __restrict__ bias, const uint16_t* __restrict__ rtile, int codes, const int (&n_g)[4],
                                           uint16_t* __restrict__ ytile, int b, int H, int W, int y0, int x0, uint32_t need, int mg0, int relu, int px,
                                           int kb, int lane, int hsel) {
  constexpr int NS = CIN / 64, NRA = NR > 0 ? NR : 1;
  const int mg = mg0 + 4 * hsel;
  v16f acc[NRA][2];
  if (NR > 0) {
#pragma unroll
    for (int m = 0; m < 2; m++) {
      const v16f bq = bias_tile(bias, (mg + m) * 32, kb);
#pragma unroll
      for (int j = 0; j < NR; j++) acc[j][m] = bq;
    }
  }
  // residual: group 0's lines are requested before the last slab's taps, group j + 1's before group j is packed (as in conv_rows_x)
  const uint16_t* const rres = HAS_RES ? rtile + mg * 32 : nullptr;
  auto code = [&](int j) { return (codes >> (8 * j)) & 255; };
  auto res_off = [&](int j) { return pix_off<COUT>(code(j), W) + (uint32_t)(16 * kb); };
  const int cw[4] = {codes, 0, 0, 0};
  uint4 rq[2][2];
#pragma unroll 1
  for (int sl = 0; sl < NS; sl++) {
    if (sl) {
      __syncthreads();  // previous slab consumed
      stage_tile64<CIN, L128_TH>(s_in, x, b, H, W, 64 * sl, y0, x0, need);
      __syncthreads();
    }
    if (NR > 0 && HAS_RES && sl == NS - 1) load_residual_u(rq, rres, res_off(0), px < n_g[0]);
    if (NR > 0) conv_taps<NRA, COUT / 32, CIN / 16, 1, 2, HAS_RES ? LDSX_RES_WD : TAPS_WD, true>(acc, s_in, wfrag, cw, mg, px, kb, lane, 4 * sl);
  }
  if (NR > 0) {
#pragma unroll
    for (int j = 0; j < NR; j++) {
      const bool act = px < n_g[j];
      uint4 rc[2][2];
      if (HAS_RES) {
#pragma unroll
        for (int m = 0; m < 2; m++)
#pragma unroll
          for (int t = 0; t < 2; t++) rc[m][t] = rq[m][t];
        if (j + 1 < NR) load_residual_u(rq, rres, res_off(j + 1), px < n_g[j + 1]);
      }
      uint4 D[4];
#pragma unroll
      for (int m = 0; m < 2; m++) {
        uint4 pk[2];
        pack_tile(acc[j][m], act, relu, pk, HAS_RES ? rc[m] : nullptr);
        D[2 * m] = pk[0], D[2 * m + 1] = pk[1];
      }
      transpose_row64(D, lane);
      store_pix64<COUT>(D, ytile + mg * 32, code(j), n_g[j], W, lane);
    }
  }
}

template <int CIN, int COUT, bool HAS_RES, bool PACK = false>
__global__ __launch_bounds__(256, 2) void k_conv3x3_ldsx(const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag,
                                                      const float* __restrict__ bias, const uint16_t* __restrict__ res,
                                                      const uint8_t* __restrict__ mask, uint16_t* __restrict__ y, int B, int H, int W,
                                                      int relu, RowDirty row_dirty, int slot, const int32_t* __restrict__ tlist,
                                                      const int32_t* __restrict__ tcount) {
  static_assert(CIN % 64 == 0 && (COUT % 128 == 0 || COUT == 64), "64-channel input slabs, 128-channel output passes (or one of 64)");
  constexpr int TH = L128_TH, HW_ = LDS_HW;
  constexpr int NRG = COUT == 64 ? 4 : 2, NRMAX = TH / NRG;  // row groups (the other waves split the 128 output channels of a pass)
  static_assert(!PACK || (CIN == COUT && NRG == 2), "the packed-pixel form serves 128 -> 128 and 256 -> 256");
  __shared__ uint4 s_in[L128_NSTAGE];
  __shared__ uint16_t s_list[PACK ? TH * 32 : 1];  // PACK: pix_code of the tile's active pixels, row-major
  __shared__ uint32_t s_rowmask2[2 * TH];  // double-buffered by iteration parity (an empty tile has a single barrier)
  __shared__ unsigned int s_next[2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int px = lane & 31, kb = lane >> 5;
  const int rg = wv % NRG, mg0 = 2 * (wv / NRG);  // row group, first 32-channel output tile of this wave within a pass
  const int tiles_x = (W + 31) >> 5, tiles_y = (H + TH - 1) / TH;
  const int n_tiles = tlist != nullptr ? __builtin_amdgcn_readfirstlane(*tcount) : B * tiles_y * tiles_x;  // < 2^31 / NH: 32-bit unit indices keep the tile loop's state in fewer registers
  // Work unit = (tile, pass of 128 output channels) (round 6): every pass re-stages the tile's input slabs anyway, so handing the COUT / 128 passes of a tile to
  // different workgroups costs nothing and doubles the number of units -- at 180 x 180 a 256 -> 256 layer has ~830 active 8 x 32 tiles for 512 workgroups.
  // A unit is coded tile * NH + pass; pass 0 also does the tile's zero-fill / row_dirty bookkeeping.
  constexpr int NH = (COUT + 127) / 128;
  const int n_units = n_tiles * NH;
  auto unit_at = [&](int64_t idx) -> int {
    if (idx >= n_units) return -1;
    const int i = (int)idx;
    const int t = tlist != nullptr ? tlist[i / NH] : i / NH;
    return t * NH + i % NH;
  };
  // requests the mask bytes / written masks (pnx.h: row_dirty) of the rows this wave looks at in tile t (t < 0: none)
  auto load_mask = [&](int t, bool (&a)[2], int (&wz)[2]) {
#pragma unroll
    for (int j = 0; j < 2; j++) a[j] = false, wz[j] = -1;
    if (t < 0) return;
    const int tx = (int)(t % tiles_x);
    const int ty = (int)((t / tiles_x) % tiles_y);
    const int b = (int)(t / ((int64_t)tiles_x * tiles_y));
    const int ox = tx * 32 + px;
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int oy = ty * TH + wv * 2 + j;
      a[j] = ox < W && oy < H && (mask == nullptr || mask[((int64_t)b * H + oy) * W + ox] != 0);
      if (oy < H) wz[j] = (int)rd_load(row_dirty, ((int64_t)b * H + oy) * tiles_x + tx);
    }
  };
  int64_t idxB = (int64_t)blockIdx.x + gridDim.x, idxC = 0;
  int tileA = unit_at(blockIdx.x), tileB = unit_at(idxB), tileC = -1;
  bool aP[2], aN[2];
  int wasP[2], wasN[2];
  load_mask(tileA >= 0 ? tileA / NH : -1, aP, wasP);
#pragma unroll
  for (int j = 0; j < 2; j++) aN[j] = false, wasN[j] = -1;
  int it = 0;
  for (; tileA >= 0; tileA = tileB, tileB = tileC, idxB = idxC, it++) {
    const int unit = __builtin_amdgcn_readfirstlane(tileA);  // uniform by construction: everything derived from it (origins, row pointers) lives in scalar registers
    const int tile = unit / NH;
    const int hsel = unit - tile * NH;
    sched_draw(s_next, it, slot);
    uint32_t* const s_rowmask = s_rowmask2 + (it & 1) * TH;
    const int tx = (int)(tile % tiles_x);
    const int ty = (int)((tile / tiles_x) % tiles_y);
    const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
    const int x0 = tx * 32, y0 = ty * TH;
    const int ox = x0 + px;
    uint32_t was[2], bal[2];  // written mask of the row segment before this launch, its active pixels now
#pragma unroll
    for (int j = 0; j < 2; j++) {  // active sites: one 32-bit column mask per row of the tile, from the bytes requested one tile ago
      was[j] = (uint32_t)__builtin_amdgcn_readfirstlane(wasP[j]);
      bal[j] = (uint32_t)__ballot(aP[j]);
      if (lane == 0) s_rowmask[wv * 2 + j] = bal[j];
    }
    __syncthreads();  // row masks visible; everybody is done reading the previous tile's s_in
    idxC = sched_next2(s_next, it, slot, idxB);
    tileC = unit_at(idxC);
    load_mask(tileB >= 0 ? tileB / NH : -1, aN, wasN);  // consumed at the top of the next iteration
#pragma unroll
    for (int j = 0; j < 2; j++) aP[j] = aN[j], wasP[j] = wasN[j];
    const uint32_t my_rm = s_rowmask[lane & 7];
    const uint32_t am = (uint32_t)__ballot(my_rm != 0) & 0xffu;
#pragma unroll
    for (int j = 0; j < 2; j++) {  // rows without any active site: zero-fill the pixels that may hold data
      const int rr = wv * 2 + j, oy = y0 + rr;
      const bool active = (am >> rr) & 1u;
      // The tile's zero-fill and bookkeeping belong to its pass-0 unit, for ALL the output channels: the units of a tile run on different workgroups in
      // either order, and a pass that read the written masks after pass 0 had updated them would find nothing stale.
      if (hsel != 0) continue;
      if (!active && ((rd_held(row_dirty, was[j]) >> px) & 1u) && oy < H && ox < W) {
        uint4* dst = reinterpret_cast<uint4*>(y + (((int64_t)b * H + oy) * W + ox) * COUT);
#pragma unroll 1
        for (int ch = kb; ch < COUT / 8; ch += 2) dst[ch] = make_uint4(0, 0, 0, 0);
      }
      if (oy < H && lane == 0) rd_store(row_dirty, ((int64_t)b * H + oy) * tiles_x + tx, was[j], bal[j]);
    }
    if (am == 0) continue;  // uniform over the workgroup
    if constexpr (PACK) {
      // the list: every wave enters the active pixels of its own 2 rows, at the count of active pixels in the rows above (lanes 0..7 hold the row masks)
      const int wvu = __builtin_amdgcn_readfirstlane(wv);
      int n_px = 0, pos = 0;
#pragma unroll
      for (int k = 0; k < TH; k++) {
        const int n = __builtin_popcount(__builtin_amdgcn_readlane(my_rm, k));
        n_px += n;
        pos += k < 2 * wvu ? n : 0;
      }
#pragma unroll
      for (int j = 0; j < 2; j++) {
        if (kb == 0 && ((bal[j] >> px) & 1u)) s_list[pos + __builtin_popcount(bal[j] & ((1u << px) - 1u))] = (uint16_t)pix_code(wvu * 2 + j, px);
        pos += __builtin_popcount(bal[j]);
      }
      // groups of 32 listed pixels, dealt round-robin to the 2 row groups: group rg + 2 j is this wave's j-th (at most TH / 2 of them)
      const int n_grp = (n_px + 31) >> 5, rgu = __builtin_amdgcn_readfirstlane(rg);
      const int nr = n_grp > rgu ? (n_grp - rgu + 1) >> 1 : 0;
      const uint32_t need = am | (am << 1) | (am << 2);  // halo rows some active row reads
      stage_tile64<CIN, TH>(s_in, x, b, H, W, 0, y0, x0, need);
      __syncthreads();  // also publishes s_list
      int codes = 0, n_g[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int g = rgu + 2 * j;
        n_g[j] = min(max(n_px - 32 * g, 0), 32);
        if (j < nr && px < n_g[j]) codes |= (int)s_list[32 * g + px] << (8 * j);  // lanes past the last pixel read pixel (0, 0) and are not stored
      }
      const int64_t t0 = (((int64_t)b * H + y0) * W + x0) * COUT;  // tile origin
#define PNX_PIX_X(N_) conv_pix_x<N_, CIN, COUT, HAS_RES>(s_in, x, wfrag, bias, HAS_RES ? res + t0 : nullptr, codes, n_g, y + t0, b, H, W, y0, x0, need, mg0, relu, px, kb, lane, hsel)
      switch (nr) {  // wave-uniform; every case runs the same barriers
        case 0: PNX_PIX_X(0); break;
        case 1: PNX_PIX_X(1); break;
        case 2: PNX_PIX_X(2); break;
        case 3: PNX_PIX_X(3); break;
        default: PNX_PIX_X(4); break;
      }
#undef PNX_PIX_X
      // inactive pixels of active rows: the row form stores their zeros with the row; here the pass-0 unit zeroes, for all COUT channels, those that went
      // stale -- written before this launch (row_dirty; without one, all of them) and inactive now.  Other bytes than any pass's consumers write, so no order
      // between the units is needed.  After the pass's stores: a store ahead of the tap loop's loads would stall them.
      // Lane L writes chunk L & 15 of pixel c0 + (L >> 4): a store instruction covers 4 consecutive pixels x 256 bytes = 8 complete 128-byte lines.
      if (hsel != 0) continue;
      int l = lane;
      asm volatile("" : "+v"(l));  // opaque: the per-lane offset is recomputed here, not held across the tap loop
      const uint32_t cols = W - x0 >= 32 ? 0xffffffffu : (1u << (W - x0)) - 1u;  // columns inside the image
#pragma unroll
      for (int j = 0; j < 2; j++) {
        const int rr = wvu * 2 + j;
        const uint32_t stale = rd_held(row_dirty, was[j]) & ~bal[j] & cols;  // wave-uniform
        if (!((am >> rr) & 1u) || y0 + rr >= H || stale == 0) continue;
        char* const row = reinterpret_cast<char*>(y + t0) + (uint32_t)(rr * W * COUT * 2);
#pragma unroll 1
        for (int c0 = 0; c0 < 32; c0 += 4) {
          if (((stale >> c0) & 15u) == 0) continue;
          const int p = c0 + (l >> 4);
          if ((stale >> p) & 1u) {
#pragma unroll
            for (int h = 0; h < NH; h++) *reinterpret_cast<uint4*>(row + (uint32_t)(p * COUT * 2 + h * 256 + (l & 15) * 16)) = make_uint4(0, 0, 0, 0);
          }
        }
      }
      continue;
    }
    int nr = 0;
    int rbase[4], rrow[4];
    {  // the active rows, dealt round-robin to the 2 row groups
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
      rbase[j] = rrow[j] * HW_ * 8;
      rmask[j] = j < nr ? __builtin_amdgcn_readfirstlane(s_rowmask[rrow[j]]) : 0u;
      yrow[j] = y + (((int64_t)b * H + (y0 + rrow[j])) * W + x0) * COUT;
    }
    const uint32_t need = am | (am << 1) | (am << 2);  // halo rows some active row reads
    stage_tile64<CIN, TH>(s_in, x, b, H, W, 0, y0, x0, need);
    __syncthreads();
#define PNX_ROWS_X(N_) conv_rows_x<(N_ <= NRMAX ? N_ : NRMAX), CIN, COUT, HAS_RES>(s_in, x, wfrag, bias, res, rrow, rbase, rmask, yrow, b, H, W, y0, x0, need, mg0, relu, px, kb, lane, hsel)
    switch (nr) {  // wave-uniform; every case runs the same barriers
      case 0: PNX_ROWS_X(0); break;
      case 1: PNX_ROWS_X(1); break;
      case 2: PNX_ROWS_X(2); break;
      case 3: PNX_ROWS_X(3); break;
      default: PNX_ROWS_X(4); break;
    }
#undef PNX_ROWS_X
  }
  sched_done(slot);
}

// pack: the packed-pixel form (masked 128 -> 128 / 256 -> 256 only; the caller decides)
template <int CIN, int COUT>
int launch_ldsx(const ConvArgs& a, bool pack = false) {
  const int slot = a.mask != nullptr ? next_sched_slot() : -1;
  int64_t nb = (int64_t)a.B * ((a.H + L128_TH - 1) / L128_TH) * ((a.W + 31) / 32) * ((COUT + 127) / 128);  // work units = (tile, pass)
  if (nb > 512) nb = 512;  // resident workgroups: 2 per CU (registers)
  if constexpr (CIN == COUT) {
    if (pack && a.mask != nullptr) {
      if (a.res != nullptr)
        k_conv3x3_ldsx<CIN, COUT, true, true><<<(unsigned)nb, 256, 0, a.st>>>(a.x, a.wfrag, a.bias, a.res, a.mask, a.y, a.B, a.H, a.W, a.relu, a.row_dirty, slot,
                                                                            a.tlist, a.tcount);
      else
        k_conv3x3_ldsx<CIN, COUT, false, true><<<(unsigned)nb, 256, 0, a.st>>>(a.x, a.wfrag, a.bias, nullptr, a.mask, a.y, a.B, a.H, a.W, a.relu, a.row_dirty, slot,
                                                                             a.tlist, a.tcount);
      PNX_LAUNCH_CHECK();
      return PNX_OK;
    }
  }
  if (a.res != nullptr)
    k_conv3x3_ldsx<CIN, COUT, true><<<(unsigned)nb, 256, 0, a.st>>>(a.x, a.wfrag, a.bias, a.res, a.mask, a.y, a.B, a.H, a.W, a.relu, a.row_dirty, slot, a.tlist,
                                                                   a.tcount);
  else
    k_conv3x3_ldsx<CIN, COUT, false><<<(unsigned)nb, 256, 0, a.st>>>(a.x, a.wfrag, a.bias, nullptr, a.mask, a.y, a.B, a.H, a.W, a.relu, a.row_dirty, slot, a.tlist,
                                                                    a.tcount);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}
