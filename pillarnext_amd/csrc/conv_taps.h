// conv_taps.h -- what the LDS-staged kernels share (included by conv3x3.hip after conv_tile.h; conv_rows.h, conv_s2.h, sephead.h, conv_pc.h and
// sephead_lazy.h build on it): the section timers, dynamic tile scheduling (g_tile_ctr, sched_*, tile_at), the staging of a 64-channel halo tile
// (stage_tile64) and the tap loop over a staged tile (tap_slot, conv_taps).
#pragma once

#ifdef PNX_CONV_TIMERS  // section timers (build with PNX_CONV_TIMERS=1 in the environment of build.py)
__device__ unsigned long long g_conv_T[8];
#define CT_DECL unsigned long long ct_T[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long tk = __builtin_amdgcn_s_memtime();
#define CT_TOCK(k)                                              \
  {                                                             \
    const unsigned long long _n = __builtin_amdgcn_s_memtime(); \
    ct_T[k] += _n - tk;                                         \
    tk = _n;                                                    \
  }
#define CT_FLUSH                                                                     \
  if ((threadIdx.x & 63) == 0) {                                                     \
    for (int k = 0; k < 8; k++) atomicAdd(&g_conv_T[k], ct_T[k]);                     \
  }
#else
#define CT_DECL
#define CT_TOCK(k)
#define CT_FLUSH
#endif

constexpr int LDS_TH = 16;    // rows per workgroup tile
constexpr int LDS_HW = 34;    // halo tile width
constexpr int LDS_NSTAGE = (LDS_TH + 2) * LDS_HW * 8;  // uint4 per staged tile (64 input channels)

__device__ __forceinline__ int lds_swz(int c) { return (c & 7) ^ ((c >> 3) & 1); }

// Dynamic tile scheduling.  Tiles cost anything between "read 16 mask rows" and "4 rows x 9 taps of MFMAs per wave"; dealing
// them to the persistent workgroups round-robin leaves the slowest workgroup 36 % above the mean on a LiDAR sweep (simulated
// from the occupancy), a shared counter 3 %.  Thread 0 draws the NEXT tile at the top of an iteration (the
// atomic's latency hides behind the mask loads), everybody reads it after the iteration's first barrier; the LDS word is
// double-buffered by iteration parity because an empty tile has no second barrier.  g_tile_ctr[slot] = {next tile - gridDim.x,
// finished workgroups}; the last workgroup to finish re-arms the slot, the host rotates 64 slots so that launches in flight
// never share one.
__device__ unsigned int g_tile_ctr[64][2];
// slot < 0: static round-robin (dense inputs: every tile costs the same and the ticket only adds latency).
__device__ __forceinline__ void sched_draw(unsigned int* s_next, int it, int slot) {
  if (slot >= 0 && threadIdx.x == 0) s_next[it & 1] = atomicAdd(&g_tile_ctr[slot][0], 1u);
}
__device__ __forceinline__ int64_t sched_next(const unsigned int* s_next, int it, int slot, int64_t tile) {
  return slot >= 0 ? (int64_t)s_next[it & 1] + gridDim.x : tile + gridDim.x;
}
// Depth-2 pipeline of the tile loops: iteration `it` works on index A, already knows index B (its mask bytes are requested during
// A) and draws index C.  Indices 0..2G-1 are dealt statically (G = gridDim.x), the tickets continue from 2G.  (Drawing the first B
// by ticket as well put 2 x 512 same-address atomics at the start of every launch: 272 us instead of 228 us for 256 -> 256 at
// 180 x 180, three runs each, no difference at the larger stages.)  With a tile list (pnx_conv_tile_list: the tiles that
// hold an active site or a stale row) an index is a position in the list.
__device__ __forceinline__ int64_t sched_next2(const unsigned int* s_next, int it, int slot, int64_t idx_b) {
  return slot >= 0 ? (int64_t)s_next[it & 1] + 2 * (int64_t)gridDim.x : idx_b + gridDim.x;
}
__device__ __forceinline__ int64_t tile_at(const int32_t* __restrict__ tlist, int64_t idx, int64_t n) {
  if (idx >= n) return -1;
  return tlist != nullptr ? (int64_t)tlist[idx] : idx;
}
__device__ __forceinline__ void sched_done(int slot) {
  if (slot >= 0 && threadIdx.x == 0) {
    __threadfence();
    if (atomicAdd(&g_tile_ctr[slot][1], 1u) == gridDim.x - 1) {
      g_tile_ctr[slot][0] = 0;
      g_tile_ctr[slot][1] = 0;
      __threadfence();
    }
  }
}

// Stage the (TH+2) x 34 halo tile of 64 input channels [ch0, ch0+64) of image b at tile origin (y0, x0).  Thread t owns slot t&7
// of halo column t>>3 (0..31) in every row: a wave covers 8 pixels x 8 slots = 1 KiB of LDS that is contiguous in lane order, so
// the rows go global -> LDS directly (global_load_lds_dwordx4: no VGPRs, no ds_write pass, ALL rows in flight at once instead of
// two register batches); the XOR swizzle is applied on the SOURCE side -- slot k of column c receives chunk k ^ swz(c) of the
// pixel's 128-byte line, so coalescing is unchanged.  LDS-DMA cannot write zeros: cells that are needed but lie outside the image
// get a plain ds_write.  The two remaining columns (32, 33; 16 slots per row) keep the register path.  `need` = halo rows that
// will be read (bit r); other rows keep stale data.  Callers follow with __syncthreads(), which drains the DMA (vmcnt(0)).
template <int CSTRIDE, int TH = LDS_TH>
__device__ __forceinline__ void stage_tile64(uint4* __restrict__ s_in, const uint16_t* __restrict__ x, int b, int H, int W, int ch0, int y0, int x0,
                                             uint32_t need) {
  constexpr int NROW = TH + 2, NEXTRA = NROW * 16;
  static_assert(NEXTRA <= 512, "two slots of the extra columns per thread");
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  const uint16_t* xt = x + (((int64_t)b * H + (y0 - 1)) * W + (x0 - 1)) * CSTRIDE + ch0;  // element (0, 0) of the halo tile
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));  // opaque: keeps per-thread staging addresses from being hoisted out of the tile loop (and spilled)
  const int slot = tid & 7, col = tid >> 3, wbase = (tid >> 6) * 8;  // wbase: first column of this wave
  uint32_t rows_in = (1u << NROW) - 1u;  // halo rows inside the image
  if (y0 == 0) rows_in &= ~1u;
  if (y0 - 1 + NROW > H) rows_in &= (1u << (H - (y0 - 1))) - 1u;
  const bool col_ok = (unsigned)(x0 - 1 + col) < (unsigned)W;
  const uint32_t voff = (uint32_t)(col * CSTRIDE + (slot ^ lds_swz(col)) * 8) * 2u;
#pragma unroll
  for (int r = 0; r < NROW; r++) {
    if (!((need >> r) & 1u)) continue;  // wave-uniform
    if (((rows_in >> r) & 1u) && col_ok) {
      __builtin_amdgcn_global_load_lds((gptr_t)(reinterpret_cast<const char*>(xt + (int64_t)r * W * CSTRIDE) + voff),
                                       (lptr_t)(s_in + (r * LDS_HW + wbase) * 8), 16, 0, 0);
    } else {
      s_in[(r * LDS_HW + col) * 8 + slot] = make_uint4(0, 0, 0, 0);
    }
  }
#pragma unroll
  for (int part = 0; part < (NEXTRA + 255) / 256; part++) {
    const int e = part * 256 + tid;  // slot of the two extra columns: row e>>4, column 32 + ((e>>3)&1), chunk e&7
    const int re = e >> 4, ce = 32 + ((e >> 3) & 1);
    if (e < NEXTRA && ((need >> re) & 1u)) {
      uint4 qe = make_uint4(0, 0, 0, 0);
      if (((rows_in >> re) & 1u) && (unsigned)(x0 - 1 + ce) < (unsigned)W)
        qe = *reinterpret_cast<const uint4*>(xt + ((int64_t)re * W + ce) * CSTRIDE + (e & 7) * 8);
      s_in[(re * LDS_HW + ce) * 8 + ((e & 7) ^ lds_swz(ce))] = qe;
    }
  }
}

// One 64-output-channel pass of a wave over its NR rows: 9 taps x 4 k-steps, software-pipelined in registers -- B fragments one
// k-step ahead (LDS), weight fragments one tap ahead (L1/L2; each register pair is refilled for the next tap right after its
// last MFMA of this tap).
// STRIDE 2 (stage_tile64_s2): a halo row is [even input columns 0..31 | odd input columns 32..64] and has S2_RS slots, so that the 32
// lanes of a tap still read 32 consecutive slots: tap column dx of output pixel px is input column 2 px + dx - 1 (relative to the
// tile), i.e. slot px of the even plane for dx = 1 and slot px + dx/2 of the odd plane otherwise; row dy of output row r is halo
// row 2 r + dy (the caller folds 2 r into rbase).
constexpr int S2_RS = 65;
template <int STRIDE>
__device__ __forceinline__ int tap_slot(int px, int dx) {
  return STRIDE == 1 ? px + dx : (dx == 1 ? px : 32 + px + (dx >> 1));
}

// The tap loop, fully unrolled (round 6): 36 k-steps (9 taps x 4 chunks of 16 input channels) of one 64-channel slab, software-pipelined in the source --
// B fragments TAPS_PD k-steps ahead (LDS), weight fragments TAPS_WD k-steps ahead (L1 / L2), both in register rings indexed by compile-time constants
// (no copies, no branches); a sched_barrier per k-step keeps hipcc from sinking the loads back to their users.  What made the full unroll spill in
// round 2 was hoisting: 36 x NR slot addresses and 36 weight pointers are loop-invariant over the persistent tile loop, so hipcc computed all of
// them at kernel entry.  Now the weight address is a wave-uniform base (scalar registers) + lane * 16, and the per-lane part of a slot address goes
// through an opaque asm at every k-step.  Measured (profiles/r06_conv_pc_ab.txt): deeper prefetch (2-3 k-steps, 6-8 fragments) is slower -- the loop was
// never latency-bound, see DESIGN.md section 4 on the power ceiling.
// History (removed forms, see git history): rounds 2-5 ran a ROLLED 9-iteration tap loop whose `tap < 8` tests compiled to branches inside the loop; its
// per-k-step sched_barrier dates from round 5 (profiles/r05_conv_sched.txt: without the fence 128 / 256 channels ran 3-4 % slower; s_setprio around the
// MFMAs: no gain).  Weights by per-lane global loads instead of the buffer resource were the A/B reference of profiles/r06_conv_pc_ab.txt.
constexpr int TAPS_PD = 1;  // B-fragment lookahead in k-steps
constexpr int TAPS_WD = 4;  // depth of the weight-fragment ring (the default of conv_taps' WD)
// MB = 32-channel output tiles per wave (2: the row-split kernels; 1: the producer / consumer kernel, whose waves split the output channels).
// PIX (the packed-pixel form of k_conv3x3_ldsx): rbase[0] is not a wave-uniform row base but this lane's own pixels in the NR pixel groups, one
// pix_code byte per group (byte j: group j), and the slot of every group is recomputed per j from an opaque copy of that word.
// PIXB = 16 (the packed form of k_conv3x3_pc: 16-row tiles, 9-bit codes): half-word codes, groups 0, 1 in rbase[0] and groups 2, 3 in rbase[1].
template <int NR, int MTALL, int CB = 4, int STRIDE = 1, int MB = 2, int WD = TAPS_WD, bool PIX = false, int PIXB = 8>
__device__ __forceinline__ void conv_taps(v16f (&acc)[NR][MB], const uint4* __restrict__ s_in, const uint4* __restrict__ wfrag, const int (&rbase)[4],
                                          int mg, int px, int kb, int lane, int kstep0 = 0) {
  constexpr int RS = STRIDE == 1 ? LDS_HW : S2_RS;
  constexpr int KS = 36, PD = TAPS_PD;
  // weight fragment (k-step ks -> tap, chunk cbl; output tile m): a wave-uniform base + lane * 16
  const uint4* wu = wfrag + (int64_t)__builtin_amdgcn_readfirstlane(kstep0 * MTALL + mg) * 64;
  // weights through a buffer resource: scalar base + scalar offset + lane * 16, one instruction per fragment and no per-lane 64-bit address
  const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(wu), 0, 0x7fffffff, 0x00020000);
  const int wlo = lane * 16;
  auto wload = [&](int ks, uint4 (&dst)[MB]) {
    const int grp = ks / 3, cbl = grp & 3;
    const int tap = (ks % 3) * 3 + (grp >> 2);  // dy * 3 + dx
#pragma unroll
    for (int m = 0; m < MB; m++) {
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(wrs, wlo, (((tap * CB + cbl) * MTALL + m) * 64) * 16, 0);
      dst[m] = make_uint4(r.x, r.y, r.z, r.w);
    }
  };
  // k-step order: ks = (dx * 4 + cbl) * 3 + dy.  The three dy taps of a (column dx, chunk cbl) group read the SAME per-lane slots one halo row apart, i.e.
  // the same address registers with another immediate offset: NR address adds per three k-steps instead of per k-step.  The per-lane slot of a group --
  // c * 8 + ((2 cbl + kb) ^ swz(c)), c = tap_slot(px, dx) -- is recomputed from an OPAQUE copy of px at every group (6 VALU per 3 k-steps): written as
  // loop-invariant arrays hipcc kept them (and, before that, all 36 x NR slot addresses) live across the persistent tile loop and spilled.
  int addr[NR];
  auto group_addr = [&](int grp) {
    const int dx = grp >> 2, cbl = grp & 3;
    if constexpr (PIX && PIXB == 16) {
      int p[2] = {rbase[0], rbase[1]};
      asm volatile("" : "+v"(p[0]));
      if (NR > 2) asm volatile("" : "+v"(p[1]));
#pragma unroll
      for (int j = 0; j < NR; j++) {
        const int q = (p[j >> 1] >> (16 * (j & 1))) & 0xffff;
        const int c = tap_slot<STRIDE>(q & 31, dx);
        addr[j] = (q >> 5) * (RS * 8) + c * 8 + ((2 * cbl + kb) ^ lds_swz(c));
        asm volatile("" : "+v"(addr[j]));
      }
      return;
    } else if constexpr (PIX) {
      int p = rbase[0];
      asm volatile("" : "+v"(p));
#pragma unroll
      for (int j = 0; j < NR; j++) {
        const int q = (p >> (8 * j)) & 255;
        const int c = tap_slot<STRIDE>(q & 31, dx);
        addr[j] = (q >> 5) * (RS * 8) + c * 8 + ((2 * cbl + kb) ^ lds_swz(c));
        asm volatile("" : "+v"(addr[j]));  // the dy rows stay immediate offsets of one address (hipcc would otherwise distribute the row term over them)
      }
      return;
    }
    int p = px;
    asm volatile("" : "+v"(p));
    const int c = tap_slot<STRIDE>(p, dx);
    const int a = c * 8 + ((2 * cbl + kb) ^ lds_swz(c));
#pragma unroll
    for (int j = 0; j < NR; j++) addr[j] = a + rbase[j];
  };
  auto bload = [&](int ks, uint4 (&dst)[NR]) {
    const int dy = ks % 3;
    if (dy == 0) group_addr(ks / 3);
#pragma unroll
    for (int j = 0; j < NR; j++) dst[j] = s_in[addr[j] + dy * (RS * 8)];
  };
  uint4 w[WD][MB];
  uint4 q[PD + 1][NR];
#pragma unroll
  for (int k = 0; k < WD; k++) wload(k, w[k]);
#pragma unroll
  for (int k = 0; k < PD; k++) bload(k, q[k]);
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    if (ks + PD < KS) bload(ks + PD, q[(ks + PD) % (PD + 1)]);
#pragma unroll
    for (int j = 0; j < NR; j++) {
      const el8 bfr = __builtin_bit_cast(el8, q[ks % (PD + 1)][j]);
#pragma unroll
      for (int m = 0; m < MB; m++) acc[j][m] = PNX_MFMA32(__builtin_bit_cast(el8, w[ks % WD][m]), bfr, acc[j][m]);
    }
    if (ks + WD < KS) wload(ks + WD, w[ks % WD]);
    __builtin_amdgcn_sched_barrier(0);  // (measured, profiles/r06_conv_pc_ab.txt: without the fence -1.5 % end to end; an explicit one-load-behind-each-MFMA sched_group_barrier pattern: no difference)
  }
}
