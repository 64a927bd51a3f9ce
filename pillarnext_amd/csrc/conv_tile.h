// conv_tile.h -- what every kernel of conv3x3.hip shares per accumulator tile (included by conv3x3.hip, first of its headers): the element type and
// the MFMA macros of the bf16 / fp16 builds, the epilogue (pack_tile, transpose_row64 / _row32, store_row64 / _row32, store_tile_f32), the bias and
// residual helpers, and ConvArgs, the host-side argument bundle of the inference launchers.
#pragma once

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// Element type of activations and weights.  conv3x3.hip is compiled TWICE (pillarnext_amd/build.py): as is for bf16 (entry points pnx_*_bf16,
// plus the type-independent tile-list helpers) and with -DPNX_CONV_F16 for IEEE half (pnx_*_f16: BASELINE configs[4], the fp16 Waymo network).
// Everything between the loads and the stores is fp32 either way; the type shows in exactly four places: the MFMA opcode, the pack of the
// epilogue (round to nearest even), the widening of the residual, and the rounding of the lazy head's intermediate.
#ifdef PNX_CONV_F16
typedef _Float16 el8 __attribute__((ext_vector_type(8)));
typedef _Float16 el2 __attribute__((ext_vector_type(2)));
#define PNX_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
#define PNX_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#define PNX_CONV_FN(name) name##_f16
// fp32 bit patterns of the low / high element of a packed pair
__device__ __forceinline__ uint32_t el_lo_bits(uint32_t w) { return __float_as_uint((float)__builtin_bit_cast(el2, w)[0]); }
__device__ __forceinline__ uint32_t el_hi_bits(uint32_t w) { return __float_as_uint((float)__builtin_bit_cast(el2, w)[1]); }
#else
typedef __bf16 el8 __attribute__((ext_vector_type(8)));
typedef __bf16 el2 __attribute__((ext_vector_type(2)));
#define PNX_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#define PNX_MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#define PNX_CONV_FN(name) name##_bf16
__device__ __forceinline__ uint32_t el_lo_bits(uint32_t w) { return w << 16; }
__device__ __forceinline__ uint32_t el_hi_bits(uint32_t w) { return w & 0xffff0000u; }
#endif
// two fp32 -> one packed pair, round to nearest even (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32: one instruction per channel pair)
__device__ __forceinline__ uint32_t pack_el(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, el2));
}
// x rounded to the element type and back (what a value becomes when it goes through a stored intermediate)
__device__ __forceinline__ float round_el(float x) { return __uint_as_float(el_lo_bits(pack_el(x, 0.f))); }

// Epilogue.  The MFMA leaves lane (px, kb) with channels {8g + 4kb + i} of pixel px: four 8-byte pieces per 32-channel tile,
// i.e. 32 scattered 8-byte stores per row of 32 pixels.  Measured, that store pattern -- not the MFMAs -- bounded the kernel
// (42-50 % of wave time: the vector-memory path pays per distinct line an instruction touches, here 32 lines for 512 bytes).
// Two steps fix it:
//  (1) pack_tile: v_permlane32_swap trades the odd 4-channel groups between the two half-waves (MI355X guide T21) so each lane
//      holds 8 consecutive channels; residual add / ReLU / bf16 rounding / active-site mask happen here in fp32;
//  (2) store_row64: the four 16-byte slots a lane holds for one pixel (64 output channels = one 128-byte line, lanes kb=0/1
//      holding the even/odd chunks) are transposed across lanes with ds_bpermute (LDS crossbar, no LDS storage): slot index
//      <-> pixel-octet index, the classic rotate / permute / rotate scheme (16 bpermutes + 64 selects per row).  Afterwards
//      store d of lane L is chunk L&7 of pixel 8d + (L>>3): every store instruction writes 8 complete 128-byte lines.
// Both must be called by all 64 lanes.
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// `res` (optional): the residual lines of this lane's pixel for the tile, res[t] = channels 16 t + 8 kb + 0..7 -- exactly the 8 consecutive channels the
// lane holds after the swap, added in fp32 before the ReLU.
__device__ __forceinline__ void pack_tile(const v16f& a, bool act, int relu, uint4 (&out)[2], const uint4* res = nullptr) {
#pragma unroll
  for (int t = 0; t < 2; t++) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a[8 * t + i]), __float_as_uint(a[8 * t + 4 + i]), false, false);
      v[i] = __uint_as_float(r.x);
      v[4 + i] = __uint_as_float(r.y);
    }
    if (res != nullptr) {
      const uint4 q = res[t];
      v[0] += __uint_as_float(el_lo_bits(q.x)), v[1] += __uint_as_float(el_hi_bits(q.x)), v[2] += __uint_as_float(el_lo_bits(q.y)), v[3] += __uint_as_float(el_hi_bits(q.y));
      v[4] += __uint_as_float(el_lo_bits(q.z)), v[5] += __uint_as_float(el_hi_bits(q.z)), v[6] += __uint_as_float(el_lo_bits(q.w)), v[7] += __uint_as_float(el_hi_bits(q.w));
    }
    if (relu) {
#pragma unroll
      for (int i = 0; i < 8; i++) v[i] = fmaxf(v[i], 0.f);
    }
    uint4 p;
    p.x = pack_el(v[0], v[1]);
    p.y = pack_el(v[2], v[3]);
    p.z = pack_el(v[4], v[5]);
    p.w = pack_el(v[6], v[7]);
    if (!act) p = make_uint4(0, 0, 0, 0);
    out[t] = p;
  }
}

__device__ __forceinline__ void cswap(bool c, uint4& x, uint4& y) {
  const uint4 a = x, b = y;
  x.x = c ? b.x : a.x, x.y = c ? b.y : a.y, x.z = c ? b.z : a.z, x.w = c ? b.w : a.w;
  y.x = c ? a.x : b.x, y.y = c ? a.y : b.y, y.z = c ? a.z : b.z, y.w = c ? a.w : b.w;
}

// R[s], s = 2*(tile within the 64-channel group) + t: chunk 2s + kb of pixel px = lane & 31.  On return R[d] of lane L is chunk
// L & 7 of pixel 8d + (L >> 3).
__device__ __forceinline__ void transpose_row64(uint4 (&R)[4], int lane) {
  const int a_src = (lane & 31) >> 3;       // pixel octet of this lane as a source
  const int s_dst = (lane & 7) >> 1;        // slot this lane stores as a destination
  // rotate: U[k] = R[k ^ a_src]
  cswap(a_src & 1, R[0], R[1]);
  cswap(a_src & 1, R[2], R[3]);
  cswap(a_src & 2, R[0], R[2]);
  cswap(a_src & 2, R[1], R[3]);
  // permute: round k fetches slot register k of source lane (octet k ^ s_dst, pixel-in-octet L>>3, half L&1)
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int src = (8 * (k ^ s_dst) + (lane >> 3)) + 32 * (lane & 1);
    R[k].x = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].x);
    R[k].y = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].y);
    R[k].z = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].z);
    R[k].w = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].w);
  }
  // rotate back: D[d] = V[d ^ s_dst]
  cswap(s_dst & 1, R[0], R[1]);
  cswap(s_dst & 1, R[2], R[3]);
  cswap(s_dst & 2, R[0], R[2]);
  cswap(s_dst & 2, R[1], R[3]);
}

// `row` (wave-uniform) points at channel 0 of the 64-channel group for pixel 0 of the 32-pixel row segment; pixels >= n_valid
// are not stored; CSTRIDE = channels per pixel.  Uniform base + 32-bit lane offset: no per-store 64-bit address arithmetic.
template <int CSTRIDE>
__device__ __forceinline__ void store_row64(const uint4 (&D)[4], uint16_t* __restrict__ row, int n_valid, int lane) {
  const uint32_t voff = (uint32_t)((lane >> 3) * CSTRIDE + (lane & 7) * 8) * 2u;
#pragma unroll
  for (int d = 0; d < 4; d++) {
    const int P = 8 * d + (lane >> 3);
    if (P < n_valid) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(row) + voff + (uint32_t)(d * 8 * CSTRIDE * 2)) = D[d];
  }
}

// ---- the same for a wave that holds ONE 32-channel tile (the producer / consumer kernel, the 64 -> 128 stride-2 kernel): 64-byte half lines
// R[t], t = 0, 1: chunk 2t + kb (8 channels = 16 bytes) of the wave's 32-channel group for pixel px = lane & 31 (what pack_tile leaves).
// On return R[d] of lane L is chunk L & 3 of pixel 16 d + (L >> 2): one store instruction writes 16 complete 64-byte half lines.
__device__ __forceinline__ void transpose_row32(uint4 (&R)[2], int lane) {
  cswap((lane & 16) != 0, R[0], R[1]);  // rotate by the pixel half of the source: U[k] = R[k ^ (px >> 4)]
  const int T = (lane >> 1) & 1;        // register (t) this lane wants as a destination
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int src = 16 * (k ^ T) + (lane >> 2) + 32 * (lane & 1);
    R[k].x = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].x);
    R[k].y = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].y);
    R[k].z = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].z);
    R[k].w = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)R[k].w);
  }
  cswap(T != 0, R[0], R[1]);  // round k delivered the piece of store k ^ T
}

// `row` (wave-uniform): channel 0 of the wave's 32-channel group at pixel 0 of the row segment
template <int CSTRIDE>
__device__ __forceinline__ void store_row32(const uint4 (&D)[2], uint16_t* __restrict__ row, int n_valid, int lane) {
  const uint32_t voff = (uint32_t)((lane >> 2) * CSTRIDE + (lane & 3) * 8) * 2u;
#pragma unroll
  for (int d = 0; d < 2; d++) {
    const int P = 16 * d + (lane >> 2);
    if (P < n_valid) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(row) + voff + (uint32_t)(d * 16 * CSTRIDE * 2)) = D[d];
  }
}

// The accumulators start from the (folded-BN) bias: register i of a lane's 32-channel tile is channel (i&3) + 8*(i>>2) + 4*kb.
// fp32 epilogue of the three-product kernels: the accumulator tile as it is, lane (px, kb) writing channels 8g + 4kb + 0..3 of its pixel (the two half-waves
// complete 32 bytes per pixel and g); inactive sites get zeros.  `row`: channel 0 of the tile at pixel 0 of the row segment.
template <int COUT>
__device__ __forceinline__ void store_tile_f32(const v16f& a, bool act, float* __restrict__ row, int n_valid, int px, int kb) {
  if (px >= n_valid) return;
  float* p = row + (int64_t)px * COUT + 4 * kb;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    float4 v = make_float4(a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]);
    if (!act) v = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(p + 8 * g) = v;
  }
}

__device__ __forceinline__ v16f bias_tile(const float* __restrict__ bias, int cbase, int kb) {
  v16f r;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float4 q = *reinterpret_cast<const float4*>(bias + cbase + 8 * g + 4 * kb);
    r[4 * g + 0] = q.x, r[4 * g + 1] = q.y, r[4 * g + 2] = q.z, r[4 * g + 3] = q.w;
  }
  return r;
}

// The residual (identity branch of a BasicBlock) is folded into the accumulators BEFORE the MFMAs, like the bias: its lines are
// loaded 16 bytes per lane (the layout pack_tile produces) and moved into MFMA register order by the same half-wave swap, which
// is its own inverse.  The loads overlap the staging of the input tile and the epilogue is left without a single load -- on
// gfx9 a load's s_waitcnt also waits for every OLDER store, so a load between stores serialises on HBM write acknowledgements.
// `res_px` = residual line of this lane's pixel (+ channel base of the 64-channel group); must be called by all 64 lanes.
__device__ __forceinline__ void load_residual(uint4 (&rq)[2][2], const uint16_t* __restrict__ res_px, bool act, int kb) {
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int t = 0; t < 2; t++) {
      rq[m][t] = make_uint4(0, 0, 0, 0);
      if (act) rq[m][t] = *reinterpret_cast<const uint4*>(res_px + m * 32 + 16 * t + 8 * kb);
    }
}
// the same lines from a WAVE-UNIFORM row pointer (pixel 0 of the row segment, channel base of the 64-channel group) + one per-lane byte offset
// ((px * CSTRIDE + 8 kb) * 2, the same for every row): scalar base + 32-bit lane offset + immediate, no 64-bit pointer per row in vector registers
__device__ __forceinline__ void load_residual_u(uint4 (&rq)[2][2], const uint16_t* __restrict__ row, uint32_t lane_off, bool act) {
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int t = 0; t < 2; t++) {
      rq[m][t] = make_uint4(0, 0, 0, 0);
      if (act) rq[m][t] = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(row) + lane_off + (uint32_t)((m * 32 + 16 * t) * 2));
    }
}
__device__ __forceinline__ void add_residual(v16f (&acc2)[2], const uint4 (&rq)[2][2]) {
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const uint4 r = rq[m][t];
      const uint32_t lo[4] = {el_lo_bits(r.x), el_hi_bits(r.x), el_lo_bits(r.y), el_hi_bits(r.y)};
      const uint32_t hi[4] = {el_lo_bits(r.z), el_hi_bits(r.z), el_lo_bits(r.w), el_hi_bits(r.w)};
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const u32x2 q = __builtin_amdgcn_permlane32_swap(lo[i], hi[i], false, false);
        acc2[m][8 * t + i] += __uint_as_float(q.x);
        acc2[m][8 * t + 4 + i] += __uint_as_float(q.y);
      }
    }
}

// ---- the row_dirty array of a persistent output buffer (include/pnx.h).  ONE allocation, n_seg = batch * ho * ceil(wo / 32) row segments:
//   flag     uint8[n_seg]   1 = the segment holds an active site (what pnx_conv_tile_list reads)
//   written  uint32[n_seg]  bit p = pixel p of the segment may hold non-zero data
// A launch zeroes `written & ~current` -- the pixels that went stale -- and leaves written = current, flag = (current != 0).  Before the masks existed a
// packed launch re-zeroed every inactive pixel of every flagged segment: 0.6-0.8 zero lines per active line, most of them over zeros.
struct RowDirtyWs {
  uint8_t* flag;
  uint32_t* written;
  size_t bytes;
};
inline RowDirtyWs row_dirty_carve(void* base, int64_t n_seg) {
  RowDirtyWs w;
  PnxCarver c(base);
  w.flag = c.take<uint8_t>((size_t)n_seg);
  w.written = c.take<uint32_t>((size_t)n_seg);
  w.bytes = c.used();
  return w;
}
// What the kernels take.  stale = 0 (PNX_CONV_STALE=0, the cross-check): zero as if every pixel of a written segment held data; the masks are kept all the same.
struct RowDirty {
  uint8_t* flag;      // nullptr: no array -- the output is a plain buffer, every inactive pixel is zeroed
  uint32_t* written;
  int stale;
};
// the written word of segment i (all pixels without an array), and the pixels of it a launch has to treat as holding data
__device__ __forceinline__ uint32_t rd_load(const RowDirty& rd, int64_t i) { return rd.written != nullptr ? rd.written[i] : 0xffffffffu; }
__device__ __forceinline__ uint32_t rd_held(const RowDirty& rd, uint32_t w) { return rd.stale != 0 || w == 0 ? w : 0xffffffffu; }
// one lane: segment i had the written word `was` and now holds the active pixels `now`
__device__ __forceinline__ void rd_store(const RowDirty& rd, int64_t i, uint32_t was, uint32_t now) {
  if (rd.written == nullptr) return;
  if ((was != 0) != (now != 0)) rd.flag[i] = now != 0 ? 1 : 0;
  if (was != now) rd.written[i] = now;
}

// What one pnx_conv3x3 call hands to whichever inference launcher its ladder picks (host side only): the entry point's arguments, checked, with the
// pointers already typed as the kernels take them.  H, W: input size.  The launchers add what is theirs alone (pack, the output size).
struct ConvArgs {
  const uint16_t* x;
  const uint4* wfrag;
  const float* bias;
  const uint16_t* res;
  const uint8_t* mask;
  uint16_t* y;
  int B, H, W, relu;
  RowDirty row_dirty;
  const int32_t *tlist, *tcount;
  hipStream_t st;
};
