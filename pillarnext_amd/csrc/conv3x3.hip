// conv3x3.hip -- masked 3x3 convolution for the dense stand-in of the sparse backbone, gfx950.
//
// One kernel = SubMConv2d / SparseConv2d(k=3, stride s, pad 1) + folded BatchNorm + [residual] + ReLU + active-site mask of
// det3d/models/utils/sparse_conv.py:16-63, on bf16 NHWC tensors:
//        y[b, oy, ox, :] = mask[b, oy, ox] * relu( sum_{ky,kx} x[b, oy*s+ky-1, ox*s+kx-1, :] . W[:, ky, kx, :] + bias [+ res] )
//
// Implicit GEMM on v_mfma_f32_32x32x16_bf16 with M = output channels, N = 32 consecutive output pixels of one image row,
// K = 9 taps x CIN.  The B fragment of a lane is 8 consecutive input channels of one pixel = ONE 16-byte NHWC read, the A
// fragments (weights) are pre-arranged on the host in fragment order.  Kernels of this translation unit, and the file that holds each:
//   k_conv3x3          (this file) direct: B fragments straight from L1/L2 (strided layers; every input line is re-read 9 times)
//   k_conv3x3_pc       (conv_pc.h, round 6; default for 64 -> 64) producer / consumer form: 4 producer waves stage the NEXT tile by LDS-DMA into a ring of
//                      slots while 8 consumer waves (row groups x 32-channel groups) run the taps; one workgroup per CU; with a mask, 64 -> 64
//                      computes the tile's active pixels packed in groups of 32 (PNX_CONV_PACK bit 1, default on; see pc_pix64)
//   k_conv3x3_lds      (conv_rows.h) stride 1, 64 input channels: 18x34 halo tile staged once in LDS, 1..7 passes of 64 output channels
//   k_conv3x3_ldsx     (conv_rows.h) stride 1, 128 -> 128 and 256 -> 256: 10x34 tile, 64-channel input slabs through one LDS buffer under live
//                      accumulators, 128 output channels per pass; with a mask, 128 -> 128 and 256 -> 256 compute the tile's active pixels
//                      packed in groups of 32 (PNX_CONV_PACK bit 0, default on; see conv_pix_x)
//   k_conv3x3_s2       (conv_s2.h) stride 2: the entry convolutions 64 -> 128, 128 -> 256, 256 -> 256; also the fp32 training forward on 2 or 3 pieces
//   k_dgrad_s2         (conv_dgrad_s2.h, bf16 build only) data gradient of the stride-2 layers
//   k_deconv2x2_64,
//   k_sephead_out      (sephead.h) the deblock's transposed convolution; block-diagonal 16-output convolution closing the merged SepHead branches
//   k_sephead_lazy     (sephead_lazy.h) the regression branches of the SepHead at the decoder's candidate cells only
//   k_tile_list        (this file) the tiles that hold an active site or a stale row
// Shared by all of them: conv_tile.h (element type, MFMA macros, epilogue, bias / residual helpers, ConvArgs) and conv_taps.h (section timers, tile
// scheduling, stage_tile64, the tap loop conv_taps).  The headers are included here and nowhere else, in the order the code was written in: what a
// header uses stands in the headers before it.  This file keeps the direct kernel, the tile list, launch_lds, launch and every extern "C" entry point.
// Rows/tiles without an active site skip their MFMAs (and, with row_dirty, their HBM traffic) -- that is where the sparsity of
// the BEV map pays in a dense layout; bias and residual start the accumulators, the epilogue (ReLU, mask, bf16 pack) writes
// complete 128-byte lines.  MIOpen needs a conv pass plus a separate elementwise pass for the same result.  DESIGN.md section 4
// has the measurements each of these choices came from.
#include "pnx_common.h"

namespace {

#include "conv_tile.h"

// wfrag layout: [kstep = tap * (CIN/16) + cb][mtile][lane][8 bf16], lane = kb*32 + n :
//   W[out = mtile*32 + n][ky][kx][cin = cb*16 + 8*kb + e]   (host: pillarnext_amd/ops.py::conv3x3_pack_weights)
template <int CIN, int COUT, int STRIDE, bool W_LDS>
__global__ __launch_bounds__(256, 2) void k_conv3x3(const uint16_t* __restrict__ x, const uint4* __restrict__ wfrag,
                                                 const float* __restrict__ bias, const uint16_t* __restrict__ res,
                                                 const uint8_t* __restrict__ mask, uint16_t* __restrict__ y, int B, int H, int W, int Ho,
                                                 int Wo, int relu, RowDirty row_dirty) {
  constexpr int CB = CIN / 16, MT = COUT / 32, KSTEPS = 9 * CB;
  constexpr int NT = (MT <= 2) ? 4 : 2;  // rows of 32 pixels per wave: 8 accumulators either way
  extern __shared__ uint4 s_w[];         // KSTEPS * MT * 64 uint4 when W_LDS
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int px = lane & 31, kb = lane >> 5;
  if (W_LDS) {
    for (int i = threadIdx.x; i < KSTEPS * MT * 64; i += 256) s_w[i] = wfrag[i];
    __syncthreads();
  }
  const int tiles_x = (Wo + 31) >> 5, tiles_y = (Ho + NT - 1) / NT;
  const int64_t n_tiles = (int64_t)B * tiles_y * tiles_x;
  for (int64_t tile = (int64_t)blockIdx.x * 4 + wv; tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
    const int tx = (int)(tile % tiles_x);
    const int ty = (int)((tile / tiles_x) % tiles_y);
    const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
    const int ox = tx * 32 + px, oy0 = ty * NT;
    // ---- active sites of the tile
    bool act[NT];
    bool any_row[NT];
    bool any = false;
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const int oy = oy0 + j;
      const bool in = ox < Wo && oy < Ho;
      act[j] = in && (mask == nullptr || mask[((int64_t)b * Ho + oy) * Wo + ox] != 0);
      any_row[j] = __ballot(act[j]) != 0;
      any = any || any_row[j];
    }
    // rows without an active site are written (as zeros) only when the row segment may hold stale data (see pnx.h: row_dirty); a row form: what it
    // writes it writes whole, so the written mask of a row is its row mask
    bool row_store[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const int oy = oy0 + j;
      row_store[j] = oy < Ho;
      const uint32_t now = (uint32_t)__ballot(act[j]);  // lanes 32..63 repeat the 32 pixels
      if (row_dirty.flag != nullptr && oy < Ho) {
        const int64_t seg = ((int64_t)b * Ho + oy) * tiles_x + tx;
        const uint32_t was = (uint32_t)__builtin_amdgcn_readfirstlane((int)rd_load(row_dirty, seg));
        row_store[j] = any_row[j] || was != 0;
        if (lane == 0) rd_store(row_dirty, seg, was, now);
      }
    }
    v16f acc[NT][MT];
#pragma unroll
    for (int m = 0; m < MT; m++) {
      const v16f bq = bias_tile(bias, m * 32, kb);
#pragma unroll
      for (int j = 0; j < NT; j++) acc[j][m] = bq;
    }

    if (res != nullptr) {
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const bool in = ox < Wo && oy0 + j < Ho;
        const uint16_t* rp = res + (in ? (((int64_t)b * Ho + oy0 + j) * Wo + ox) * COUT : 0);
#pragma unroll
        for (int m0 = 0; m0 < MT; m0 += 2) {
          uint4 rq[2][2];
          load_residual(rq, rp + m0 * 32, act[j], kb);
          v16f a2[2] = {acc[j][m0], acc[j][m0 + 1]};
          add_residual(a2, rq);
          acc[j][m0] = a2[0], acc[j][m0 + 1] = a2[1];
        }
      }
    }

    if (any) {
      for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const uint16_t* src[NT];
        bool ok[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) {
          const int iy = (oy0 + j) * STRIDE + dy, ix = ox * STRIDE + dx;
          ok[j] = any_row[j] && ox < Wo && (oy0 + j) < Ho && iy >= 0 && iy < H && ix >= 0 && ix < W;
          src[j] = x + (((int64_t)b * H + (ok[j] ? iy : 0)) * W + (ok[j] ? ix : 0)) * CIN + 8 * kb;
        }
#pragma unroll
        for (int cb = 0; cb < CB; cb++) {
          const int ks = tap * CB + cb;
          el8 af[MT];
#pragma unroll
          for (int m = 0; m < MT; m++) {
            const uint4 wq = W_LDS ? s_w[(ks * MT + m) * 64 + lane] : wfrag[(ks * MT + m) * 64 + lane];
            af[m] = __builtin_bit_cast(el8, wq);
          }
#pragma unroll
          for (int j = 0; j < NT; j++) {
            if (!any_row[j]) continue;  // wave-uniform
            uint4 q = make_uint4(0, 0, 0, 0);
            if (ok[j]) q = *reinterpret_cast<const uint4*>(src[j] + cb * 16);
            const el8 bfr = __builtin_bit_cast(el8, q);
#pragma unroll
            for (int m = 0; m < MT; m++) acc[j][m] = PNX_MFMA32(af[m], bfr, acc[j][m]);
          }
        }
      }
    }
    // ---- epilogue (see pack_tile / store_row64)
    const int n_valid = Wo - tx * 32;  // pixels of this row segment inside the image (>= 32: all)
#pragma unroll
    for (int j = 0; j < NT; j++) {
      const bool row_in = row_store[j];  // wave-uniform
      if (!row_in) continue;
      uint16_t* row = y + (((int64_t)b * Ho + (oy0 + j)) * Wo + tx * 32) * COUT;
#pragma unroll
      for (int m0 = 0; m0 < MT; m0 += 2) {
        uint4 R[4];
#pragma unroll
        for (int m = 0; m < 2; m++) {
          uint4 pk[2];
          pack_tile(acc[j][m0 + m], act[j], relu, pk);
          R[2 * m] = pk[0], R[2 * m + 1] = pk[1];
        }
        transpose_row64(R, lane);
        store_row64<COUT>(R, row + m0 * 32, row_in ? n_valid : 0, lane);
      }
    }
  }
}

#include "conv_taps.h"
#include "conv_rows.h"
#include "conv_s2.h"
#include "sephead.h"

// ---- tile list: the 32-pixel-wide, `th`-row tiles that hold an active site now or a stale row in one of the persistent output
// buffers (row_dirty).  A 1440 x 1440 sweep leaves 65 % of the 16 x 32 tiles empty, and an empty tile costs the convolution
// kernels a mask read + a barrier (~1.5 us) each.  One THREAD per tile (consecutive lanes read consecutive 32-byte pieces of a mask
// row), the workgroup compacts its hits in LDS and draws ONE range of the list: a wave per tile with an atomic per hit ran 73 us
// on the 32 400 tiles of stage 0 (11 000 same-address atomics at ~13 ns), this form ~10 us.  The list order follows the atomics.
struct DirtySet {
  const uint8_t* p[4];
};
// Round 6: ONE LANE PER ROW of a tile (th <= 16 lanes per tile, 4 tiles per wave) instead of one thread per tile: a thread walked its 16 rows one dependent
// load after the other (38-47 us per stage for 25 MB of mask bytes); now every lane issues its two 16-byte mask loads and its <= 4 flag bytes at once and the
// tile's verdict is an OR across its 16 lanes.
__global__ __launch_bounds__(256) void k_tile_list(const uint8_t* __restrict__ mask, DirtySet ds, int B, int H, int W, int th, int32_t* __restrict__ list,
                                                   int32_t* __restrict__ count) {
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int tiles_x = (W + 31) >> 5, tiles_y = (H + th - 1) / th;
  const int64_t n_tiles = (int64_t)B * tiles_y * tiles_x;
  const int r = lane & 15;                                       // row of the tile this lane looks at (th <= 16)
  const int64_t tile = ((int64_t)blockIdx.x * 4 + wv) * 4 + (lane >> 4);  // 16 tiles per workgroup
  uint32_t acc = 0;
  if (tile < n_tiles && r < th) {
    const int tx = (int)(tile % tiles_x);
    const int ty = (int)((tile / tiles_x) % tiles_y);
    const int b = (int)(tile / ((int64_t)tiles_x * tiles_y));
    const int x0 = tx * 32, oy = ty * th + r;
    if (oy < H) {
      const uint8_t* row = mask + ((int64_t)b * H + oy) * W + x0;
      if ((W & 15) == 0 && x0 + 32 <= W) {  // two aligned 16-byte loads per row
        const uint4 a = reinterpret_cast<const uint4*>(row)[0], c = reinterpret_cast<const uint4*>(row)[1];
        acc |= a.x | a.y | a.z | a.w | c.x | c.y | c.z | c.w;
      } else {
        for (int k = 0; k < 32 && x0 + k < W; k++) acc |= row[k];
      }
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (ds.p[k] != nullptr) acc |= ds.p[k][((int64_t)b * H + oy) * tiles_x + tx];
    }
  }
  // OR over the 16 lanes of the tile (xor butterfly inside aligned groups of 16)
  acc |= (uint32_t)__shfl_xor((int)acc, 1);
  acc |= (uint32_t)__shfl_xor((int)acc, 2);
  acc |= (uint32_t)__shfl_xor((int)acc, 4);
  acc |= (uint32_t)__shfl_xor((int)acc, 8);
  const bool any = acc != 0 && r == 0 && tile < n_tiles;         // one lane per listed tile
  const unsigned long long bal = __ballot(any);
  if (lane == 0) s_wave[wv] = __popcll(bal);
  __syncthreads();
  if (t == 0) {
    const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = tot > 0 ? atomicAdd(count, tot) : 0;
  }
  __syncthreads();
  if (any) {
    int off = s_base + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wv; w++) off += s_wave[w];
    list[off] = (int32_t)tile;
  }
}

template <int COUT>
int launch_lds(const ConvArgs& a) {
  constexpr int TH = LDS_TH;
  const int64_t n_tiles = (int64_t)a.B * ((a.H + TH - 1) / TH) * ((a.W + 31) / 32);
  int64_t nb = n_tiles;
  const int64_t cap = 256 * 2;  // resident workgroups (LDS: 76.5 KiB per workgroup)
  if (nb > cap) nb = cap;
  const int slot = a.mask != nullptr ? next_sched_slot() : -1;
  if constexpr (COUT == 64) {
    if (a.res != nullptr) {
      k_conv3x3_lds<COUT, true><<<(unsigned)nb, 256, 0, a.st>>>(a.x, a.wfrag, a.bias, a.res, a.mask, a.y, a.B, a.H, a.W, a.relu, a.row_dirty, slot, a.tlist,
                                                               a.tcount);
      PNX_LAUNCH_CHECK();
      return PNX_OK;
    }
  } else {
    PNX_REQUIRE(a.res == nullptr, PNX_ERR_UNSUPPORTED, "residual with %d output channels", COUT);
  }
  k_conv3x3_lds<COUT, false><<<(unsigned)nb, 256, 0, a.st>>>(a.x, a.wfrag, a.bias, nullptr, a.mask, a.y, a.B, a.H, a.W, a.relu, a.row_dirty, slot, a.tlist,
                                                            a.tcount);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

#include "conv_pc.h"

template <int CIN, int COUT, int STRIDE>
int launch(const ConvArgs& a, int Ho, int Wo) {
  constexpr size_t wbytes = (size_t)9 * (CIN / 16) * (COUT / 32) * 64 * 16;
  constexpr bool W_LDS = wbytes <= 76 * 1024;
  constexpr int NT = (COUT / 32 <= 2) ? 4 : 2;
  const int64_t n_tiles = (int64_t)a.B * ((Ho + NT - 1) / NT) * ((Wo + 31) / 32);
  int64_t nb = (n_tiles + 3) / 4;
  if (nb > 512) nb = 512;  // persistent: 2 workgroups per CU
  constexpr auto kern = k_conv3x3<CIN, COUT, STRIDE, W_LDS>;
  if (W_LDS) {
    if (const int rc = pnx_lds_optin<kern>(wbytes); rc != PNX_OK) return rc;
  }
  kern<<<(unsigned)nb, 256, W_LDS ? wbytes : 0, a.st>>>(a.x, a.wfrag, a.bias, a.res, a.mask, a.y, a.B, a.H, a.W, Ho, Wo, a.relu, a.row_dirty);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

}  // namespace

extern "C" {

#if defined(PNX_CONV_TIMERS) && !defined(PNX_CONV_F16)
int pnx_debug_conv_timers(unsigned long long* out) {  // sums over waves of s_memtime ticks per section; resets the counters
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  PNX_CHECK_HIP(hipDeviceSynchronize());
  PNX_CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_conv_T), sizeof(z)));
  PNX_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_conv_T), z, sizeof(z)));
  return PNX_OK;
}
#endif

int PNX_CONV_FN(pnx_sephead_out)(const void* x, const void* wfrag, const float* bias, void* y, int32_t batch, int32_t h, int32_t w, int32_t n_branch,
                         pnx_stream_t stream) {
  PNX_REQUIRE(x && wfrag && bias && y && batch > 0 && h > 0 && w > 0, PNX_ERR_INVALID, "bad arguments");
  PNX_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)wfrag | (uintptr_t)bias) & 15) == 0, PNX_ERR_INVALID, "16-byte alignment required");
  hipStream_t st = (hipStream_t)stream;
  switch (n_branch) {
    case 1: return launch_sephead<1>(x, wfrag, bias, y, batch, h, w, st);  // lazy head: the class branch alone ...
    case 2: return launch_sephead<2>(x, wfrag, bias, y, batch, h, w, st);  // ... or iou + class
    case 5: return launch_sephead<5>(x, wfrag, bias, y, batch, h, w, st);
    case 6: return launch_sephead<6>(x, wfrag, bias, y, batch, h, w, st);
    case 7: return launch_sephead<7>(x, wfrag, bias, y, batch, h, w, st);
    default: break;
  }
  pnx_set_error("pnx_sephead_out: no kernel for %d branches", n_branch);
  return PNX_ERR_UNSUPPORTED;
}

int PNX_CONV_FN(pnx_deconv2x2)(const void* x, const void* wfrag, const float* bias, void* y, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                       int32_t relu, pnx_stream_t stream) {
  PNX_REQUIRE(x && wfrag && bias && y && batch > 0 && h > 0 && w > 0, PNX_ERR_INVALID, "bad arguments");
  PNX_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)wfrag | (uintptr_t)bias) & 15) == 0, PNX_ERR_INVALID, "16-byte alignment required");
  if (cin != 64 || cout != 64) {
    pnx_set_error("pnx_deconv2x2: no kernel for %d -> %d channels", cin, cout);
    return PNX_ERR_UNSUPPORTED;
  }
  const int64_t n_seg = (int64_t)batch * h * ((w + 31) / 32);
  int64_t nb = (n_seg + 3) / 4;
  if (nb > 512) nb = 512;  // persistent: the weights are loaded once per wave
  k_deconv2x2_64<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>((const uint16_t*)x, (const uint4*)wfrag, bias, (uint16_t*)y, batch, h, w, relu);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

#ifndef PNX_CONV_F16  // type-independent helpers: in the bf16 object only
size_t pnx_conv3x3_row_dirty_bytes(int32_t batch, int32_t ho, int32_t wo) {
  if (batch <= 0 || ho <= 0 || wo <= 0) return 0;
  return row_dirty_carve(nullptr, (int64_t)batch * ho * ((wo + 31) / 32)).bytes;
}

int pnx_conv3x3_tile_rows(int32_t cin, int32_t cout, int32_t stride) {
  if (stride != 1) return 0;
  if (cin == 64 && (cout == 64 || cout == 320 || cout == 384 || cout == 448)) return LDS_TH;
  if ((cin == 128 && cout == 128) || (cin == 256 && (cout == 256 || cout == 64))) return L128_TH;
  return 0;
}

static int conv_tile_list_impl(const uint8_t* mask, const uint8_t* const* row_dirty, int32_t n_dirty, int32_t batch, int32_t h, int32_t w, int32_t tile_rows,
                               int32_t* tile_list, int32_t* tile_count, pnx_stream_t stream, bool zero_count) {
  PNX_REQUIRE(mask && tile_list && tile_count && batch > 0 && h > 0 && w > 0 && tile_rows > 0, PNX_ERR_INVALID, "bad arguments");
  PNX_REQUIRE(n_dirty >= 0 && n_dirty <= 4 && (n_dirty == 0 || row_dirty != nullptr), PNX_ERR_INVALID, "0..4 row_dirty arrays");
  DirtySet ds;
  for (int k = 0; k < 4; k++) ds.p[k] = k < n_dirty ? row_dirty[k] : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (zero_count) PNX_CHECK_HIP(hipMemsetAsync(tile_count, 0, sizeof(int32_t), st));
  const int64_t n_tiles = (int64_t)batch * ((h + tile_rows - 1) / tile_rows) * ((w + 31) / 32);
  PNX_REQUIRE(tile_rows <= 16, PNX_ERR_UNSUPPORTED, "tile_rows %d (at most 16: one lane per row)", tile_rows);
  k_tile_list<<<(unsigned)((n_tiles + 15) / 16), 256, 0, st>>>(mask, ds, batch, h, w, tile_rows, tile_list, tile_count);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}
int pnx_conv_tile_list(const uint8_t* mask, const uint8_t* const* row_dirty, int32_t n_dirty, int32_t batch, int32_t h, int32_t w, int32_t tile_rows,
                       int32_t* tile_list, int32_t* tile_count, pnx_stream_t stream) {
  return conv_tile_list_impl(mask, row_dirty, n_dirty, batch, h, w, tile_rows, tile_list, tile_count, stream, true);
}
// internal (enqueue.hip): *tile_count is already zero -- pnx_enqueue clears the counters of all tile-list entries of a table in one launch
int pnx_conv_tile_list_prezeroed(const uint8_t* mask, const uint8_t* const* row_dirty, int32_t n_dirty, int32_t batch, int32_t h, int32_t w, int32_t tile_rows,
                                 int32_t* tile_list, int32_t* tile_count, pnx_stream_t stream) {
  return conv_tile_list_impl(mask, row_dirty, n_dirty, batch, h, w, tile_rows, tile_list, tile_count, stream, false);
}

#endif

int PNX_CONV_FN(pnx_conv3x3)(const void* x, const void* wfrag, const float* bias, const void* residual, const uint8_t* mask, void* y, int32_t batch,
                     int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride, int32_t relu, uint8_t* row_dirty, const int32_t* tile_list,
                     const int32_t* tile_count, pnx_stream_t stream) {
  PNX_REQUIRE((tile_list == nullptr) == (tile_count == nullptr), PNX_ERR_INVALID, "tile_list and tile_count come together");
  PNX_REQUIRE(tile_list == nullptr || (mask != nullptr && pnx_conv3x3_tile_rows(cin, cout, stride) > 0), PNX_ERR_INVALID,
              "a tile list needs a mask and a kernel that takes one (pnx_conv3x3_tile_rows)");
  PNX_REQUIRE(x && wfrag && bias && y && batch > 0 && h > 0 && w > 0, PNX_ERR_INVALID, "bad arguments");
  PNX_REQUIRE(stride == 1 || stride == 2, PNX_ERR_UNSUPPORTED, "stride %d", stride);
  PNX_REQUIRE(row_dirty == nullptr || mask != nullptr, PNX_ERR_INVALID, "row_dirty needs an active-site mask");
  PNX_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)wfrag | (uintptr_t)bias | (uintptr_t)residual) & 15) == 0, PNX_ERR_INVALID,
              "16-byte alignment required");
  const int ho = (h + 2 - 3) / stride + 1, wo = (w + 2 - 3) / stride + 1;
  hipStream_t st = (hipStream_t)stream;
  // PNX_CONV_STALE: 1 (default) zero only the pixels that went stale since the buffer's last launch (the written masks behind the flags); 0: every inactive
  // pixel of a flagged segment, as before the masks (the cross-check)
  static const int stale_mode = getenv("PNX_CONV_STALE") != nullptr ? atoi(getenv("PNX_CONV_STALE")) : 1;
  RowDirty rd = {nullptr, nullptr, stale_mode != 0 ? 1 : 0};
  if (row_dirty != nullptr) {
    PNX_REQUIRE(((uintptr_t)row_dirty & 255) == 0, PNX_ERR_INVALID, "row_dirty must be 256-byte aligned (pnx_conv3x3_row_dirty_bytes: flags, then written masks)");
    const RowDirtyWs rw = row_dirty_carve(row_dirty, (int64_t)batch * ho * ((wo + 31) / 32));
    rd.flag = rw.flag, rd.written = rw.written;
  }
  const ConvArgs a = {(const uint16_t*)x, (const uint4*)wfrag, bias, (const uint16_t*)residual, mask, (uint16_t*)y, batch, h, w, relu, rd, tile_list,
                      tile_count, st};
  if (stride == 1 && getenv("PNX_CONV_DIRECT") == nullptr) {
    static const int pc_mode = getenv("PNX_CONV_PC") != nullptr ? atoi(getenv("PNX_CONV_PC")) : 1;  // bit 0: 64 -> 64 on the producer / consumer kernel (default), bit 1: 128 -> 128 and 256 -> 256, bit 2: 64 -> 320 / 384 / 448; 0: row-split kernels only (the cross-check)
    // PNX_CONV_PACK: the packed-pixel forms, used whenever a mask is given.  Bit 0: 128 -> 128 and 256 -> 256 (k_conv3x3_ldsx<..., PACK>), bit 1: 64 -> 64
    // (k_conv3x3_pc<64, 64, ..., PACK>); unset: both; 0: the row forms everywhere (the cross-check)
    static const int pack_mode = getenv("PNX_CONV_PACK") != nullptr ? atoi(getenv("PNX_CONV_PACK")) : 3;
    if (pc_mode != 0) {
      if (cin == 64 && cout == 64) return launch_pc<64, 64>(a, (pack_mode & 2) != 0);
      if (residual == nullptr && (pc_mode & 4)) {  // slower than the multi-pass row-split kernel (profiles/r06_conv_pc_ab.txt): each pass re-reads the B fragments for half the channels
        if (cin == 64 && cout == 320) return launch_pc<64, 320>(a);
        if (cin == 64 && cout == 384) return launch_pc<64, 384>(a);
        if (cin == 64 && cout == 448) return launch_pc<64, 448>(a);
      }
      if (pc_mode & 2) {
        if (cin == 128 && cout == 128) return launch_pc<128, 128>(a);
        if (cin == 256 && cout == 256) return launch_pc<256, 256>(a);
      }
    }
    if (cin == 64 && cout == 64) return launch_lds<64>(a);
    const bool pack = (pack_mode & 1) != 0;
    if (cin == 128 && cout == 128) return launch_ldsx<128, 128>(a, pack);
    if (cin == 256 && cout == 64) return launch_ldsx<256, 64>(a);
    if (cin == 256 && cout == 256) return launch_ldsx<256, 256>(a, pack);
    if (cin == 64 && cout == 384) return launch_lds<384>(a);
    if (cin == 64 && cout == 320) return launch_lds<320>(a);
    if (cin == 64 && cout == 448) return launch_lds<448>(a);
  }
  if (stride == 2 && residual == nullptr && getenv("PNX_CONV_DIRECT") == nullptr) {  // launch_s2 is shared with the fp32 training entries: pieces + plain arguments
    if (cin == 64 && cout == 128) return launch_s2<64, 128, 1>(x, wfrag, bias, mask, y, batch, h, w, ho, wo, relu, rd, st);
    if (cin == 128 && cout == 256) return launch_s2<128, 256, 1>(x, wfrag, bias, mask, y, batch, h, w, ho, wo, relu, rd, st);
    if (cin == 256 && cout == 256) return launch_s2<256, 256, 1>(x, wfrag, bias, mask, y, batch, h, w, ho, wo, relu, rd, st);
  }
#define PNX_CONV_CASE(CI, CO)                             \
  if (cin == CI && cout == CO) {                          \
    if (stride == 1) return launch<CI, CO, 1>(a, ho, wo); \
    return launch<CI, CO, 2>(a, ho, wo);                  \
  }
  PNX_CONV_CASE(64, 64)
  PNX_CONV_CASE(64, 128)
  PNX_CONV_CASE(128, 128)
#undef PNX_CONV_CASE
  pnx_set_error("pnx_conv3x3: no kernel for %d -> %d channels", cin, cout);
  return PNX_ERR_UNSUPPORTED;
}

#ifndef PNX_CONV_F16  // the training-only entries exist once, on the bf16 instructions
}  // extern "C"
namespace {
#include "conv_dgrad_s2.h"

// The stride-2 data gradient and the fp32 forward come with 1, 2 or 3 bf16 pieces per operand (PnxPieces<NP>).  Each family has ONE implementation that holds
// its checks and its shape ladder; the entry points below fill the piece structs and pass their own NP and their name (for the messages).
template <int NP>
int dgrad_s2_impl(const char* name, PnxPieces<NP> g, PnxPieces<NP> wfrag_t, const uint8_t* mask_in, void* dx, int32_t batch, int32_t h, int32_t w, int32_t cin,
                  int32_t cout, pnx_stream_t stream) {
  PNX_REQUIRE(g.complete() && wfrag_t.complete() && mask_in && dx && batch > 0 && h > 0 && w > 0, PNX_ERR_INVALID, "%s: bad arguments", name);
  PNX_REQUIRE(((g.bits() | wfrag_t.bits() | (uintptr_t)dx) & 15) == 0, PNX_ERR_INVALID, "16-byte alignment required");
  hipStream_t st = (hipStream_t)stream;
  if (cin == 64 && cout == 128) return launch_dgrad_s2<128, 64, NP>(g, wfrag_t, mask_in, dx, batch, h, w, st);
  if (cin == 128 && cout == 256) return launch_dgrad_s2<256, 128, NP>(g, wfrag_t, mask_in, dx, batch, h, w, st);
  if (cin == 256 && cout == 256) return launch_dgrad_s2<256, 256, NP>(g, wfrag_t, mask_in, dx, batch, h, w, st);
  pnx_set_error("%s: no kernel for %d -> %d channels", name, cin, cout);
  return PNX_ERR_UNSUPPORTED;
}

template <int NP>
int conv3x3_f32_impl(const char* name, PnxPieces<NP> x, PnxPieces<NP> wfrag, const float* bias, const uint8_t* mask, float* y, int32_t batch, int32_t h, int32_t w,
                     int32_t cin, int32_t cout, int32_t stride, pnx_stream_t stream) {
  PNX_REQUIRE(x.complete() && wfrag.complete() && y, PNX_ERR_INVALID, "null pointer");
  PNX_REQUIRE(batch > 0 && h > 0 && w > 0, PNX_ERR_INVALID, "bad shape");
  PNX_REQUIRE(stride == 1 || stride == 2, PNX_ERR_UNSUPPORTED, "stride %d", stride);
  PNX_REQUIRE(((x.bits() | wfrag.bits() | (uintptr_t)y | (uintptr_t)bias) & 15) == 0, PNX_ERR_INVALID, "16-byte alignment required");
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1) {
    if (cin == 64 && cout == 64) return launch_pc_f32<64, 64, NP>(x, wfrag, bias, mask, y, batch, h, w, st);
    if (cin == 128 && cout == 128) return launch_pc_f32<128, 128, NP>(x, wfrag, bias, mask, y, batch, h, w, st);
    if (cin == 256 && cout == 256) return launch_pc_f32<256, 256, NP>(x, wfrag, bias, mask, y, batch, h, w, st);
  } else {
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    if (cin == 64 && cout == 128) return launch_s2<64, 128, NP>(x, wfrag, bias, mask, y, batch, h, w, ho, wo, 0, RowDirty{nullptr, nullptr, 1}, st);
    if (cin == 128 && cout == 256) return launch_s2<128, 256, NP>(x, wfrag, bias, mask, y, batch, h, w, ho, wo, 0, RowDirty{nullptr, nullptr, 1}, st);
    if (cin == 256 && cout == 256) return launch_s2<256, 256, NP>(x, wfrag, bias, mask, y, batch, h, w, ho, wo, 0, RowDirty{nullptr, nullptr, 1}, st);
  }
  pnx_set_error("%s: no kernel for %d -> %d channels, stride %d", name, cin, cout, stride);
  return PNX_ERR_UNSUPPORTED;
}

}  // namespace
extern "C" {

// Data gradient of a stride-2 SparseConv2d layer (conv_dgrad_s2.h): g (batch, ho, wo, cout) NHWC bf16, wfrag_t = pnx_conv3x3_pack_weights(transposed = 1) of the
// layer's (cout, cin, 3, 3) weights, mask_in = active sites of the layer's INPUT (batch, h, w); dx (batch, h, w, cin) bf16, zeros at inactive sites, every site written.
int pnx_conv3x3_dgrad_s2_bf16(const void* g, const void* wfrag_t, const uint8_t* mask_in, void* dx, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout,
                              pnx_stream_t stream) {
  return dgrad_s2_impl<1>("pnx_conv3x3_dgrad_s2_bf16", {g}, {wfrag_t}, mask_in, dx, batch, h, w, cin, cout, stream);
}

// The same from the bf16 halves of an fp32 gradient and of the fp32 weights (pnx_split_f32), fp32 out: the stride-2 companion of pnx_conv3x3_x3.
int pnx_conv3x3_dgrad_s2_x3(const void* g_hi, const void* g_lo, const void* wfrag_t_hi, const void* wfrag_t_lo, const uint8_t* mask_in, float* dx, int32_t batch,
                            int32_t h, int32_t w, int32_t cin, int32_t cout, pnx_stream_t stream) {
  return dgrad_s2_impl<2>("pnx_conv3x3_dgrad_s2_x3", {g_hi, g_lo}, {wfrag_t_hi, wfrag_t_lo}, mask_in, dx, batch, h, w, cin, cout, stream);
}

// Three bf16 pieces of g and of the weights (pnx_split3_f32), six products, fp32 out: the stride-2 companion of pnx_conv3x3_x6.
int pnx_conv3x3_dgrad_s2_x6(const void* g_hi, const void* g_mid, const void* g_lo, const void* wfrag_t_hi, const void* wfrag_t_mid, const void* wfrag_t_lo,
                            const uint8_t* mask_in, float* dx, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, pnx_stream_t stream) {
  return dgrad_s2_impl<3>("pnx_conv3x3_dgrad_s2_x6", {g_hi, g_mid, g_lo}, {wfrag_t_hi, wfrag_t_mid, wfrag_t_lo}, mask_in, dx, batch, h, w, cin, cout, stream);
}

// fp32 convolution out of three bf16 products: x = x_hi + x_lo and W = W_hi + W_lo (bf16 halves of fp32 values, pnx_split_f32; both weight halves in
// pnx_conv3x3_pack_weights order), y = x_hi W_hi + x_hi W_lo + x_lo W_hi accumulated in fp32 inside ONE launch (the low x low term is below the
// halves' own rounding, 2^-17 relative) and written as fp32 NHWC; zeros at inactive sites, every site written.  bias (fp32, may be null) starts the
// accumulators; no activation: this is the convolution of the fp32 training graph (forward, and the stride-1 data gradient with transposed weights).
int pnx_conv3x3_x3(const void* x_hi, const void* x_lo, const void* wfrag_hi, const void* wfrag_lo, const float* bias, const uint8_t* mask, float* y,
                   int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride, pnx_stream_t stream) {
  return conv3x3_f32_impl<2>("pnx_conv3x3_x3", {x_hi, x_lo}, {wfrag_hi, wfrag_lo}, bias, mask, y, batch, h, w, cin, cout, stride, stream);
}

// fp32 convolution out of six bf16 products: x = x_hi + x_mid + x_lo and W = W_hi + W_mid + W_lo (pnx_split3_f32, exact for |x| >= 2^-100), y = the
// products of piece orders 0..2 (hi.hi, hi.mid, mid.hi, mid.mid, hi.lo, lo.hi; the dropped mid.lo, lo.mid, lo.lo are ~2^-23 of sum |x||W|, fp32's own
// rounding) accumulated in fp32 inside ONE launch, low-order products first and hi.hi last.  Otherwise exactly pnx_conv3x3_x3: shapes, mask, bias, output.
int pnx_conv3x3_x6(const void* x_hi, const void* x_mid, const void* x_lo, const void* wfrag_hi, const void* wfrag_mid, const void* wfrag_lo, const float* bias,
                   const uint8_t* mask, float* y, int32_t batch, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t stride, pnx_stream_t stream) {
  return conv3x3_f32_impl<3>("pnx_conv3x3_x6", {x_hi, x_mid, x_lo}, {wfrag_hi, wfrag_mid, wfrag_lo}, bias, mask, y, batch, h, w, cin, cout, stride, stream);
}
#endif

}  // extern "C"

// ---- the lazy SepHead (sephead_lazy.h): sizes shared by the kernel and its entry point
namespace {

constexpr int kLzG = 32, kLzN = kLzG * 9, kLzNT = kLzN / 32;  // candidates, pixels, N tiles per workgroup
constexpr int kLzPatch = kLzG * 25 * 8;                       // uint4 slots of the staged patches
constexpr int kLzW2 = 10 * 9 * 32 * 3;                        // floats of the packed second-convolution weights
constexpr int kLzMaxTasks = 8, kLzMaxClasses = 32;
constexpr int kLzAhead = 2;  // taps of weight-fragment lookahead

#include "sephead_lazy.h"

}  // namespace

extern "C" int PNX_CONV_FN(pnx_sephead_lazy)(const PnxLazyTask* tasks, int32_t n_tasks, const int32_t* class_task, int32_t nc_total, int32_t batch,
                                     const int64_t* local, const int32_t* seg_len, int32_t pre_max, float* out, pnx_stream_t stream) {
  PNX_REQUIRE(tasks && class_task && local && seg_len && out && batch > 0 && pre_max > 0, PNX_ERR_INVALID, "bad arguments");
  PNX_REQUIRE(n_tasks >= 1 && n_tasks <= kLzMaxTasks && nc_total >= 1 && nc_total <= kLzMaxClasses, PNX_ERR_UNSUPPORTED, "at most 8 tasks / 32 classes");
  LazyArgs a;
  for (int i = 0; i < n_tasks; i++) {
    const PnxLazyTask& s = tasks[i];
    PNX_REQUIRE(s.up && s.wfrag1 && s.bias1 && s.w2c && s.bias2 && s.h > 0 && s.w > 0, PNX_ERR_INVALID, "bad task");
    PNX_REQUIRE((int64_t)batch * s.h * s.w < ((int64_t)1 << 31), PNX_ERR_UNSUPPORTED, "map too large for 32-bit cell indices");
    PNX_REQUIRE((((uintptr_t)s.up | (uintptr_t)s.wfrag1 | (uintptr_t)s.w2c) & 15) == 0, PNX_ERR_INVALID, "16-byte alignment required");
    a.t[i] = LazyTaskDev{(const uint16_t*)s.up, (const uint4*)s.wfrag1, s.bias1, s.w2c, s.bias2, s.h, s.w};
  }
  for (int c = 0; c < nc_total; c++) {
    PNX_REQUIRE(class_task[c] >= 0 && class_task[c] < n_tasks, PNX_ERR_INVALID, "class_task out of range");
    a.class_task[c] = (signed char)class_task[c];
  }
  a.nc_total = nc_total, a.pre_max = pre_max, a.bps = (pre_max + kLzG - 1) / kLzG;
  if (const int rc = pnx_lds_optin<&k_sephead_lazy>(kLzLds); rc != PNX_OK) return rc;
  const unsigned nb = (unsigned)((int64_t)batch * nc_total * a.bps);
  k_sephead_lazy<<<nb, 512, kLzLds, (hipStream_t)stream>>>(a, local, seg_len, out);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}
