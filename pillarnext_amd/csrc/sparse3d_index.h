// sparse3d_index.h -- the index of an active set (sparse3d.hip's header comment): key-order occupancy bitmap + popcount word prefix over
// (batch, D, H, W).  Included inside the anonymous namespace of every file that reads one: sparse3d.hip builds it, group.hip looks the
// corners of a sample up in it (pnx_sp3_bilinear_gather).  A site's key is ((b*D + z)*H + y)*W + x, its rank the number of set bits below it.
#pragma once

struct Sp3Grid {
  int B, D, H, W;
};

struct Sp3Index {
  uint32_t* bitmap;
  uint32_t* pre;
  uint32_t* blk;
  int64_t nwords;
  int nblk;
  size_t bytes;
};

Sp3Index sp3_carve(void* base, const Sp3Grid& g) {
  Sp3Index r;
  const int64_t cells = (int64_t)g.B * g.D * g.H * g.W;
  r.nwords = (cells + 31) >> 5;
  r.nblk = (int)((r.nwords + PNX_SCAN_ITEMS - 1) / PNX_SCAN_ITEMS);
  PnxCarver c(base);
  r.bitmap = c.take<uint32_t>((size_t)r.nwords);
  r.pre = c.take<uint32_t>((size_t)r.nwords);
  r.blk = c.take<uint32_t>((size_t)r.nblk + 1);
  r.bytes = c.used();
  return r;
}

int sp3_grid(int32_t batch, const int32_t* grid3, Sp3Grid* g) {
  PNX_REQUIRE(grid3 != nullptr, PNX_ERR_INVALID, "sparse3d: grid is NULL");
  PNX_REQUIRE(batch >= 0 && grid3[0] >= 1 && grid3[1] >= 1 && grid3[2] >= 1, PNX_ERR_INVALID, "sparse3d: bad grid %d x (%d, %d, %d)", batch,
              grid3[0], grid3[1], grid3[2]);
  const int64_t cells = (int64_t)batch * grid3[0] * grid3[1] * grid3[2];
  PNX_REQUIRE(cells < ((int64_t)1 << 36), PNX_ERR_UNSUPPORTED, "sparse3d: %lld grid cells (at most 2^36)", (long long)cells);
  g->B = batch, g->D = grid3[0], g->H = grid3[1], g->W = grid3[2];
  return PNX_OK;
}

int sp3_index_args(const Sp3Grid& g, void* index, size_t index_bytes, Sp3Index* ix) {
  *ix = sp3_carve(index, g);
  return pnx_check_workspace(index, index_bytes, ix->bytes, "sparse3d index");
}

__device__ __forceinline__ int64_t sp3_key(const Sp3Grid& g, int b, int z, int y, int x) { return (((int64_t)b * g.D + z) * g.H + y) * g.W + x; }

__device__ __forceinline__ uint32_t sp3_rank(const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk,
                                             int64_t k) {
  const int64_t w = k >> 5;
  return blk[w >> PNX_SCAN_SHIFT] + pre[w] + (uint32_t)__popc(bitmap[w] & ((1u << (k & 31)) - 1u));
}
