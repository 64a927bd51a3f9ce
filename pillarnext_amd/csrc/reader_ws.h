// reader_ws.h -- host side shared by the reader's translation units (reader.hip, chunk_sort.hip, pfn_spans.hip, pfn_v3.hip, pfn_train.hip):
// the carved workspace, the launchers that cross files, the environment switches, the feature-count and canvas-dtype dispatchers.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "pnx_common.h"
#include "spans.h"

struct PnxFillJob;  // pnx_fill.h

struct ReaderWs {
  int32_t* counters;  // [0]=P [1]=N'
  int32_t* tick;      // 16 ticket words in separate lines (pfn_v3.hip), zeroed with the counters
  uint32_t *bitmap, *wpre, *wblk;
  uint8_t* bytemap;
  int32_t* owner;
  uint32_t* rec;
  int32_t* biglist;  // pillars with more than 32 points (handled by k_pfn_big)
  int32_t* cell;     // canvas cell of every pillar
  int64_t bigcap;
  size_t zero_bytes, zero_bytes2;  // counters | tick | bytemap [| count] are contiguous: one memset per call
  int32_t *key, *rank, *slot;
  uint32_t *count, *cpre, *cblk;
  int32_t* plist;
  uint32_t *kpre, *kblk;
  float* mean;
  float* g1;
  int64_t nwords, pcap;
  int nblk_w, nblk_c, nblk_k;
  // binned path (reader_bins.h): bins of 2^sh pillars, K1 bins, points handled in `nwg` chunks of `chunk`
  int sh, K1, chunk, nwg, nblk_m;
  int gthreads;  // threads per workgroup of k_bin_count / k_bin_scatter
  int64_t matlen;
  uint32_t *histmat, *hpre, *hblk;
  uint32_t* rec64;               // pillar-sorted decorated records, 64 B per kept point
  uint32_t *pfirst, *pcnt;       // first sorted slot / number of points of every pillar
  uint2* wcomb;                  // {bitmap word, popcount prefix} pairs
  // span path (chunk_sort.hip + pfn_spans.hip, PNX_READER_IMPL=4, default)
  SpanGeom sg;
  uint4* srecs;                  // chunk-sorted 32-byte records
  uint16_t* stab;                // run table
  int32_t* srowframe;
  uint32_t* srowbase;
  int32_t *frame_lo, *frame_hi;
  uint32_t* slab_tot;
  uint2* span_desc;
  int32_t* nspan;
  int32_t* row_of;               // feat_max row per spill id
  uint8_t* cbytes;               // occupancy bytes in canvas order (when the caller passes no occupancy output)
  size_t zero_bytes_span;        // counters | tick | frame_lo | frame_hi
  size_t bytes;
};

// reader.hip
int64_t cells_padded(const pnx_geom* g, int32_t batch);
ReaderWs carve(void* ws, int64_t n, int32_t batch, const pnx_geom* g);  // ws == nullptr: sizes only (w.bytes)
PnxGeomDev make_geom(const pnx_geom* g, int32_t batch);

// pfn_v3.hip: PFN over the pillar-sorted records of the binned path (w.rec64 / w.pfirst / w.pcnt / w.cell).  n_fill > 0: blocks
// [0, n_fill) of the launch take the zero-fill tiles of `fj` (pnx_fill.h) concurrently with the PFN.
int pnx_launch_pfn_v3(const ReaderWs& w, int F, const float* folded, float* g1, int64_t g1_rows, void* canvas, int canvas_dt, int64_t n_points,
                      int n_fill, const PnxGeomDev& geom, const PnxFillJob& fj, hipStream_t st);
// pfn_v3.hip: the one-wave-per-pillar kernel alone, for what the span kernel spills.  ranked: g1 rows come from w.row_of.
int pnx_launch_pfn3_tail(const ReaderWs& w, int F, bool ranked, const float* folded, float* g1, int64_t g1_rows, void* canvas, int canvas_dt,
                         int blocks, hipStream_t st);

// pfn_train.hip.  pass: 0 gram0, 1 gram1, 2 output, 3 backward-1, 4 backward-0
int pnx_launch_pfn_train(const ReaderWs& w, int F, int pass, const float* prm, float* part, const float* G, const float* out_saved, float* out,
                         int64_t out_rows, hipStream_t st);
int pnx_pfn_train_blocks(void);

// chunk_sort.hip / pfn_spans.hip: the one-pass grouping front end and its consumer (spans.h)
size_t pnx_chunk_sort_lds(const SpanGeom& sg);
int pnx_launch_chunk_sort(const ReaderWs& w, const float* points, int64_t n, int stride, const PnxGeomDev& g, uint8_t* bytemap, hipStream_t st,
                          hipEvent_t sorted);
int pnx_launch_span_pfn(const ReaderWs& w, int F, bool ranked, int32_t* coords, int64_t pillar_capacity, const float* folded, float* g1,
                        int64_t g1_rows, void* canvas, int canvas_dt, int canvas_nt, int64_t n_points, const PnxGeomDev& geom, hipStream_t st);

// ---- switches, read from the environment on EVERY call (tests and experiments change them between calls)
inline int pnx_env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline int pnx_fill_blocks() { return pnx_env_int("PNX_FILL_BLOCKS", 256); }  // zero-fill workgroups: one per CU (0: timing experiments, the canvas is wrong)
inline int pnx_pfn_blocks() { return pnx_env_int("PNX_PFN_BLOCKS", 512); }    // persistent PFN workgroups: 256 CUs x 2 workgroups x 4 waves = 2 waves per SIMD
// nontemporal zero-fill: from 1.5 GiB on, far beyond what the Infinity Cache absorbs
inline bool pnx_fill_nt(size_t canvas_bytes) {
  const char* e = getenv("PNX_FILL_NT");
  return e ? e[0] == '1' : canvas_bytes >= ((size_t)3 << 29);
}
// layer 1 of the PFN on fp16 hi/lo pairs (0: plain fp32 MFMA, which only the binned pipeline has)
inline bool pnx_pfn_f16x3() {
  const char* e = getenv("PNX_PFN_F16X3");
  return !(e && e[0] == '0');
}

// ---- run-time value -> template argument: `f` is a generic lambda that receives the value as a std::integral_constant.
// Point features 3..FMAX:
template <int FMAX = 6, typename Fn>
int pnx_with_features(int F, Fn&& f) {
  switch (F) {
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6:
      if constexpr (FMAX >= 6) return f(std::integral_constant<int, 6>{});
  }
  pnx_set_error("num_point_features %d not in 3..%d", F, FMAX);
  return PNX_ERR_UNSUPPORTED;
}
// Canvas dtype (validated by the entry points: anything that is not PNX_F32 or PNX_BF16 is PNX_F16).
template <typename Fn>
auto pnx_with_dtype(int dt, Fn&& f) {
  if (dt == PNX_F32) return f(std::integral_constant<int, PNX_F32>{});
  if (dt == PNX_BF16) return f(std::integral_constant<int, PNX_BF16>{});
  return f(std::integral_constant<int, PNX_F16>{});
}
// Canvas dtype and the packed LDS output rows of the PFN kernels, which exist for the 16-bit dtypes only.
template <typename Fn>
auto pnx_with_dtype_pack(int dt, bool pack, Fn&& f) {
  return pnx_with_dtype(dt, [&](auto d) {
    if constexpr (d() != PNX_F32) {
      if (pack) return f(d, std::true_type{});
    }
    return f(d, std::false_type{});
  });
}
