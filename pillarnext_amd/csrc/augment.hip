// augment.hip -- GT-database paste and the four global augmentations on the device, for gfx950.
//
// Reference: det3d/datasets/base.py:72-99, i.e. DataBaseSamplerV2.sample_all / sample_class_v2 (sample_ops.py:112-235) with box_collision_test and
// points_in_boxes_jit (box_np_ops.py:190-302), then Rotation, Scaling, Translation, Flip (pipelines/augmentation.py with box_np_ops.py:5-46): numpy
// and a numba N x M loop per frame on the host.  Here the candidates the host sampler picked and the parameters it drew arrive as small device
// arrays, and everything that touches a box or a point is done in a handful of launches on one stream:
//   k_paste_select   one workgroup per frame.  BEV corners in fp64 from the fp32 boxes; one bit per (candidate, box) pair of the directed
//                    collision test, 32 pairs per work item so that every word of the bit matrix has one writer; the greedy pass in group
//                    order by one wave, lane w holding word w of the live set (one LDS read and one ballot per candidate); then the merged [gt, accepted] boxes and classes, the acceptance
//                    flags and each accepted object's first row inside the frame's pasted rows.
//   k_paste_head     the pasted-row counts of the frames go in front of the frames' chunk counts.
//   k_paste_flags    one workgroup per chunk of kChunk scene rows: the frames present in the chunk are walked, the frame's accepted boxes sit
//                    in LDS as (centre, half sizes, cos, sin, bounding radius^2), a row is tested in fp64 after a cheap fp32 radius reject.
//                    Leaves one keep bit per row and one count per (frame, chunk).
//   k_scan_local / k_scan_blocks (pnx_scan.h) over [frame 0: pasted, chunk 0, chunk 1, ..; frame 1: ..]: the exclusive prefix of an entry is the
//                    output row where that piece starts, the total is n_out.
//   k_paste_write    survivors: stable rank inside (chunk, frame) by ballots, transformed, written once.
//   k_paste_objects  one workgroup per accepted candidate: bank rows + fp32 centre, transformed, written once.
//   k_paste_frame_rows / k_paste_tail   the per-frame row counts; rows [n_out, capacity): batch index -1.
//   k_augment_boxes  the box side of the transforms, one thread per box.
// The scene rows are read twice (xyz and the batch index for the flags, the whole row for the write) and written once; the flags are one bit per row.
// There is no atomic anywhere: every output element has one writer and no result depends on an order of execution.
#include <math.h>

#include "pnx_common.h"
#include "pnx_scan.h"

namespace {

constexpr int kPB = 256;                  // threads of every kernel here
constexpr int kChunkIters = 8;
constexpr int kChunk = kPB * kChunkIters;  // scene rows per workgroup of the point pass
constexpr int kMaxBoxes = PNX_PASTE_MAX_BOXES;
constexpr int kWordsMax = kMaxBoxes / 32;
constexpr int kMaxB = PNX_PASTE_MAX_BATCH;
constexpr int kMaxGroups = 64;
constexpr float kPiF = 3.14159274101257324219f;      // fp32(pi)
constexpr float kTwoPiF = 6.28318548202514648438f;   // fp32(2 pi)

struct Xform {
  double c, s, t;
  float a, scale;
  int flags;
};

__device__ __forceinline__ Xform load_xform(const double* __restrict__ xf, int b) {
  Xform f;
  f.c = 1.0, f.s = 0.0, f.t = 0.0, f.a = 0.f, f.scale = 1.f, f.flags = 0;
  if (xf != nullptr) {
    const double* p = xf + (int64_t)b * 6;
    f.c = p[0], f.s = p[1], f.a = (float)p[2], f.scale = (float)p[3], f.t = p[4], f.flags = (int)p[5];
  }
  return f;
}

// x' = fp32(x c - y s), y' = fp32(x s + y c): two products and one sum each, all fp64, rounded once (numpy: fp32 row times an fp64 matrix)
__device__ __forceinline__ void rot2(const Xform& f, float& x, float& y) {
  const double xd = x, yd = y;
  const float nx = (float)__dadd_rn(__dmul_rn(xd, f.c), -__dmul_rn(yd, f.s));
  const float ny = (float)__dadd_rn(__dmul_rn(xd, f.s), __dmul_rn(yd, f.c));
  x = nx, y = ny;
}

__device__ __forceinline__ void xform_point(const Xform& f, float& x, float& y, float& z) {
  if (f.flags & PNX_AUG_ROTATE) rot2(f, x, y);
  if (f.flags & PNX_AUG_SCALE) x = __fmul_rn(x, f.scale), y = __fmul_rn(y, f.scale), z = __fmul_rn(z, f.scale);
  if (f.flags & PNX_AUG_TRANSLATE) x = (float)__dadd_rn((double)x, f.t), y = (float)__dadd_rn((double)y, f.t), z = (float)__dadd_rn((double)z, f.t);
  if (f.flags & PNX_AUG_FLIP_X) y = -y;
  if (f.flags & PNX_AUG_FLIP_Y) x = -x;
}

// v: x y z dx dy dz vx vy yaw (vx, vy unused when !vel).  Every stage: NaN elements enter as 0 and are NaN again afterwards.
struct NanMask {
  unsigned m;
  __device__ __forceinline__ void enter(float* v) {
    m = 0;
#pragma unroll
    for (int j = 0; j < 9; j++)
      if (isnan(v[j])) m |= 1u << j, v[j] = 0.f;
  }
  __device__ __forceinline__ void leave(float* v) const {
#pragma unroll
    for (int j = 0; j < 9; j++)
      if (m >> j & 1u) v[j] = __builtin_nanf("");
  }
};

__device__ __forceinline__ float wrap_yaw(float yaw) {
  if (yaw > kPiF) yaw = yaw - kTwoPiF;
  if (yaw < -kPiF) yaw = yaw + kTwoPiF;
  return yaw;
}

__device__ __forceinline__ void xform_box(const Xform& f, float* v, bool vel) {
  NanMask nm;
  if (f.flags & PNX_AUG_ROTATE) {
    nm.enter(v);
    rot2(f, v[0], v[1]);
    if (vel) rot2(f, v[6], v[7]);
    v[8] = __fadd_rn(v[8], f.a);
    nm.leave(v);
  }
  if (f.flags & PNX_AUG_SCALE) {
    nm.enter(v);
#pragma unroll
    for (int j = 0; j < 6; j++) v[j] = __fmul_rn(v[j], f.scale);
    if (vel) v[6] = __fmul_rn(v[6], f.scale), v[7] = __fmul_rn(v[7], f.scale);
    nm.leave(v);
  }
  if (f.flags & PNX_AUG_TRANSLATE) {
    nm.enter(v);
#pragma unroll
    for (int j = 0; j < 3; j++) v[j] = (float)__dadd_rn((double)v[j], f.t);
    nm.leave(v);
  }
  if (f.flags & PNX_AUG_FLIP_X) {
    nm.enter(v);
    v[1] = -v[1], v[8] = -v[8];
    if (vel) v[7] = -v[7];
    v[8] = wrap_yaw(v[8]);
    nm.leave(v);
  }
  if (f.flags & PNX_AUG_FLIP_Y) {
    nm.enter(v);
    v[0] = -v[0], v[8] = __fadd_rn(-v[8], kPiF);
    if (vel) v[6] = -v[6];
    v[8] = wrap_yaw(v[8]);
    nm.leave(v);
  }
}

// ----------------------------------------------------------------------------------------------------------------------------- selection

// box_np_ops.py:216-302 with `a` as boxes[i] and `q` as qboxes[j]; corners x0 y0 x1 y1 x2 y2 x3 y3, clockwise
__device__ bool collide(const double* a, const double* q) {
  const double aminx = fmin(fmin(a[0], a[2]), fmin(a[4], a[6])), amaxx = fmax(fmax(a[0], a[2]), fmax(a[4], a[6]));
  const double qminx = fmin(fmin(q[0], q[2]), fmin(q[4], q[6])), qmaxx = fmax(fmax(q[0], q[2]), fmax(q[4], q[6]));
  if (!(fmin(amaxx, qmaxx) - fmax(aminx, qminx) > 0.0)) return false;
  const double aminy = fmin(fmin(a[1], a[3]), fmin(a[5], a[7])), amaxy = fmax(fmax(a[1], a[3]), fmax(a[5], a[7]));
  const double qminy = fmin(fmin(q[1], q[3]), fmin(q[5], q[7])), qmaxy = fmax(fmax(q[1], q[3]), fmax(q[5], q[7]));
  if (!(fmin(amaxy, qmaxy) - fmax(aminy, qminy) > 0.0)) return false;
  for (int k = 0; k < 4; k++) {
    const double Ax = a[2 * k], Ay = a[2 * k + 1], Bx = a[2 * ((k + 1) & 3)], By = a[2 * ((k + 1) & 3) + 1];
    for (int l = 0; l < 4; l++) {
      const double Cx = q[2 * l], Cy = q[2 * l + 1], Dx = q[2 * ((l + 1) & 3)], Dy = q[2 * ((l + 1) & 3) + 1];
      const bool acd = (Dy - Ay) * (Cx - Ax) > (Cy - Ay) * (Dx - Ax);
      const bool bcd = (Dy - By) * (Cx - Bx) > (Cy - By) * (Dx - Bx);
      if (acd != bcd) {
        const bool abc = (Cy - Ay) * (Bx - Ax) > (By - Ay) * (Cx - Ax);
        const bool abd = (Dy - Ay) * (Bx - Ax) > (By - Ay) * (Dx - Ax);
        if (abc != abd) return true;
      }
    }
  }
  // no edges cross: every corner of q strictly inside a, or every corner of a strictly inside q
  bool inside = true;
  for (int l = 0; l < 4 && inside; l++)
    for (int k = 0; k < 4; k++) {
      const double vx = -(a[2 * k] - a[2 * ((k + 1) & 3)]), vy = -(a[2 * k + 1] - a[2 * ((k + 1) & 3) + 1]);
      double cross = vy * (a[2 * k] - q[2 * l]);
      cross -= vx * (a[2 * k + 1] - q[2 * l + 1]);
      if (cross >= 0.0) {
        inside = false;
        break;
      }
    }
  if (inside) return true;
  inside = true;
  for (int l = 0; l < 4 && inside; l++)
    for (int k = 0; k < 4; k++) {
      const double vx = -(q[2 * k] - q[2 * ((k + 1) & 3)]), vy = -(q[2 * k + 1] - q[2 * ((k + 1) & 3) + 1]);
      double cross = vy * (q[2 * k] - a[2 * l]);
      cross -= vx * (q[2 * k + 1] - a[2 * l + 1]);
      if (cross >= 0.0) {
        inside = false;
        break;
      }
    }
  return inside;
}

struct SelectArgs {
  const float* gt_boxes;
  const int32_t* gt_cls;
  const int32_t* num_gt;
  const int32_t* cand_bank;
  const float* cand_boxes;
  const int32_t* cand_cls;
  const int32_t* cand_group;
  const int64_t* bank_offsets;
  uint8_t* accept;
  int32_t* paste_offset;
  float* boxes_out;
  int32_t* classes_out;
  int32_t* num_out;
  int32_t* pasted_rows;
  int K, S, D, G, n_obj;
};

// dynamic LDS: corners (K+S) x 8 doubles | bits S x W words | rows, slot, off, group: S ints each | group members G x W words
__host__ __device__ inline size_t select_lds_bytes(int K, int S, int G) {
  const int n = K + S, W = (n + 31) / 32;
  return (size_t)n * 8 * sizeof(double) + (size_t)S * W * 4 + (size_t)S * 4 * 4 + (size_t)G * W * 4;
}

__global__ __launch_bounds__(kPB) void k_paste_select(SelectArgs p) {
  extern __shared__ double s_dyn[];
  __shared__ uint32_t s_valid[kWordsMax], s_live[kWordsMax];
  __shared__ int s_nacc, s_nrows;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = p.K, S = p.S, D = p.D, n = K + S, W = (n + 31) / 32;
  double* corners = s_dyn;
  uint32_t* bits = reinterpret_cast<uint32_t*>(corners + (size_t)n * 8);
  int* s_rows = reinterpret_cast<int*>(bits + (size_t)S * W);
  int* s_slot = s_rows + S;
  int* s_off = s_slot + S;
  int* s_group = s_off + S;
  uint32_t* gbits = reinterpret_cast<uint32_t*>(s_group + S);
  int ng = K;
  if (p.num_gt != nullptr) ng = min(max(p.num_gt[b], 0), K);
  // corners and validity: one writer per word of s_valid (32 boxes per thread)
  for (int j = tid; j < n; j += kPB) {
    const float* bx = j < K ? p.gt_boxes + ((int64_t)b * K + j) * D : p.cand_boxes + ((int64_t)b * S + (j - K)) * D;
    bool ok = j < ng;
    if (j >= K) {
      const int i = j - K;
      const int id = p.cand_bank[(int64_t)b * S + i];
      ok = id >= 0 && id < p.n_obj;
      int64_t rows = 0;
      if (ok) rows = p.bank_offsets[id + 1] - p.bank_offsets[id];
      s_rows[i] = (int)min(max(rows, (int64_t)0), (int64_t)INT32_MAX);
      s_slot[i] = -1, s_off[i] = -1;
      s_group[i] = ok ? p.cand_group[(int64_t)b * S + i] : -1;
    }
    double* c = corners + (size_t)j * 8;
    if (ok) {
      const double cx = bx[0], cy = bx[1], hx = (double)bx[3] * 0.5, hy = (double)bx[4] * 0.5;
      const double cs = cos((double)bx[D - 1]), sn = sin((double)bx[D - 1]);
      const double lx[4] = {-hx, -hx, hx, hx}, ly[4] = {-hy, hy, hy, -hy};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        c[2 * k] = (lx[k] * cs - ly[k] * sn) + cx;
        c[2 * k + 1] = (lx[k] * sn + ly[k] * cs) + cy;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) c[k] = 0.0;
    }
  }
  __syncthreads();
  if (tid < kWordsMax) {
    uint32_t v = 0, g = 0;
    for (int k = 0; k < 32; k++) {
      const int j = tid * 32 + k;
      if (j >= n) break;
      const bool ok = j < K ? j < ng : s_group[j - K] >= 0;  // a padded candidate has group -1 (so has one whose group is negative)
      if (ok) v |= 1u << k;
      if (ok && j < K) g |= 1u << k;
    }
    s_valid[tid] = v, s_live[tid] = g;
  }
  __syncthreads();
  // collision bits of candidate i against boxes 32 w .. 32 w + 31
  for (int item = tid; item < S * W; item += kPB) {
    const int i = item / W, w = item - i * W;
    uint32_t word = 0;
    if (s_valid[(K + i) >> 5] >> ((K + i) & 31) & 1u) {
      double a[8];
#pragma unroll
      for (int k = 0; k < 8; k++) a[k] = corners[(size_t)(K + i) * 8 + k];
      const uint32_t vw = s_valid[w];
      for (int k = 0; k < 32; k++) {
        const int j = w * 32 + k;
        if (!(vw >> k & 1u) || j == K + i) continue;
        double q[8];
#pragma unroll
        for (int e = 0; e < 8; e++) q[e] = corners[(size_t)j * 8 + e];
        if (collide(a, q)) word |= 1u << k;
      }
    }
    bits[item] = word;
  }
  // the members of group g among boxes 32 w .. 32 w + 31
  for (int item = tid; item < p.G * W; item += kPB) {
    const int g = item / W, w = item - g * W;
    uint32_t word = 0;
    for (int k = 0; k < 32; k++) {
      const int j = w * 32 + k;
      if (j >= K && j < n && s_group[j - K] == g) word |= 1u << k;
    }
    gbits[item] = word;
  }
  __syncthreads();
  if (tid < 64) {  // sample_ops.py:137-153 over 202-235, group by group, candidate by candidate; wave 0, lane w owning word w of the live set
    const int lane = tid;
    uint32_t live = lane < W ? s_live[lane] : 0u;  // the gt boxes
    int nacc = 0, nrows = 0;
    for (int g = 0; g < p.G; g++) {
      if (lane < W) live |= gbits[g * W + lane];  // every candidate of the group counts until it is rejected
      for (int c0 = 0; c0 < S; c0 += 64) {
        const int ii = c0 + lane;
        unsigned long long m = __ballot(ii < S && s_group[ii] == g);  // uniform over the wave, as is everything derived from it
        while (m) {
          const int i = c0 + __ffsll((long long)m) - 1;
          m &= m - 1;
          const uint32_t hit = lane < W ? (bits[i * W + lane] & live) : 0u;
          if (__ballot(hit != 0u) != 0ull) {
            if (lane == ((K + i) >> 5)) live &= ~(1u << ((K + i) & 31));
          } else {
            if (lane == 0) s_slot[i] = nacc, s_off[i] = nrows;
            nacc++;
            nrows = (int)min((int64_t)nrows + s_rows[i], (int64_t)INT32_MAX);
          }
        }
      }
    }
    if (lane == 0) s_nacc = nacc, s_nrows = nrows;
  }
  __syncthreads();
  const int nacc = s_nacc;
  if (tid == 0) p.num_out[b] = ng + nacc, p.pasted_rows[b] = s_nrows;
  for (int i = tid; i < S; i += kPB) {
    p.accept[(int64_t)b * S + i] = s_slot[i] >= 0 ? 1 : 0;
    p.paste_offset[(int64_t)b * S + i] = s_slot[i] >= 0 ? s_off[i] : -1;
  }
  // [gt, accepted]; zeros and class -1 beyond
  for (int j = tid; j < n; j += kPB) {
    int dst = -1;
    const float* bx = nullptr;
    int cls = -1;
    if (j < ng) {
      dst = j, bx = p.gt_boxes + ((int64_t)b * K + j) * D, cls = p.gt_cls[(int64_t)b * K + j];
    } else if (j >= K && s_slot[j - K] >= 0) {
      dst = ng + s_slot[j - K], bx = p.cand_boxes + ((int64_t)b * S + (j - K)) * D, cls = p.cand_cls[(int64_t)b * S + (j - K)];
    }
    if (dst >= 0) {
      float* o = p.boxes_out + ((int64_t)b * n + dst) * D;
      for (int e = 0; e < D; e++) o[e] = bx[e];
      p.classes_out[(int64_t)b * n + dst] = cls;
    }
    if (j >= ng + nacc) {
      float* o = p.boxes_out + ((int64_t)b * n + j) * D;
      for (int e = 0; e < D; e++) o[e] = 0.f;
      p.classes_out[(int64_t)b * n + j] = -1;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------------------- point pass

struct PBox {
  float cx, cy, cz, hx, hy, hz, r2, pad;
  double cs, sn;
};

struct PointArgs {
  const float* points;
  int64_t N;
  int stride, B, S, D, nch;
  const float* cand_boxes;
  const int32_t* paste_offset;
};

__device__ __forceinline__ int row_frame(const float* __restrict__ pts, int64_t r, int64_t N, int stride, int B) {
  if (r >= N) return -1;
  const float bf = pts[r * stride];
  return (bf >= 0.f && bf < (float)B) ? (int)bf : -1;
}

// min and max of the valid frame indices of the chunk (lo > hi: none); every thread returns the same pair
__device__ __forceinline__ void frame_span(const int* fr, int& lo, int& hi, int* s_red) {
  int l = INT32_MAX, h = -1;
#pragma unroll
  for (int it = 0; it < kChunkIters; it++)
    if (fr[it] >= 0) l = min(l, fr[it]), h = max(h, fr[it]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) l = min(l, __shfl_xor(l, d)), h = max(h, __shfl_xor(h, d));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_red[2 * wave] = l, s_red[2 * wave + 1] = h;
  __syncthreads();
  lo = min(min(s_red[0], s_red[2]), min(s_red[4], s_red[6]));
  hi = max(max(s_red[1], s_red[3]), max(s_red[5], s_red[7]));
  if (lo > hi) lo = 0, hi = -1;  // no valid row: an empty span that is safe to add a thread index to
  __syncthreads();
}

__global__ __launch_bounds__(64) void k_paste_head(const int32_t* __restrict__ pasted_rows, int B, int nch, uint32_t* __restrict__ arr) {
  for (int b = threadIdx.x; b < B; b += 64) arr[(int64_t)b * (nch + 1)] = pasted_rows != nullptr ? (uint32_t)max(pasted_rows[b], 0) : 0u;
}

__global__ __launch_bounds__(kPB) void k_paste_flags(PointArgs p, uint32_t* __restrict__ keepw, uint32_t* __restrict__ arr) {
  __shared__ PBox s_box[kMaxBoxes];
  __shared__ int s_wn[kPB / 64], s_red[8], s_nbox;
  __shared__ int s_wcnt[kPB / 64][kMaxB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kChunk;
  int fr[kChunkIters];
  float x[kChunkIters], y[kChunkIters], z[kChunkIters];
  unsigned keep = 0;
#pragma unroll
  for (int it = 0; it < kChunkIters; it++) {
    const int64_t r = r0 + it * kPB + tid;
    fr[it] = row_frame(p.points, r, p.N, p.stride, p.B);
    x[it] = y[it] = z[it] = 0.f;
    if (fr[it] >= 0) {
      const float* q = p.points + r * p.stride;
      x[it] = q[1], y[it] = q[2], z[it] = q[3];
      keep |= 1u << it;
    }
  }
  for (int i = tid; i < (kPB / 64) * kMaxB; i += kPB) (&s_wcnt[0][0])[i] = 0;
  int lo, hi;
  frame_span(fr, lo, hi, s_red);
  for (int f = lo; f <= hi; f++) {  // lo, hi are uniform: every thread takes every barrier
    // the frame's accepted boxes, compacted in candidate order
    if (tid == 0) s_nbox = 0;
    __syncthreads();
    for (int i0 = 0; i0 < p.S; i0 += kPB) {
      const int i = i0 + tid;
      const bool acc = i < p.S && p.paste_offset[(int64_t)f * p.S + i] >= 0;
      const unsigned long long m = __ballot(acc);
      if (lane == 0) s_wn[wave] = __popcll(m);
      __syncthreads();
      int at = s_nbox + __popcll(m & ((1ull << lane) - 1ull));
      for (int w = 0; w < wave; w++) at += s_wn[w];
      if (acc) {
        const float* bx = p.cand_boxes + ((int64_t)f * p.S + i) * p.D;
        PBox e;
        e.cx = bx[0], e.cy = bx[1], e.cz = bx[2], e.hx = bx[3] * 0.5f, e.hy = bx[4] * 0.5f, e.hz = bx[5] * 0.5f;
        e.r2 = (e.hx * e.hx + e.hy * e.hy) * 1.001f + 1e-12f;  // above the corner distance whatever the rounding of the fp32 test below
        e.pad = 0.f;
        e.cs = cos((double)bx[p.D - 1]), e.sn = sin((double)bx[p.D - 1]);
        s_box[at] = e;
      }
      __syncthreads();
      if (tid == 0) s_nbox += s_wn[0] + s_wn[1] + s_wn[2] + s_wn[3];
      __syncthreads();
    }
    const int nb = s_nbox;
#pragma unroll
    for (int it = 0; it < kChunkIters; it++) {
      if (fr[it] != f) continue;
      bool in = false;
      for (int e = 0; e < nb && !in; e++) {
        const PBox& bx = s_box[e];
        const float dx = x[it] - bx.cx, dy = y[it] - bx.cy;
        if (!(dx * dx + dy * dy <= bx.r2)) continue;
        // points_in_boxes_jit, in fp64 on the fp32 inputs; the halves of fp32 sizes are exact
        if (!(fabs((double)z[it] - (double)bx.cz) <= (double)bx.hz)) continue;
        const double sx = (double)x[it] - (double)bx.cx, sy = (double)y[it] - (double)bx.cy;
        const double lx = sx * bx.cs + sy * bx.sn, ly = -sx * bx.sn + sy * bx.cs;
        in = fabs(lx) <= (double)bx.hx && fabs(ly) <= (double)bx.hy;
      }
      if (in) keep &= ~(1u << it);
    }
    __syncthreads();
  }
  // one keep bit per row, one count per (wave, frame)
#pragma unroll
  for (int it = 0; it < kChunkIters; it++) {
    const bool k = keep >> it & 1u;
    const unsigned long long m = __ballot(k);
    if (lane == 0) {
      const int64_t w = (r0 + it * kPB + wave * 64) >> 5;
      keepw[w] = (uint32_t)m, keepw[w + 1] = (uint32_t)(m >> 32);
    }
    for (int f = lo; f <= hi; f++) {
      const unsigned long long mf = __ballot(k && fr[it] == f);
      if (lane == 0) s_wcnt[wave][f] += __popcll(mf);  // this wave's own counter
    }
  }
  __syncthreads();
  for (int f = tid; f < p.B; f += kPB)
    arr[(int64_t)f * (p.nch + 1) + 1 + blockIdx.x] = (uint32_t)(s_wcnt[0][f] + s_wcnt[1][f] + s_wcnt[2][f] + s_wcnt[3][f]);
}

__device__ __forceinline__ int64_t prefix_at(const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk, int64_t i) {
  return (int64_t)blk[i >> PNX_SCAN_SHIFT] + pre[i];
}

__global__ __launch_bounds__(kPB) void k_paste_write(PointArgs p, const uint32_t* __restrict__ keepw, const uint32_t* __restrict__ pre,
                                                     const uint32_t* __restrict__ blk, int nblk, const double* __restrict__ xform, float* __restrict__ out,
                                                     int64_t capacity) {
  __shared__ int s_red[8];
  __shared__ int s_wave[kPB / 64][kMaxB];
  __shared__ int64_t s_run[kMaxB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kChunk;
  int fr[kChunkIters];
  unsigned keep = 0;
#pragma unroll
  for (int it = 0; it < kChunkIters; it++) {
    const int64_t r = r0 + it * kPB + tid;
    fr[it] = row_frame(p.points, r, p.N, p.stride, p.B);
    if (r < p.N && (keepw[r >> 5] >> (r & 31) & 1u)) keep |= 1u << it;
  }
  int lo, hi;
  frame_span(fr, lo, hi, s_red);
  for (int f = lo + tid; f <= hi; f += kPB) s_run[f] = prefix_at(pre, blk, (int64_t)f * (p.nch + 1) + 1 + blockIdx.x);
  __syncthreads();
#pragma unroll
  for (int it = 0; it < kChunkIters; it++) {
    const bool k = keep >> it & 1u;
    int before = 0;
    for (int f = lo; f <= hi; f++) {
      const bool mine = k && fr[it] == f;
      const unsigned long long m = __ballot(mine);
      if (mine) before = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_wave[wave][f] = __popcll(m);
    }
    __syncthreads();
    if (k) {
      const int f = fr[it];
      int64_t dst = s_run[f] + before;
      for (int w = 0; w < wave; w++) dst += s_wave[w][f];
      if (dst < capacity) {
        const float* q = p.points + (r0 + it * kPB + tid) * p.stride;
        float* o = out + dst * p.stride;
        const Xform xf = load_xform(xform, f);
        float x = q[1], y = q[2], z = q[3];
        xform_point(xf, x, y, z);
        o[0] = (float)f, o[1] = x, o[2] = y, o[3] = z;
        for (int c = 4; c < p.stride; c++) o[c] = q[c];
      }
    }
    __syncthreads();
    for (int f = lo + tid; f <= hi; f += kPB) s_run[f] += s_wave[0][f] + s_wave[1][f] + s_wave[2][f] + s_wave[3][f];
    __syncthreads();
  }
}

// workgroup (frame, candidate): the accepted object's bank rows, moved to the box centre with fp32 adds (sample_ops.py:169)
__global__ __launch_bounds__(kPB) void k_paste_objects(PointArgs p, const int32_t* __restrict__ cand_bank, const float* __restrict__ bank,
                                                       const int64_t* __restrict__ bank_offsets, int n_obj, int64_t bank_rows,
                                                       const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk, const double* __restrict__ xform,
                                                       float* __restrict__ out, int64_t capacity) {
  const int f = blockIdx.x / p.S, i = blockIdx.x - f * p.S;
  const int off = p.paste_offset[(int64_t)f * p.S + i];
  const int id = cand_bank[(int64_t)f * p.S + i];
  if (off < 0 || id < 0 || id >= n_obj) return;
  const int64_t b0 = min(max(bank_offsets[id], (int64_t)0), bank_rows), b1 = min(max(bank_offsets[id + 1], b0), bank_rows);
  const float* bx = p.cand_boxes + ((int64_t)f * p.S + i) * p.D;
  const float cx = bx[0], cy = bx[1], cz = bx[2];
  const int F = p.stride - 1;
  const int64_t base = prefix_at(pre, blk, (int64_t)f * (p.nch + 1)) + off;
  const Xform xf = load_xform(xform, f);
  for (int64_t r = threadIdx.x; r < b1 - b0; r += kPB) {
    const int64_t dst = base + r;
    if (dst >= capacity) break;
    const float* q = bank + (b0 + r) * F;
    float x = __fadd_rn(q[0], cx), y = __fadd_rn(q[1], cy), z = __fadd_rn(q[2], cz);
    xform_point(xf, x, y, z);
    float* o = out + dst * p.stride;
    o[0] = (float)f, o[1] = x, o[2] = y, o[3] = z;
    for (int c = 3; c < F; c++) o[1 + c] = q[c];
  }
}

// rows of frame f in the output = distance between the frame's first entry of the scanned array and the next frame's (or the total)
__global__ __launch_bounds__(64) void k_paste_frame_rows(const uint32_t* __restrict__ pre, const uint32_t* __restrict__ blk, int nblk, int B, int nch,
                                                         int32_t* __restrict__ frame_rows) {
  for (int f = threadIdx.x; f < B; f += 64) {
    const int64_t begin = prefix_at(pre, blk, (int64_t)f * (nch + 1));
    const int64_t end = f + 1 < B ? prefix_at(pre, blk, (int64_t)(f + 1) * (nch + 1)) : (int64_t)blk[nblk];
    frame_rows[f] = (int32_t)(end - begin);
  }
}

__global__ __launch_bounds__(kPB) void k_paste_tail(float* __restrict__ out, int stride, int64_t capacity, const int32_t* __restrict__ n_out) {
  const int64_t i = (int64_t)blockIdx.x * kPB + threadIdx.x;
  if (i >= capacity || i < (int64_t)n_out[0]) return;
  float* o = out + i * stride;
  o[0] = -1.0f;
  for (int c = 1; c < stride; c++) o[c] = 0.f;
}

__global__ __launch_bounds__(kPB) void k_augment_boxes(float* __restrict__ boxes, const int32_t* __restrict__ num, int B, int M, int D,
                                                       const double* __restrict__ xform) {
  const int64_t i = (int64_t)blockIdx.x * kPB + threadIdx.x;
  if (i >= (int64_t)B * M) return;
  const int b = (int)(i / M), j = (int)(i - (int64_t)b * M);
  if (num != nullptr && j >= num[b]) return;
  const Xform xf = load_xform(xform, b);
  if (xf.flags == 0) return;
  float* q = boxes + i * D;
  float v[9];
  const bool vel = D == 9;
#pragma unroll
  for (int e = 0; e < 6; e++) v[e] = q[e];
  v[6] = vel ? q[6] : 0.f, v[7] = vel ? q[7] : 0.f, v[8] = q[D - 1];
  xform_box(xf, v, vel);
#pragma unroll
  for (int e = 0; e < 6; e++) q[e] = v[e];
  if (vel) q[6] = v[6], q[7] = v[7];
  q[D - 1] = v[8];
}

// Point pass: keep bits of the scene rows (one word per 32 rows of a chunk), the per-(frame, chunk) row counts with one head slot per frame
// (the pasted rows), their exclusive prefix and the block totals of the two-level scan.
struct PasteWs {
  uint32_t *keepw, *arr, *pre, *blk;
  int nch, nblk;
  int64_t len;
  size_t bytes;
};
PasteWs paste_carve(void* base, int64_t n_points, int batch) {
  PasteWs w;
  PnxCarver c(base);
  w.nch = (int)((n_points + kChunk - 1) / kChunk);
  w.len = (int64_t)batch * (w.nch + 1);
  w.nblk = (int)((w.len + PNX_SCAN_ITEMS - 1) / PNX_SCAN_ITEMS);
  w.keepw = c.take<uint32_t>((size_t)w.nch * (kChunk / 32) + 8);
  w.arr = c.take<uint32_t>(w.len + 8);
  w.pre = c.take<uint32_t>(w.len + 8);
  w.blk = c.take<uint32_t>(w.nblk + 8);
  w.bytes = c.used();
  return w;
}

}  // namespace

extern "C" {

int32_t pnx_paste_chunk_rows(void) { return kChunk; }

int pnx_paste_select(const float* gt_boxes, const int32_t* gt_cls, const int32_t* num_gt, int32_t batch, int32_t k, int32_t box_dim,
                     const int32_t* cand_bank, const float* cand_boxes, const int32_t* cand_cls, const int32_t* cand_group, int32_t s, int32_t n_groups,
                     const int64_t* bank_offsets, int32_t n_obj, uint8_t* accept, int32_t* paste_offset, float* boxes_out, int32_t* classes_out,
                     int32_t* num_out, int32_t* pasted_rows, pnx_stream_t stream) {
  PNX_REQUIRE(batch >= 1 && batch <= PNX_PASTE_MAX_BATCH && k >= 0 && s >= 0, PNX_ERR_INVALID, "pnx_paste_select: bad sizes (batch %d outside 1..%d, k %d, s %d)",
              batch, PNX_PASTE_MAX_BATCH, k, s);
  PNX_REQUIRE(box_dim == 7 || box_dim == 9, PNX_ERR_INVALID, "pnx_paste_select: box_dim %d is neither 7 nor 9", box_dim);
  if (cand_bank == nullptr) s = 0;
  PNX_REQUIRE(k + s >= 1, PNX_ERR_INVALID, "pnx_paste_select: no gt box and no candidate (k + s = 0)");
  PNX_REQUIRE(k + s <= PNX_PASTE_MAX_BOXES, PNX_ERR_UNSUPPORTED, "pnx_paste_select: k + s = %d boxes per frame, more than PNX_PASTE_MAX_BOXES = %d", k + s,
              PNX_PASTE_MAX_BOXES);
  PNX_REQUIRE(k == 0 || (gt_boxes && gt_cls), PNX_ERR_INVALID, "pnx_paste_select: null pointer (boxes / classes of %d gt objects)", k);
  PNX_REQUIRE(s == 0 || (cand_boxes && cand_cls && cand_group && bank_offsets && accept && paste_offset), PNX_ERR_INVALID,
              "pnx_paste_select: null pointer (a candidate array, the bank offsets, accept or paste_offset)");
  PNX_REQUIRE(s == 0 || (n_groups >= 1 && n_groups <= kMaxGroups && n_obj >= 1), PNX_ERR_INVALID, "pnx_paste_select: n_groups %d outside 1..%d or n_obj %d < 1",
              n_groups, kMaxGroups, n_obj);
  PNX_REQUIRE(boxes_out && classes_out && num_out && pasted_rows, PNX_ERR_INVALID, "pnx_paste_select: null pointer (an output)");
  SelectArgs p{gt_boxes, gt_cls, num_gt, cand_bank, cand_boxes, cand_cls, cand_group, bank_offsets, accept, paste_offset, boxes_out, classes_out, num_out,
               pasted_rows, k, s, box_dim, s == 0 ? 0 : n_groups, n_obj};
  const size_t lds = select_lds_bytes(k, s, p.G);
  if (lds > 48 * 1024) {
    const int rc = pnx_lds_optin<k_paste_select>(lds);
    if (rc != PNX_OK) return rc;
  }
  k_paste_select<<<batch, kPB, lds, (hipStream_t)stream>>>(p);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

size_t pnx_paste_augment_workspace_bytes(int64_t n_points, int32_t batch) {
  if (n_points < 0 || batch <= 0) return 0;
  return paste_carve(nullptr, n_points, batch).bytes;
}

int pnx_paste_augment_points(const float* points, int64_t n_points, int32_t point_dim, int32_t batch, const int32_t* cand_bank, const float* cand_boxes,
                             const int32_t* paste_offset, const int32_t* pasted_rows, int32_t s, int32_t box_dim, const float* bank_points,
                             const int64_t* bank_offsets, int32_t n_obj, int64_t bank_rows, const double* xform, float* out, int64_t capacity,
                             int32_t* n_out, int32_t* frame_rows, void* workspace, size_t workspace_bytes, pnx_stream_t stream) {
  PNX_REQUIRE(n_points >= 0 && point_dim >= 3 && point_dim <= 64 && capacity >= 0, PNX_ERR_INVALID,
              "pnx_paste_augment_points: bad sizes (n_points %lld, point_dim %d outside 3..64, capacity %lld)", (long long)n_points, point_dim, (long long)capacity);
  PNX_REQUIRE(batch >= 1 && batch <= PNX_PASTE_MAX_BATCH, PNX_ERR_INVALID, "pnx_paste_augment_points: batch %d outside 1..%d", batch, PNX_PASTE_MAX_BATCH);
  PNX_REQUIRE(n_points == 0 || points, PNX_ERR_INVALID, "pnx_paste_augment_points: null pointer (points)");
  PNX_REQUIRE(capacity == 0 || out, PNX_ERR_INVALID, "pnx_paste_augment_points: null pointer (out)");
  PNX_REQUIRE(n_out && frame_rows, PNX_ERR_INVALID, "pnx_paste_augment_points: null pointer (n_out / frame_rows)");
  PNX_REQUIRE(n_points < ((int64_t)1 << 31) - kChunk && capacity < ((int64_t)1 << 31), PNX_ERR_UNSUPPORTED, "pnx_paste_augment_points: more than 2^31 rows");
  if (cand_bank == nullptr) s = 0;
  if (s > 0) {
    PNX_REQUIRE(box_dim == 7 || box_dim == 9, PNX_ERR_INVALID, "pnx_paste_augment_points: box_dim %d is neither 7 nor 9", box_dim);
    PNX_REQUIRE(s <= PNX_PASTE_MAX_BOXES, PNX_ERR_UNSUPPORTED, "pnx_paste_augment_points: %d candidates per frame, more than PNX_PASTE_MAX_BOXES = %d", s,
                PNX_PASTE_MAX_BOXES);
    PNX_REQUIRE(cand_boxes && paste_offset && pasted_rows && bank_points && bank_offsets && n_obj >= 1 && bank_rows >= 0, PNX_ERR_INVALID,
                "pnx_paste_augment_points: null pointer or bad size (a candidate array, paste_offset, pasted_rows or the bank)");
  }
  const PasteWs ws = paste_carve(workspace, n_points, batch);
  PNX_CHECK_WORKSPACE(workspace, workspace_bytes, ws.bytes, "pnx_paste_augment_points");
  hipStream_t st = (hipStream_t)stream;
  PointArgs p{points, n_points, point_dim + 1, batch, s, box_dim, ws.nch, cand_boxes, paste_offset};
  k_paste_head<<<1, 64, 0, st>>>(s > 0 ? pasted_rows : nullptr, batch, ws.nch, ws.arr);
  if (ws.nch > 0) k_paste_flags<<<ws.nch, kPB, 0, st>>>(p, ws.keepw, ws.arr);
  k_scan_local<SCAN_IDENT><<<ws.nblk, kBlock, 0, st>>>(ws.arr, ws.len, ws.pre, ws.blk);
  k_scan_blocks<<<1, kBlock, 0, st>>>(ws.blk, ws.nblk, n_out);
  k_paste_frame_rows<<<1, 64, 0, st>>>(ws.pre, ws.blk, ws.nblk, batch, ws.nch, frame_rows);
  if (ws.nch > 0) k_paste_write<<<ws.nch, kPB, 0, st>>>(p, ws.keepw, ws.pre, ws.blk, ws.nblk, xform, out, capacity);
  if (s > 0) k_paste_objects<<<batch * s, kPB, 0, st>>>(p, cand_bank, bank_points, bank_offsets, n_obj, bank_rows, ws.pre, ws.blk, xform, out, capacity);
  if (capacity > 0) k_paste_tail<<<(unsigned)((capacity + kPB - 1) / kPB), kPB, 0, st>>>(out, point_dim + 1, capacity, n_out);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

int pnx_augment_boxes(float* boxes, const int32_t* num, int32_t batch, int32_t m, int32_t box_dim, const double* xform, pnx_stream_t stream) {
  PNX_REQUIRE(batch >= 1 && batch <= PNX_PASTE_MAX_BATCH && m >= 0, PNX_ERR_INVALID, "pnx_augment_boxes: bad sizes (batch %d outside 1..%d, m %d)", batch,
              PNX_PASTE_MAX_BATCH, m);
  PNX_REQUIRE(box_dim == 7 || box_dim == 9, PNX_ERR_INVALID, "pnx_augment_boxes: box_dim %d is neither 7 nor 9", box_dim);
  PNX_REQUIRE(m == 0 || boxes, PNX_ERR_INVALID, "pnx_augment_boxes: null pointer (boxes)");
  if (m == 0 || xform == nullptr) return PNX_OK;
  const int64_t n = (int64_t)batch * m;
  k_augment_boxes<<<(unsigned)((n + kPB - 1) / kPB), kPB, 0, (hipStream_t)stream>>>(boxes, num, batch, m, box_dim, xform);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

}  // extern "C"
