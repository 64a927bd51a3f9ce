// assign.hip -- CenterHead training labels from ground-truth boxes, on the device, for gfx950.
//
// Reference: det3d/datasets/pipelines/assign.py:23-116 (AssignLabel.__call__) with det3d/datasets/pipelines/center_utils.py:12-60
// (gaussian_radius, gaussian2D, draw_gaussian): a per-object Python loop over numpy patches on the host, followed by the upload of the dense
// heat maps.  Here a padded (B, K, 9) box tensor [x y z dx dy dz vx vy yaw] and its (B, K) global class indices become the per-task label
// lists CenterHead.loss reads (hm (B,ncls,H,W), ind / mask / cat (B,M), anno_box (B,M,10), gt_boxes (B,M,7)) in two launches for all tasks:
//   k_assign_objects  one workgroup per frame.  Per object, in fp64 as numpy does it (the boxes are fp32, the config values are Python
//                     floats, so every mixed expression of the reference is fp64): the size in cells (two divisions), the CenterNet radius
//                     (three quadratic roots, truncated), the centre cell.  Survivors of a task take slots 0, 1, .. in input order: a
//                     ballot-based block scan per task, the per-task running counts carried from one 256-object chunk to the next, no
//                     atomics.  Every slot of every list is written exactly once (zeros beyond the count), and a compact draw list
//                     (x, y, radius, class) per (frame, task) is left in the workspace.
//   k_assign_heatmap  a gather.  One workgroup owns a 128 x 8 tile of one class plane of one (frame, task) map; it keeps in LDS the draw
//                     list entries of that class whose (2r+1)^2 window meets the tile, and every thread takes the running maximum over them
//                     for its four cells.  Every cell is stored exactly once (zeros included), 16 bytes per lane along W when the row
//                     pitch allows it: no memset, no floating-point atomics, the result does not depend on any order.
// Mirrored quirks of the reference:
//   - the third root of gaussian_radius is (b3 + sqrt(b3^2 - 16 o c3)) / 2, NOT divided by its leading coefficient 4 o;
//   - the centre is truncated toward zero, so a centre in (-1, 0) cells lands in cell 0 and is kept, with a negative offset target;
//   - the Gaussian is centred on the integer cell, so the centre cell is exactly 1.0f;
//   - gaussian2D zeroes values below eps * max; the smallest value in a window is exp(-(r^2 + r^2) / (2 ((2r+1)/6)^2)) > e^-9 = 1.2e-4,
//     far above 2.2e-16, so the threshold never fires and needs no code here.
// Unlike the reference (IndexError), a task with more than max_objs survivors drops the later ones, from the lists and from the heat map; the
// un-clamped count is reported.
#include <math.h>

#include "pnx_common.h"

namespace {

constexpr int kAB = 256;            // threads of both kernels
constexpr int kTileW = 128;         // heat-map tile: 32 lanes x 4 cells wide,
constexpr int kTileH = kAB / 32;    // 8 rows
constexpr int kDrawCap = 1024;      // draw-list entries staged in LDS per round

struct AssignTask {
  int osf, H, W, ncls;
  int tile0;  // first workgroup of this task in the heat-map launch
  int tx;     // tiles per row
  int vec;    // 16-byte stores possible (W % 4 == 0 and an aligned base)
  int pad;
};

struct AssignParams {
  double lox, loy, vx, vy, overlap;
  int min_radius, max_objs, n_tasks, n_classes, B, K;
  AssignTask task[PNX_ASSIGN_MAX_TASKS];
  signed char class_task[PNX_ASSIGN_MAX_CLASSES];
  signed char class_cls[PNX_ASSIGN_MAX_CLASSES];
  float* hm[PNX_ASSIGN_MAX_TASKS];
  float* anno[PNX_ASSIGN_MAX_TASKS];
  int64_t* ind[PNX_ASSIGN_MAX_TASKS];
  uint8_t* mask[PNX_ASSIGN_MAX_TASKS];
  int64_t* cat[PNX_ASSIGN_MAX_TASKS];
  float* gtb[PNX_ASSIGN_MAX_TASKS];
};

// center_utils.py:12-32 in fp64, operation by operation (-ffp-contract=off keeps the products and sums apart)
__device__ __forceinline__ double gaussian_radius(double height, double width, double o) {
  const double b1 = height + width;
  const double c1 = width * height * (1.0 - o) / (1.0 + o);
  const double r1 = (b1 + sqrt(b1 * b1 - 4.0 * c1)) / 2.0;
  const double b2 = 2.0 * (height + width);
  const double c2 = (1.0 - o) * width * height;
  const double r2 = (b2 + sqrt(b2 * b2 - 16.0 * c2)) / 2.0;
  const double a3 = 4.0 * o;
  const double b3 = -2.0 * o * (height + width);
  const double c3 = (o - 1.0) * width * height;
  const double r3 = (b3 + sqrt(b3 * b3 - 4.0 * a3 * c3)) / 2.0;
  return fmin(r1, fmin(r2, r3));
}

__global__ __launch_bounds__(kAB) void k_assign_objects(AssignParams p, const float* __restrict__ boxes, const int32_t* __restrict__ cls,
                                                        const int32_t* __restrict__ num_gt, int32_t* __restrict__ counts, int4* __restrict__ draw,
                                                        int32_t* __restrict__ draw_len) {
  __shared__ int s_wave[kAB / 64][PNX_ASSIGN_MAX_TASKS];
  __shared__ int s_run[PNX_ASSIGN_MAX_TASKS];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = p.n_tasks, M = p.max_objs;
  int n = p.K;
  if (num_gt != nullptr) n = min(max(num_gt[b], 0), p.K);
  if (tid < PNX_ASSIGN_MAX_TASKS) s_run[tid] = 0;
  __syncthreads();
  for (int k0 = 0; k0 < n; k0 += kAB) {  // n is uniform over the workgroup: every thread takes every barrier
    const int k = k0 + tid;
    int t = -1, c = 0, radius = 0, cx = 0, cy = 0;
    float ctx = 0.f, cty = 0.f;
    const float* bx = boxes + ((int64_t)b * p.K + (k < n ? k : 0)) * 9;
    if (k < n) {
      const int g = cls[(int64_t)b * p.K + k];
      if (g >= 0 && g < p.n_classes) {
        const int tt = p.class_task[g];
        const AssignTask tk = p.task[tt];
        const float x = bx[0], y = bx[1];
        const double sx = (double)bx[3] / p.vx / (double)tk.osf;
        const double sy = (double)bx[4] / p.vy / (double)tk.osf;
        if (sx > 0.0 && sy > 0.0 && isfinite(x) && isfinite(y)) {
          double r = gaussian_radius(sy, sx, p.overlap);
          r = fmin(r, 1.0e9);  // an infinite size: keeps the conversion and 2r+1 inside int32
          radius = max(p.min_radius, (int)r);
          ctx = (float)(((double)x - p.lox) / p.vx / (double)tk.osf);
          cty = (float)(((double)y - p.loy) / p.vy / (double)tk.osf);
          cx = (int)ctx, cy = (int)cty;  // truncation; the conversion saturates, so a far centre fails the range test
          if (cx >= 0 && cx < tk.W && cy >= 0 && cy < tk.H) t = tt, c = p.class_cls[g];
        }
      }
    }
    // stable per-task slot: objects before this one in the chunk (earlier waves, then earlier lanes) plus the chunks before
    int before = 0;
    for (int tt = 0; tt < T; tt++) {
      const unsigned long long m = __ballot(t == tt);
      if (t == tt) before = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) s_wave[wave][tt] = __popcll(m);
    }
    __syncthreads();
    if (t >= 0) {
      int slot = s_run[t] + before;
      for (int w = 0; w < wave; w++) slot += s_wave[w][t];
      if (slot < M) {
        const AssignTask tk = p.task[t];
        const int64_t o = (int64_t)b * M + slot;
        p.ind[t][o] = (int64_t)cy * tk.W + cx;
        p.mask[t][o] = 1;
        p.cat[t][o] = c;
        float* g7 = p.gtb[t] + o * 7;
        g7[0] = bx[0], g7[1] = bx[1], g7[2] = bx[2], g7[3] = bx[3], g7[4] = bx[4], g7[5] = bx[5], g7[6] = bx[8];
        float* a = p.anno[t] + o * 10;
        a[0] = ctx - (float)cx;
        a[1] = cty - (float)cy;
        a[2] = bx[2];
        a[3] = (float)log((double)bx[3]);  // fp64 on the fp32 input, rounded once
        a[4] = (float)log((double)bx[4]);
        a[5] = (float)log((double)bx[5]);
        a[6] = bx[6];
        a[7] = bx[7];
        a[8] = (float)sin((double)bx[8]);
        a[9] = (float)cos((double)bx[8]);
        draw[((int64_t)b * T + t) * M + slot] = make_int4(cx, cy, radius, c);
      }
    }
    __syncthreads();
    if (tid < T) {
      int s = s_run[tid];
      for (int w = 0; w < kAB / 64; w++) s += s_wave[w][tid];
      s_run[tid] = s;
    }
    __syncthreads();
  }
  if (tid < T) {
    counts[b * T + tid] = s_run[tid];
    draw_len[b * T + tid] = min(s_run[tid], M);
  }
  // the unused slots: zeros, as the reference's np.zeros leaves them
  for (int t = 0; t < T; t++) {
    const int used = min(s_run[t], M);
    for (int s = used + tid; s < M; s += kAB) {
      const int64_t o = (int64_t)b * M + s;
      p.ind[t][o] = 0;
      p.mask[t][o] = 0;
      p.cat[t][o] = 0;
      float* g7 = p.gtb[t] + o * 7;
#pragma unroll
      for (int j = 0; j < 7; j++) g7[j] = 0.f;
      float* a = p.anno[t] + o * 10;
#pragma unroll
      for (int j = 0; j < 10; j++) a[j] = 0.f;
    }
  }
}

// workgroup -> (task, frame, class plane, tile): task[t].tile0 .. +B * ncls * ty * tx
__global__ __launch_bounds__(kAB) void k_assign_heatmap(AssignParams p, const int4* __restrict__ draw, const int32_t* __restrict__ draw_len) {
  __shared__ int4 s_e[kDrawCap];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  int t = 0;
  while (t + 1 < p.n_tasks && (int)blockIdx.x >= p.task[t + 1].tile0) t++;
  const AssignTask tk = p.task[t];
  int w = blockIdx.x - tk.tile0;
  const int tix = w % tk.tx;
  w /= tk.tx;
  const int ty = (tk.H + kTileH - 1) / kTileH;
  const int tiy = w % ty;
  w /= ty;
  const int c = w % tk.ncls;
  const int b = w / tk.ncls;
  const int x_lo = tix * kTileW, y_lo = tiy * kTileH;
  const int x_hi = min(x_lo + kTileW, tk.W) - 1, y_hi = min(y_lo + kTileH, tk.H) - 1;
  const int y = y_lo + (tid >> 5), x0 = x_lo + (tid & 31) * 4;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int n = draw_len[b * p.n_tasks + t];
  const int4* list = draw + ((int64_t)b * p.n_tasks + t) * p.max_objs;
  for (int e0 = 0; e0 < n; e0 += kDrawCap) {
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int e = e0 + tid; e < min(n, e0 + kDrawCap); e += kAB) {
      const int4 v = list[e];  // x, y, radius, class
      // 64-bit: r may be as large as 1e9
      const bool hit = v.w == c && (int64_t)v.x - v.z <= x_hi && (int64_t)v.x + v.z >= x_lo && (int64_t)v.y - v.z <= y_hi && (int64_t)v.y + v.z >= y_lo;
      if (hit) s_e[atomicAdd(&s_n, 1)] = v;  // LDS integer counter; the maximum below does not depend on the order
    }
    __syncthreads();
    const int m = s_n;
    if (y <= y_hi) {
      for (int e = 0; e < m; e++) {
        const int4 v = s_e[e];
        const double dy = (double)y - (double)v.y, r = (double)v.z;
        if (fabs(dy) > r) continue;
        const double sigma = (2.0 * r + 1.0) / 6.0;
        const double den = 2.0 * sigma * sigma;
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const double dx = (double)(x0 + j) - (double)v.x;
          if (fabs(dx) <= r) acc[j] = fmaxf(acc[j], (float)exp(-(dx * dx + dy * dy) / den));
        }
      }
    }
    __syncthreads();
  }
  if (y > y_hi || x0 > x_hi) return;
  float* row = p.hm[t] + (((int64_t)b * tk.ncls + c) * tk.H + y) * tk.W;
  if (tk.vec) {  // W % 4 == 0: x0 + 3 <= x_hi
    *reinterpret_cast<float4*>(row + x0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (x0 + j <= x_hi) row[x0 + j] = acc[j];
  }
}

// The draw lists k_assign_objects leaves for k_assign_heatmap: (x, y, radius, class) per object and the length of every (frame, task) list.
struct AssignWs {
  int4* draw;
  int32_t* draw_len;
  size_t bytes;
};
AssignWs assign_carve(void* base, int batch, int n_tasks, int max_objs) {
  AssignWs w;
  PnxCarver c(base);
  const size_t lists = (size_t)batch * n_tasks;
  w.draw = c.take<int4>(lists * max_objs);
  w.draw_len = c.take<int32_t>(lists);
  w.bytes = c.used();
  return w;
}

}  // namespace

extern "C" {

size_t pnx_assign_workspace_bytes(int32_t batch, int32_t n_tasks, int32_t max_objs) {
  if (batch <= 0 || n_tasks <= 0 || max_objs <= 0) return 0;
  return assign_carve(nullptr, batch, n_tasks, max_objs).bytes;
}

int pnx_assign_labels(const float* gt_boxes, const int32_t* gt_cls, const int32_t* num_gt, int32_t batch, int32_t k, const pnx_assign_desc* desc_host,
                      float* const* hm_host, float* const* anno_box_host, int64_t* const* ind_host, uint8_t* const* mask_host, int64_t* const* cat_host,
                      float* const* gt_boxes_out_host, int32_t* counts, void* workspace, size_t workspace_bytes, pnx_stream_t stream) {
  PNX_REQUIRE(desc_host && hm_host && anno_box_host && ind_host && mask_host && cat_host && gt_boxes_out_host && counts && workspace, PNX_ERR_INVALID,
              "pnx_assign_labels: null pointer");
  PNX_REQUIRE(batch >= 1 && k >= 0, PNX_ERR_INVALID, "pnx_assign_labels: bad sizes (batch %d, k %d)", batch, k);
  PNX_REQUIRE(k == 0 || (gt_boxes && gt_cls), PNX_ERR_INVALID, "pnx_assign_labels: null pointer (boxes / classes of %d objects)", k);
  const pnx_assign_desc& d = *desc_host;
  PNX_REQUIRE(d.n_tasks >= 1 && d.n_tasks <= PNX_ASSIGN_MAX_TASKS, PNX_ERR_INVALID, "pnx_assign_labels: n_tasks %d outside 1..%d", d.n_tasks,
              PNX_ASSIGN_MAX_TASKS);
  PNX_REQUIRE(d.max_objs >= 1, PNX_ERR_INVALID, "pnx_assign_labels: max_objs %d < 1", d.max_objs);
  PNX_REQUIRE(d.n_classes >= 1 && d.n_classes <= PNX_ASSIGN_MAX_CLASSES, PNX_ERR_INVALID, "pnx_assign_labels: n_classes %d outside 1..%d", d.n_classes,
              PNX_ASSIGN_MAX_CLASSES);
  PNX_REQUIRE(d.voxel[0] > 0.0 && d.voxel[1] > 0.0 && isfinite(d.lo[0]) && isfinite(d.lo[1]) && d.overlap >= 0.0 && d.overlap < 1.0 && d.min_radius >= 0,
              PNX_ERR_INVALID, "pnx_assign_labels: bad geometry (voxel, range origin, gaussian_overlap in [0, 1), min_radius >= 0)");
  PNX_REQUIRE((int64_t)batch * d.max_objs <= INT32_MAX / 16, PNX_ERR_UNSUPPORTED, "pnx_assign_labels: batch * max_objs too large");
  AssignParams p;
  p.lox = d.lo[0], p.loy = d.lo[1], p.vx = d.voxel[0], p.vy = d.voxel[1], p.overlap = d.overlap;
  p.min_radius = d.min_radius, p.max_objs = d.max_objs, p.n_tasks = d.n_tasks, p.n_classes = d.n_classes, p.B = batch, p.K = k;
  int64_t tiles = 0;
  for (int t = 0; t < PNX_ASSIGN_MAX_TASKS; t++) {
    AssignTask& tk = p.task[t];
    tk = AssignTask{1, 1, 1, 1, 0, 1, 0, 0};
    p.hm[t] = nullptr, p.anno[t] = nullptr, p.ind[t] = nullptr, p.mask[t] = nullptr, p.cat[t] = nullptr, p.gtb[t] = nullptr;
    if (t >= d.n_tasks) continue;
    PNX_REQUIRE(d.osf[t] >= 1 && d.h[t] >= 1 && d.w[t] >= 1 && d.ncls[t] >= 1, PNX_ERR_INVALID, "pnx_assign_labels: task %d: bad osf / map size / class count", t);
    PNX_REQUIRE((int64_t)d.h[t] * d.w[t] <= INT32_MAX, PNX_ERR_UNSUPPORTED, "pnx_assign_labels: task %d: H * W = %d * %d overflows int32", t, d.h[t], d.w[t]);
    PNX_REQUIRE(hm_host[t] && anno_box_host[t] && ind_host[t] && mask_host[t] && cat_host[t] && gt_boxes_out_host[t], PNX_ERR_INVALID,
                "pnx_assign_labels: null pointer (an output of task %d)", t);
    tk.osf = d.osf[t], tk.H = d.h[t], tk.W = d.w[t], tk.ncls = d.ncls[t];
    tk.tx = (tk.W + kTileW - 1) / kTileW;
    tk.tile0 = (int)tiles;
    tk.vec = (tk.W % 4 == 0) && ((uintptr_t)hm_host[t] % 16 == 0);
    tiles += (int64_t)batch * tk.ncls * ((tk.H + kTileH - 1) / kTileH) * tk.tx;
    PNX_REQUIRE(tiles <= INT32_MAX, PNX_ERR_UNSUPPORTED, "pnx_assign_labels: heat maps too large for one launch");
    p.hm[t] = hm_host[t], p.anno[t] = anno_box_host[t], p.ind[t] = ind_host[t], p.mask[t] = mask_host[t], p.cat[t] = cat_host[t], p.gtb[t] = gt_boxes_out_host[t];
  }
  for (int g = 0; g < PNX_ASSIGN_MAX_CLASSES; g++) {
    p.class_task[g] = 0, p.class_cls[g] = 0;
    if (g >= d.n_classes) continue;
    PNX_REQUIRE(d.class_task[g] >= 0 && d.class_task[g] < d.n_tasks && d.class_cls[g] >= 0 && d.class_cls[g] < d.ncls[d.class_task[g]], PNX_ERR_INVALID,
                "pnx_assign_labels: class %d maps to (task %d, class %d), outside the task list", g, d.class_task[g], d.class_cls[g]);
    p.class_task[g] = (signed char)d.class_task[g], p.class_cls[g] = (signed char)d.class_cls[g];
  }
  const AssignWs ws = assign_carve(workspace, batch, d.n_tasks, d.max_objs);
  PNX_CHECK_WORKSPACE(workspace, workspace_bytes, ws.bytes, "pnx_assign_labels");
  hipStream_t st = (hipStream_t)stream;
  k_assign_objects<<<batch, kAB, 0, st>>>(p, gt_boxes, gt_cls, num_gt, counts, ws.draw, ws.draw_len);
  PNX_LAUNCH_CHECK();
  k_assign_heatmap<<<(unsigned)tiles, kAB, 0, st>>>(p, ws.draw, ws.draw_len);
  PNX_LAUNCH_CHECK();
  return PNX_OK;
}

}  // extern "C"
