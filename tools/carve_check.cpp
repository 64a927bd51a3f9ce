// carve_check.cpp -- host sanitizer run over every workspace layout of pillarnext_amd/csrc (no GPU, never through Python).
//
// A layout is one *_carve(base, sizes...) function on PnxCarver.  This program calls it with a null base (the size query), then with a malloc'ed
// block of exactly that many bytes; PNX_CARVE_PROBE makes PnxCarver::take write the first and the last element of every field it hands out, so
// AddressSanitizer sees a field that ends behind `bytes` and UBSan a misaligned one.  The carves live in the anonymous namespaces of their .hip files:
// one program per file, chosen with -DUNIT_<name>, linked against the built library for what the file calls in other files.  From the repository root:
//
//   for u in reader group scatter sparse3d point_layer center_loss assign merge augment decode iou3d; do
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -DUNIT_$u -Xarch_host -fsanitize=address,undefined -c tools/carve_check.cpp -o /tmp/carve_$u.o &&
//     /opt/rocm/llvm/bin/clang++ -fsanitize=address,undefined /tmp/carve_$u.o -Lpillarnext_amd -l:libpnx_hip.so -L/opt/rocm/lib -lamdhip64 \
//       -Wl,-rpath,$PWD/pillarnext_amd -Wl,-rpath,/opt/rocm/lib -o /tmp/carve_$u && ASAN_OPTIONS=detect_leaks=0 /tmp/carve_$u || break
//   done
#define PNX_CARVE_PROBE 1
#include <stdio.h>
#include <stdlib.h>

#if defined(UNIT_reader)
#include "../pillarnext_amd/csrc/reader.hip"
#elif defined(UNIT_group)
#include "../pillarnext_amd/csrc/group.hip"
#elif defined(UNIT_scatter)
#include "../pillarnext_amd/csrc/scatter.hip"
#elif defined(UNIT_sparse3d)
#include "../pillarnext_amd/csrc/sparse3d.hip"
#elif defined(UNIT_point_layer)
#include "../pillarnext_amd/csrc/point_layer_train.hip"
#elif defined(UNIT_center_loss)
#include "../pillarnext_amd/csrc/center_loss.hip"
#elif defined(UNIT_assign)
#include "../pillarnext_amd/csrc/assign.hip"
#elif defined(UNIT_merge)
#include "../pillarnext_amd/csrc/merge.hip"
#elif defined(UNIT_augment)
#include "../pillarnext_amd/csrc/augment.hip"
#elif defined(UNIT_decode)
#include "../pillarnext_amd/csrc/decode.hip"
#elif defined(UNIT_iou3d)
#include "../pillarnext_amd/csrc/iou3d.hip"
#else
#error "pick a unit: -DUNIT_reader, _group, _scatter, _sparse3d, _point_layer, _center_loss, _assign, _merge, _augment, _decode or _iou3d"
#endif

static int g_layouts = 0;

// bytes_of(base) carves over `base` and returns the layout's size
template <typename F>
static void check(const char* what, F bytes_of) {
  const size_t bytes = bytes_of(nullptr);
  void* block = malloc(bytes ? bytes : 1);
  const size_t again = bytes_of(block);
  free(block);
  if (again != bytes || bytes == 0) {
    fprintf(stderr, "%s: %zu bytes from the null base, %zu over the block\n", what, bytes, again);
    exit(1);
  }
  g_layouts++;
}

static const int64_t kCounts[] = {0, 1, 2047, 2048, 2049, 16385};

int main() {
  for (int64_t n : kCounts) {
#if defined(UNIT_reader)
    const double range[6] = {0.0, 0.0, -1.0, 8.0, 8.0, 1.0}, voxel[3] = {0.5, 0.5, 2.0};
    pnx_geom g;
    if (pnx_geom_init(range, voxel, &g) != PNX_OK) return 2;
    for (int batch : {1, 4}) check("carve", [&](void* b) { return carve(b, n, batch, &g).bytes; });
#elif defined(UNIT_group)
    pnx_group_geom g = {};
    for (int k = 0; k < 3; k++) g.voxel[k] = 0.5f, g.grid[k] = k < 2 ? 16 : 4;
    for (int mode : {PNX_GROUP_VOXEL, PNX_GROUP_PILLAR_CLAMP}) {
      g.mode = mode;
      check("group_carve", [&](void* b) { return group_carve(b, n, 6, 2, &g).bytes; });
    }
    check("bilgrad_carve", [&](void* b) { return bilgrad_carve(b, n, 2 * 9 * 11).bytes; });
    for (int64_t rows : kCounts) check("sp3_bilgrad_carve", [&](void* b) { return sp3_bilgrad_carve(b, n, rows).bytes; });
#elif defined(UNIT_scatter)
    for (int64_t p : kCounts) check("sm_carve", [&](void* b) { return sm_carve(b, n, p).bytes; });
#elif defined(UNIT_sparse3d)
    const int32_t grid3[3] = {3, 17, (int32_t)(n % 97) + 1};
    Sp3Grid g;
    if (sp3_grid(2, grid3, &g) != PNX_OK) return 2;
    check("sp3_carve", [&](void* b) { return sp3_carve(b, g).bytes; });
    for (int cout : {18, 72, 144}) check("sp3_wgrad_h_carve", [&](void* b) { return sp3_wgrad_h_carve(b, n, 27, 18, cout).bytes; });
    for (int backward : {0, 1})
      for (int c : {1, 18, 144, 256}) check("sp3_bn_carve", [&](void* b) { return sp3_bn_carve(b, n * 40, c, backward != 0).bytes; });
#elif defined(UNIT_point_layer)
    for (int backward : {0, 1})
      for (int c : {20, 576}) check("pl_carve", [&](void* b) { return pl_carve(b, n, c, c < 256 ? 24 : 256, backward != 0).bytes; });
#elif defined(UNIT_center_loss)
    if (n > 0 && n < 4096) check("loss_carve", [&](void* b) { return loss_carve(b, 2, (int)n).bytes; });
#elif defined(UNIT_assign)
    if (n > 0 && n < 4096)
      for (int tasks : {1, 6}) check("assign_carve", [&](void* b) { return assign_carve(b, 2, tasks, (int)n).bytes; });
#elif defined(UNIT_merge)
    check("merge_carve", [&](void* b) { return merge_carve(b, n).bytes; });
#elif defined(UNIT_augment)
    for (int batch : {1, 2, 64}) check("paste_carve", [&](void* b) { return paste_carve(b, n, batch).bytes; });
#elif defined(UNIT_decode)
    for (int segments : {1, 2, 72}) check("topk_carve", [&](void* b) { return topk_carve(b, n, segments).bytes; });
#elif defined(UNIT_iou3d)
    if (n > 0 && n <= 4096)
      for (int cap : {0, 64}) {
        const int prev = pnx_debug_nms_pair_cap(cap);
        for (int segments : {1, 2, 72}) check("nms_layout", [&](void* b) { return nms_layout(b, segments, (int)n).mask_off; });
        pnx_debug_nms_pair_cap(prev);
      }
#endif
  }
  printf("carve_check: %d layouts carved over blocks of exactly their size\n", g_layouts);
  return g_layouts > 0 ? 0 : 1;
}
