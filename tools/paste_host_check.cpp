// paste_host_check.cpp -- a stand-alone host program over the host code of csrc/lgs_paste.hip: workspace sizing and the argument checks
// that run before any HIP call.  It needs no GPU; build it with the host sanitizers and run it:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/paste_host_check.cpp languagegroundedsemseg_amd/csrc/lgs_paste.hip -o paste_host_check && ./paste_host_check
//
// The few engine symbols lgs_paste.hip links against (error text, launch counters, lgs_aug_bounds) are defined here, so that the
// translation unit under test is the only part of the engine in the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/lgs_engine.h"

namespace lgs {
static std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }
int dispatch_site(const char *, const char *) { return 0; }
void dispatch_hit(int) {}
}  // namespace lgs

extern "C" int lgs_aug_bounds(const void *, int64_t, int, int64_t *, int, void *, void *) {
  std::fprintf(stderr, "lgs_aug_bounds reached: an argument check let a call through\n");
  std::abort();
}

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      return 1;                                                             \
    }                                                                       \
  } while (0)

struct Args {
  // dummy non-null addresses: a call that passes its checks would abort in lgs_aug_bounds above, none of them is dereferenced
  char mem[64];
  const int32_t *coords;
  const float *feats, *bank_points, *bank_colors;
  const int64_t *labels, *bank_labels, *slot_table, *scene_table;
  const double *slot_affines, *scene_xforms, *boxes;
  void *workspace;
  int32_t *coords_out, *placement, *status;
  float *feats_out;
  int64_t *labels_out;
  int64_t n = 100, bank_rows = 10, inst_rows = 10, n_boxes = 1, max_map_cells = 1 << 18;
  int b = 2, slots = 2, trials = 50;
  Args() {
    void *p = mem;
    coords = (const int32_t *)p; feats = bank_points = bank_colors = (const float *)p;
    labels = bank_labels = slot_table = scene_table = (const int64_t *)p;
    slot_affines = scene_xforms = boxes = (const double *)p;
    workspace = p; coords_out = placement = status = (int32_t *)p; feats_out = (float *)p; labels_out = (int64_t *)p;
  }
  int call() const {
    return lgs_paste_instances(coords, feats, labels, n, b, bank_points, bank_colors, bank_labels, bank_rows, slot_table, slot_affines,
                               slots, inst_rows, scene_table, scene_xforms, boxes, n_boxes, nullptr, trials, 0, max_map_cells, workspace,
                               coords_out, feats_out, labels_out, placement, status, nullptr);
  }
};

int main() {
  // workspace sizing: refusals, non-decreasing in the rows, the map region is b * max_map_cells words
  EXPECT(lgs_paste_workspace_bytes(0, 0, 0, 1 << 18) == 0);
  EXPECT(lgs_paste_workspace_bytes(33, 0, 0, 1 << 18) == 0);
  EXPECT(lgs_paste_workspace_bytes(8, LGS_PASTE_MAX_SLOTS + 1, 5000, 1 << 18) == 0);
  EXPECT(lgs_paste_workspace_bytes(8, 3, 0, 1 << 18) == 0 && lgs_paste_workspace_bytes(8, 0, 3, 1 << 18) == 0);
  EXPECT(lgs_paste_workspace_bytes(8, 4, 3, 1 << 18) == 0);
  EXPECT(lgs_paste_workspace_bytes(8, 0, 0, 0) == 0 && lgs_paste_workspace_bytes(8, 0, 0, (1ll << 26) + 1) == 0);
  EXPECT(lgs_paste_workspace_bytes(8, 1, (1ll << 31), 1) == 0 && lgs_paste_workspace_bytes(8, 1, -1, 1) == 0);
  int64_t prev = 0;
  for (int64_t rows : {1ll, 63ll, 64ll, 65ll, 80000ll, 1ll << 20, (1ll << 31) - 257}) {
    const int64_t bytes = lgs_paste_workspace_bytes(32, 1, rows, 1ll << 26);
    EXPECT(bytes >= prev && bytes > 0 && bytes % 256 == 0);
    EXPECT(bytes >= 32 * (1ll << 26) * 4 + rows * (2 * 12 + 4 + 16));
    prev = bytes;
  }
  EXPECT(lgs_paste_workspace_bytes(8, 40, 80000, 1 << 18) - lgs_paste_workspace_bytes(8, 40, 80000, 1 << 17) == 8ll * (1 << 17) * 4);
  EXPECT(lgs_paste_workspace_bytes(1, 0, 0, 1) > 0);

  // argument checks: each call is refused before any HIP call (lgs_aug_bounds above aborts if one gets through)
  Args ok;
  { Args a = ok; a.b = 0; EXPECT(a.call() != 0); }
  { Args a = ok; a.b = 33; EXPECT(a.call() != 0); }
  { Args a = ok; a.slots = LGS_PASTE_MAX_SLOTS + 1; a.inst_rows = 5000; EXPECT(a.call() != 0 && lgs::g_error.find("LGS_PASTE_MAX_SLOTS") != std::string::npos); }
  { Args a = ok; a.slots = -1; EXPECT(a.call() != 0); }
  { Args a = ok; a.inst_rows = 0; EXPECT(a.call() != 0); }
  { Args a = ok; a.inst_rows = 1; EXPECT(a.call() != 0); }
  { Args a = ok; a.trials = 0; EXPECT(a.call() != 0); }
  { Args a = ok; a.max_map_cells = 0; EXPECT(a.call() != 0); }
  { Args a = ok; a.n = -1; EXPECT(a.call() != 0); }
  { Args a = ok; a.n = 1ll << 31; EXPECT(a.call() != 0); }
  { Args a = ok; a.n_boxes = -1; EXPECT(a.call() != 0); }
  { Args a = ok; a.bank_rows = 0; EXPECT(a.call() != 0); }
  { Args a = ok; a.coords = nullptr; EXPECT(a.call() != 0 && lgs::g_error.find("null") != std::string::npos); }
  { Args a = ok; a.feats = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.labels = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.bank_points = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.bank_colors = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.bank_labels = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.slot_table = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.slot_affines = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.scene_table = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.scene_xforms = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.boxes = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.workspace = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.coords_out = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.feats_out = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.labels_out = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.placement = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.status = nullptr; EXPECT(a.call() != 0); }
  { Args a = ok; a.n = 0; EXPECT(a.call() != 0); }                                       // instances without a scene row
  { Args a = ok; a.n = 0; a.slots = 0; a.inst_rows = 0; EXPECT(a.call() == 0); }         // an empty batch is legal and launches nothing
  std::printf("paste_host_check: ok\n");
  return 0;
}
