// lgs_paste.hip -- class-balanced tail-instance paste on the device, gfx950 (the reference's --sample_tail_instances).
//
// Replaces ScannetVoxelizationDataset.add_instances_to_cloud (lib/datasets/scannet.py:143-241), which runs per scene on one
// DataLoader core: a Python loop per voxel for the height map, a 5 x 5 maximum filter, up to 50 sequential placement trials per
// instance with a Python loop of box tests each, a concatenate, a rotation and a second dedup.  Here a batch is b <= 32 scenes of
// int32 [n, 4] voxel rows (scene id in column 0), and a "slot" is one (scene, instance) pair, at most 1024 of them; the rows of all
// slots' instances form one concatenated range of inst_rows rows.  Every host decision arrives in device tables (lgs_engine.h).
// Integer atomics only: two calls give the same bits.  Nothing is read back.
//
//   k_paste_init      voxel table, per-slot statistics and per-scene flags to their neutral values.
//   k_paste_map_init  per scene: the height map [dim_x, dim_y] = z_min; a map of more than max_map_cells cells flags the scene.
//   k_paste_height    one scene row per thread: atomicMax of z into its map cell.
//   k_paste_voxelize  one instance row per thread: floor(M p) with k_voxelize_batched's arithmetic, then the voxel is claimed in an
//                     open-addressing table keyed by (slot, x, y, z): 64-bit compare-and-swap on the key, atomicMin of the row index.
//   k_paste_stats     a row is "first" iff it holds its voxel's minimum; over first rows per slot: min, max, int64 sum, count.
//                     Reduced in the wave by shuffles, one set of atomics per wave and slot.
//   k_paste_place     one wave per slot, lane t = trial t (chunks of 64, the first chunk with a hit wins): the clamped 5 x 5 max of
//                     the height map at the trial's cell, the float64 box tests against the scene's boxes (wave-uniform loads),
//                     ballot + find-first.
//   k_paste_write     every output row = floor(M_r c): scene rows as they are, instance rows c = voxel - mean + centroid; features
//                     and labels alongside.  Instance rows of a flagged scene are copies of the scene's first row.
#include <algorithm>
#include <climits>
#include <cmath>

#include "lgs_common.h"
#include "lgs_keypack.h"
#include "lgs_philox.h"

namespace lgs {

namespace {

constexpr int kPasteBlock = 256;
constexpr int kPasteScenes = LGS_AUG_MAX_SCENES;
constexpr int kMapBlocks = 64;                  // grid.x of k_paste_map_init (it loops over the scene's cells)

struct SlotStats {                              // 64 bytes
  int32_t mn[3], count;
  int32_t mx[3], pad;
  unsigned long long sum[3], pad64;             // two's-complement sums of signed coordinates
};
static_assert(sizeof(SlotStats) == kPasteStatsBytes, "paste_layout (lgs_idioms.h) sizes the statistics at 64 bytes per slot");

constexpr int kSlotCols = LGS_PASTE_SLOT_COLS, kSceneCols = LGS_PASTE_SCENE_COLS;
enum { kSlotBank = 0, kSlotFirst = 1, kSlotOut = 2, kSlotScene = 3, kSlotIndex = 4, kSlotRows = 5 };      // columns of slot_table
enum { kSceneOut = 0, kSceneBox = 1, kSceneSeed = 2, kSceneFirst = 3 };                                   // columns of scene_table

// the slot of an instance row (every slot has at least one row), the scene of a scene row
__device__ inline int slot_of(const int64_t *__restrict__ slot_table, int slots, int64_t r) { return last_not_above(slot_table + kSlotFirst, kSlotCols, slots, r); }
__device__ inline int scene_of_row(const int64_t *__restrict__ scene_table, int b, int64_t i) { return last_not_above(scene_table + kSceneFirst, kSceneCols, b, i); }
// the tables are the caller's: a scene id is clamped before it indexes anything
__device__ inline int slot_scene(const int64_t *__restrict__ slot_table, int slot, int b) {
  return (int)std::min<int64_t>(std::max<int64_t>(slot_table[kSlotCols * slot + kSlotScene], 0), b - 1);
}

// a scene's map: its dimensions from the bounds; false for an empty scene
__device__ inline bool map_dims(const int32_t *__restrict__ bnd, int64_t &dx, int64_t &dy) {
  if (bnd[0] > bnd[3]) return false;
  dx = (int64_t)bnd[3] - bnd[0] + 1;
  dy = (int64_t)bnd[4] - bnd[1] + 1;
  return true;
}
__device__ inline bool map_fits(int64_t dx, int64_t dy, int64_t max_map_cells) {
  return dx <= max_map_cells && dy <= max_map_cells && dx * dy <= max_map_cells;
}

__global__ void __launch_bounds__(kPasteBlock) k_paste_init(uint64_t *__restrict__ hkeys, int32_t *__restrict__ hmin, int64_t cap,
                                                            SlotStats *__restrict__ stats, int slots, int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * kPasteBlock + threadIdx.x;
  if (i < cap) {
    hkeys[i] = kEmpty;
    hmin[i] = INT_MAX;
  }
  if (i < slots) {
    SlotStats s;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s.mn[a] = INT_MAX;
      s.mx[a] = INT_MIN;
      s.sum[a] = 0ull;
    }
    s.count = 0;
    s.pad = 0;
    s.pad64 = 0ull;
    stats[i] = s;
  }
  if (i < kPasteScenes) flags[i] = 0;
}

__global__ void __launch_bounds__(kPasteBlock) k_paste_map_init(const int32_t *__restrict__ bounds, int b, int64_t max_map_cells,
                                                                int32_t *__restrict__ maps, int32_t *__restrict__ flags,
                                                                int32_t *__restrict__ status) {
  const int s = blockIdx.y;
  int64_t dx, dy;
  if (s >= b || !map_dims(bounds + s * 6, dx, dy)) return;
  if (!map_fits(dx, dy, max_map_cells)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      atomicOr(flags + s, 1);
      atomicOr(status, (int32_t)(1u << s));
    }
    return;
  }
  const int32_t z_min = bounds[s * 6 + 2];
  int32_t *map = maps + (int64_t)s * max_map_cells;
  for (int64_t c = (int64_t)blockIdx.x * kPasteBlock + threadIdx.x; c < dx * dy; c += (int64_t)gridDim.x * kPasteBlock) map[c] = z_min;
}

__global__ void __launch_bounds__(kPasteBlock) k_paste_height(const int32_t *__restrict__ coords, int64_t n,
                                                              const int64_t *__restrict__ scene_table, int b, const int32_t *__restrict__ bounds, int64_t max_map_cells,
                                                              int32_t *__restrict__ maps) {
  const int64_t i = (int64_t)blockIdx.x * kPasteBlock + threadIdx.x;
  if (i >= n) return;
  const int s = scene_of_row(scene_table, b, i);
  const int32_t *bnd = bounds + s * 6;
  int64_t dx, dy;
  if (!map_dims(bnd, dx, dy) || !map_fits(dx, dy, max_map_cells)) return;
  const int4 c = reinterpret_cast<const int4 *>(coords)[i];
  // the bounds are taken by the scene id in column 0, the scene here by the caller's offsets: where the two disagree the cell may
  // lie outside the map, and such a row is left out
  const int64_t ix = (int64_t)c.y - bnd[0], iy = (int64_t)c.z - bnd[1];
  if (ix < 0 || ix >= dx || iy < 0 || iy >= dy) return;
  // one atomic per row.  Reading the cell first and skipping rows that are not above it was measured and is slower (355 us against
  // 126 us on the 8-scene batch): the read misses where the atomic, executed at the memory side, does not wait
  atomicMax(maps + (int64_t)s * max_map_cells + ix * dy + iy, c.w);
}

__global__ void __launch_bounds__(kPasteBlock) k_paste_voxelize(const float *__restrict__ bank_points, int64_t bank_rows,
                                                                const int64_t *__restrict__ slot_table,
                                                                const double *__restrict__ slot_affines, int slots, int64_t inst_rows, int b,
                                                                uint64_t *__restrict__ hkeys, int32_t *__restrict__ hmin, uint64_t capm1,
                                                                int32_t *__restrict__ hslot, int32_t *__restrict__ ivox,
                                                                int32_t *__restrict__ flags, int32_t *__restrict__ status) {
  const int64_t r = (int64_t)blockIdx.x * kPasteBlock + threadIdx.x;
  if (r >= inst_rows) return;
  const int slot = slot_of(slot_table, slots, r);
  const int64_t src = slot_table[kSlotCols * slot + kSlotBank] + (r - slot_table[kSlotCols * slot + kSlotFirst]);
  bool in_range = src >= 0 && src < bank_rows;
  int32_t v[3] = {0, 0, 0};
  if (in_range) {
    const double x = (double)bank_points[3 * src], y = (double)bank_points[3 * src + 1], z = (double)bank_points[3 * src + 2];
    const double *a = slot_affines + 12 * slot;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double f = floor(affine_row(a + 4 * k, x, y, z));
      in_range = in_range && f >= (double)-kBias && f < (double)kBias;      // also NaN
      v[k] = in_range ? (int32_t)f : 0;
    }
  }
  reinterpret_cast<int4 *>(ivox)[r] = make_int4(slot, v[0], v[1], v[2]);
  if (!in_range) {                              // outside the 18-bit key range (or the bank): the scene passes through unpasted
    const int s = slot_scene(slot_table, slot, b);
    atomicOr(flags + s, 2);
    atomicOr(status, (int32_t)(1u << s));
    hslot[r] = -1;
    return;
  }
  const uint64_t key = pack_key(slot, v[0] + kBias, v[1] + kBias, v[2] + kBias);
  const int64_t at = table_claim(hkeys, hash64(key) & capm1, capm1, key, kEmpty, capm1 + 1);      // the table holds at least twice the rows
  if (at >= 0) atomicMin(hmin + at, (int32_t)r);
  hslot[r] = (int32_t)at;
}

__global__ void __launch_bounds__(kPasteBlock) k_paste_stats(const int64_t *__restrict__ slot_table, int slots, int64_t inst_rows,
                                                             const int32_t *__restrict__ hmin, const int32_t *__restrict__ hslot,
                                                             const int32_t *__restrict__ ivox, SlotStats *__restrict__ stats) {
  const int64_t r = (int64_t)blockIdx.x * kPasteBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t wave_first = r - lane;
  if (wave_first >= inst_rows) return;                       // wave-uniform
  const bool valid = r < inst_rows;
  int my_slot = -1;
  bool first = false;
  int4 v = make_int4(0, 0, 0, 0);
  if (valid) {
    v = reinterpret_cast<const int4 *>(ivox)[r];
    my_slot = v.x;
    const int32_t at = hslot[r];
    first = at >= 0 && hmin[at] == (int32_t)r;
  }
  const int s_first = slot_of(slot_table, slots, wave_first);
  const int s_last = slot_of(slot_table, slots, std::min<int64_t>(wave_first + 63, inst_rows - 1));
  for (int s = s_first; s <= s_last; ++s) {
    const bool mine = first && my_slot == s;
    int32_t mn[3], mx[3];
    long long sm[3];
    const int32_t cnt = wave_sum(mine ? 1 : 0);
    const int32_t c[3] = {v.y, v.z, v.w};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = wave_min(mine ? c[a] : INT_MAX);
      mx[a] = wave_max(mine ? c[a] : INT_MIN);
      sm[a] = wave_sum(mine ? (long long)c[a] : 0ll);
    }
    if (lane == 0 && cnt > 0) {
      SlotStats *q = stats + s;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(q->mn + a, mn[a]);
        atomicMax(q->mx + a, mx[a]);
        atomicAdd(q->sum + a, (unsigned long long)sm[a]);
      }
      atomicAdd(&q->count, cnt);
    }
  }
}

// place[slot] = (trial, cx - mean_x, cy - mean_y, cz - mean_z) for k_paste_write; placement[slot] = (trial, cx, cy, cz) for the caller.
// trial = the first trial without an intersection, `trials` if all intersect (the last trial's centroid is used), -1 = not pasted.
__global__ void __launch_bounds__(64) k_paste_place(const int64_t *__restrict__ slot_table, int slots, const int64_t *__restrict__ scene_table,
                                                    int b, const double *__restrict__ scene_xforms, const double *__restrict__ boxes,
                                                    int64_t n_boxes,
                                                    const int32_t *__restrict__ bounds, const int32_t *__restrict__ flags,
                                                    const SlotStats *__restrict__ stats, const int32_t *__restrict__ maps,
                                                    int64_t max_map_cells, const int32_t *__restrict__ trial_draws, int trials,
                                                    uint32_t seed_lo, uint32_t seed_hi, int32_t *__restrict__ place,
                                                    int32_t *__restrict__ placement) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  if (slot >= slots) return;
  const int s = slot_scene(slot_table, slot, b);
  const SlotStats st = stats[slot];
  const int32_t *bnd = bounds + s * 6;
  int64_t dx = 0, dy = 0;
  if (flags[s] != 0 || st.count <= 0 || !map_dims(bnd, dx, dy) || !map_fits(dx, dy, max_map_cells)) {
    if (lane < 4) place[4 * slot + lane] = placement[4 * slot + lane] = lane == 0 ? -1 : 0;
    return;
  }
  const int32_t x_min = bnd[0], y_min = bnd[1];
  const int32_t *map = maps + (int64_t)s * max_map_cells;
  const double scale = scene_xforms[13 * s];
  const int64_t box0 = std::max<int64_t>(scene_table[kSceneCols * s + kSceneBox], 0);
  const int64_t box1 = std::min<int64_t>(scene_table[kSceneCols * (s + 1) + kSceneBox], n_boxes);
  const uint32_t scene_seed = (uint32_t)scene_table[kSceneCols * s + kSceneSeed];
  const uint32_t k = (uint32_t)slot_table[kSlotCols * slot + kSlotIndex];      // the instance's index within its scene
  double half[3];
  int32_t mean[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    half[a] = (double)(st.mx[a] - st.mn[a] + 1) / 2.0;
    mean[a] = (int32_t)((double)(long long)st.sum[a] / (double)st.count);      // C truncation, as numpy's astype(int)
  }
  int32_t win_trial = trials, win[3] = {0, 0, 0};
  for (int t0 = 0; t0 < trials; t0 += 64) {
    const int t = t0 + lane;
    const bool live = t < trials;
    int32_t c[3] = {x_min, y_min, 0};
    bool ok = false;
    if (live) {
      if (trial_draws) {                        // teacher-forced; clamped into the scene so that the map read stays inside it
        c[0] = trial_draws[((int64_t)slot * trials + t) * 2];
        c[1] = trial_draws[((int64_t)slot * trials + t) * 2 + 1];
        c[0] = (int32_t)std::min<int64_t>(std::max<int64_t>(c[0], x_min), x_min + dx - 1);
        c[1] = (int32_t)std::min<int64_t>(std::max<int64_t>(c[1], y_min), y_min + dy - 1);
      } else {
        uint32_t w[4] = {(uint32_t)t, k, (uint32_t)LGS_AUG_STAGE_PASTE, seed_hi};
        philox4x32_10(w, seed_lo, scene_seed);
        c[0] = x_min + (int32_t)(((uint64_t)w[0] * (uint64_t)dx) >> 32);       // dx, dy <= max_map_cells <= 2^26
        c[1] = y_min + (int32_t)(((uint64_t)w[1] * (uint64_t)dy) >> 32);
      }
      // maximum_filter(size = 5) with the reflect boundary at one cell = the max over the 5 x 5 window clamped to the map
      const int64_t ix = (int64_t)c[0] - x_min, iy = (int64_t)c[1] - y_min;
      int32_t h = INT_MIN;
      for (int64_t jx = std::max<int64_t>(ix - 2, 0); jx <= std::min<int64_t>(ix + 2, dx - 1); ++jx)
        for (int64_t jy = std::max<int64_t>(iy - 2, 0); jy <= std::min<int64_t>(iy + 2, dy - 1); ++jy) h = std::max(h, map[jx * dy + jy]);
      c[2] = (int32_t)((double)h + half[2]);    // int(height + dims_z / 2.)
      double lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        lo[a] = (double)c[a] - half[a];
        hi[a] = (double)c[a] + half[a];
      }
      ok = true;
      for (int64_t j = box0; j < box1; ++j) {   // j and the box are wave-uniform
        const double *q = boxes + 6 * j;
        bool hit = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) hit = hit && __dmul_rn(q[a], scale) <= hi[a] && __dmul_rn(q[3 + a], scale) >= lo[a];
        if (hit) ok = false;
      }
    }
    const unsigned long long hits = __ballot(ok);
    const int src = hits ? __ffsll((long long)hits) - 1 : std::min(63, trials - 1 - t0);      // else this chunk's last live trial
#pragma unroll
    for (int a = 0; a < 3; ++a) win[a] = __shfl(c[a], src, 64);
    if (hits) {
      win_trial = t0 + src;
      break;
    }
  }
  if (lane < 4) {
    placement[4 * slot + lane] = lane == 0 ? win_trial : win[lane - 1];
    place[4 * slot + lane] = lane == 0 ? win_trial : win[lane - 1] - mean[lane - 1];
  }
}

__global__ void __launch_bounds__(kPasteBlock) k_paste_write(const int32_t *__restrict__ coords, const float *__restrict__ feats,
                                                             const int64_t *__restrict__ labels, int64_t n, int b,
                                                             const float *__restrict__ bank_colors,
                                                             const int64_t *__restrict__ bank_labels, const int64_t *__restrict__ slot_table,
                                                             int slots, int64_t inst_rows, const int64_t *__restrict__ scene_table,
                                                             const double *__restrict__ scene_xforms, const int32_t *__restrict__ flags,
                                                             const int32_t *__restrict__ place, const int32_t *__restrict__ ivox,
                                                             int32_t *__restrict__ coords_out, float *__restrict__ feats_out,
                                                             int64_t *__restrict__ labels_out) {
  const int64_t i = (int64_t)blockIdx.x * kPasteBlock + threadIdx.x;
  if (i >= n + inst_rows) return;
  int s;
  int64_t dst, src_scene = -1, src_bank = -1;      // exactly one source is set
  int32_t c[3];
  if (i < n) {
    s = scene_of_row(scene_table, b, i);
    dst = scene_table[kSceneCols * s + kSceneOut] + (i - scene_table[kSceneCols * s + kSceneFirst]);
    src_scene = i;
  } else {
    const int64_t r = i - n;
    const int slot = slot_of(slot_table, slots, r);
    const int64_t *rec = slot_table + kSlotCols * slot;
    s = slot_scene(slot_table, slot, b);
    dst = rec[kSlotOut] + (r - rec[kSlotFirst]);
    const int32_t trial = place[4 * slot];
    if (flags[s] != 0 || trial < 0) {              // a flagged scene: copies of its first row, which the dedup drops
      src_scene = std::min<int64_t>(std::max<int64_t>(scene_table[kSceneCols * s + kSceneFirst], 0), n - 1);
    } else {
      src_bank = rec[kSlotBank] + (r - rec[kSlotFirst]);
      const int4 v = reinterpret_cast<const int4 *>(ivox)[r];
      c[0] = v.y + place[4 * slot + 1];
      c[1] = v.z + place[4 * slot + 2];
      c[2] = v.w + place[4 * slot + 3];
    }
  }
  if (dst < 0 || dst >= n + inst_rows) return;      // the tables are the caller's
  if (src_scene >= 0) {
    const int4 v = reinterpret_cast<const int4 *>(coords)[src_scene];
    c[0] = v.y;
    c[1] = v.z;
    c[2] = v.w;
  }
  const double *m = scene_xforms + 13 * s + 1;
  const double x = (double)c[0], y = (double)c[1], z = (double)c[2];
  reinterpret_cast<int4 *>(coords_out)[dst] = make_int4(s, (int32_t)floor(affine_row(m, x, y, z)), (int32_t)floor(affine_row(m + 4, x, y, z)),
                                                        (int32_t)floor(affine_row(m + 8, x, y, z)));
  const float *f = src_scene >= 0 ? feats + 3 * src_scene : bank_colors + 3 * src_bank;
#pragma unroll
  for (int k = 0; k < 3; ++k) feats_out[3 * dst + k] = f[k];
  labels_out[dst] = src_scene >= 0 ? labels[src_scene] : bank_labels[src_bank];
}

inline unsigned paste_blocks(int64_t n) { return (unsigned)((n + kPasteBlock - 1) / kPasteBlock); }
inline bool paste_rows_fit(int64_t n) { return n >= 0 && n < (1ll << 31) - kPasteBlock; }      // row indices are int32 in the voxel table
inline bool paste_shape_ok(int b, int slots, int64_t inst_rows, int64_t max_map_cells) {
  return b >= 1 && b <= kPasteScenes && slots >= 0 && slots <= LGS_PASTE_MAX_SLOTS && paste_rows_fit(inst_rows) &&
         (slots == 0) == (inst_rows == 0) && inst_rows >= slots && max_map_cells >= 1 && max_map_cells <= (1ll << 26);
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_paste_workspace_bytes(int b, int slots, int64_t inst_rows, int64_t max_map_cells) {
  if (!paste_shape_ok(b, slots, inst_rows, max_map_cells)) return 0;
  return paste_layout(b, slots, inst_rows, max_map_cells).total;
}

int lgs_paste_instances(const int32_t *coords, const float *feats, const int64_t *labels, int64_t n, int b, const float *bank_points,
                        const float *bank_colors, const int64_t *bank_labels, int64_t bank_rows, const int64_t *slot_table,
                        const double *slot_affines, int slots, int64_t inst_rows, const int64_t *scene_table,
                        const double *scene_xforms, const double *boxes, int64_t n_boxes, const int32_t *trial_draws, int trials, int64_t seed, int64_t max_map_cells, void *workspace,
                        int32_t *coords_out, float *feats_out, int64_t *labels_out, int32_t *placement, int32_t *status, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kPasteScenes, "lgs_paste_instances: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(slots >= 0 && slots <= LGS_PASTE_MAX_SLOTS, "lgs_paste_instances: at most LGS_PASTE_MAX_SLOTS (scene, instance) slots per call");
  LGS_REQUIRE(paste_shape_ok(b, slots, inst_rows, max_map_cells), "lgs_paste_instances: bad slots / inst_rows / max_map_cells");
  LGS_REQUIRE(trials >= 1 && trials <= (1 << 20), "lgs_paste_instances: 1 <= trials <= 2^20");
  LGS_REQUIRE(paste_rows_fit(n) && paste_rows_fit(n + inst_rows), "lgs_paste_instances: too many rows");
  LGS_REQUIRE(scene_table && scene_xforms && workspace && status && (n == 0 || (coords && feats && labels)) &&
                  (n + inst_rows == 0 || (coords_out && feats_out && labels_out)),
              "lgs_paste_instances: null argument");
  LGS_REQUIRE(slots == 0 || (bank_points && bank_colors && bank_labels && bank_rows > 0 && slot_table && slot_affines && placement),
              "lgs_paste_instances: null bank / slot argument");
  LGS_REQUIRE(n_boxes >= 0 && (n_boxes == 0 || boxes), "lgs_paste_instances: null boxes");
  LGS_REQUIRE(slots == 0 || n > 0, "lgs_paste_instances: instances need a scene with rows");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const PasteWs w = paste_layout(b, slots, inst_rows, max_map_cells);
  int64_t *off = Layout::at<int64_t>(workspace, w.off);
  int32_t *bounds = Layout::at<int32_t>(workspace, w.bounds), *flags = Layout::at<int32_t>(workspace, w.flags);
  SlotStats *stats = Layout::at<SlotStats>(workspace, w.stats);
  int32_t *place = Layout::at<int32_t>(workspace, w.place);
  uint64_t *hkeys = Layout::at<uint64_t>(workspace, w.hkeys);
  int32_t *hmin = Layout::at<int32_t>(workspace, w.hmin), *hslot = Layout::at<int32_t>(workspace, w.hslot);
  int32_t *ivox = Layout::at<int32_t>(workspace, w.ivox), *maps = Layout::at<int32_t>(workspace, w.maps);
  const int64_t init_n = slots ? std::max<int64_t>(w.cap, kPasteScenes) : kPasteScenes;
  LGS_KLAUNCH(k_paste_init, paste_blocks(init_n), kPasteBlock, 0, s, hkeys, hmin, slots ? w.cap : 0, stats, slots, flags);
  if (slots) {
    if (int rc = lgs_aug_bounds(coords, n, LGS_AUG_I32X4, off, b, bounds, stream)) return rc;
    LGS_KLAUNCH(k_paste_map_init, dim3(kMapBlocks, b), kPasteBlock, 0, s, bounds, b, max_map_cells, maps, flags, status);
    LGS_KLAUNCH(k_paste_height, paste_blocks(n), kPasteBlock, 0, s, coords, n, scene_table, b, bounds, max_map_cells, maps);
    LGS_KLAUNCH(k_paste_voxelize, paste_blocks(inst_rows), kPasteBlock, 0, s, bank_points, bank_rows, slot_table, slot_affines, slots, inst_rows, b,
                hkeys, hmin, (uint64_t)(w.cap - 1), hslot, ivox, flags, status);
    LGS_KLAUNCH(k_paste_stats, paste_blocks(inst_rows), kPasteBlock, 0, s, slot_table, slots, inst_rows, hmin, hslot, ivox, stats);
    LGS_KLAUNCH(k_paste_place, slots, 64, 0, s, slot_table, slots, scene_table, b, scene_xforms, boxes, n_boxes, bounds, flags, stats, maps,
                max_map_cells, trial_draws, trials, (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), place, placement);
  }
  LGS_KLAUNCH(k_paste_write, paste_blocks(n + inst_rows), kPasteBlock, 0, s, coords, feats, labels, n, b, bank_colors, bank_labels,
              slot_table, slots, inst_rows, scene_table, scene_xforms, flags, place, ivox, coords_out, feats_out, labels_out);
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
