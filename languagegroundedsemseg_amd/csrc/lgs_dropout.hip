// lgs_dropout.hip -- RandomDropout on the device: an exact-count uniform row subset per scene, gfx950.
//
// Replaces lib/transforms.py:172-195 and downstream/insseg/datasets/transforms.py:145-159 (np.random.choice(N, int(N * (1 - ratio)),
// replace=False) on one scene's voxel rows).  Row i of scene s gets a 32-bit key, word 0 of a Philox block that is a function of
// (i, seed, scene seed) alone; the scene keeps its k_s = floor(n_s * keep) smallest rows under (key, i), in ascending row order.
// Keys are computed where they are needed and never stored: the selection reads no row data at all.
//
// A TILE is kDropTile consecutive rows of ONE scene (the last tile of a scene is short), so a workgroup never straddles two scenes;
// tile t of the batch is found from the scene offsets alone (at most 33 entries, held in LDS), and the grid is n / kDropTile + b
// workgroups, a bound on the tile count that needs nothing read back.  Launches of one call, in stream order:
//   k_drop_init     per scene n_s, k_s, the mode (keep all / select / keep none) and offsets_out.
//   k_drop_hist     x 3 (digits of 11, 11 and 10 bits from the top): per tile an LDS histogram of the current digit over the rows whose
//                   higher digits equal the scene's prefix; non-zero bins leave by 64-bit integer atomics into the scene's table.
//   k_drop_pick     x 3, one workgroup per scene: the digit at which the running count crosses what is left of k_s joins the prefix.
//                   After the third, prefix = T_s, the k_s-th smallest key, and left = r_s, how many rows with key == T_s are kept.
//   k_drop_count    per tile: rows with key < T_s, rows with key == T_s.
//   k_drop_scan     one workgroup per scene: exclusive scan of both over the scene's tiles -> first output row and first tie rank of
//                   every tile.
//   k_drop_write    per tile: ranks by ballot and popcount in the wave, through LDS across waves; a row is kept if key < T_s, or
//                   key == T_s and its rank among the scene's ties is below r_s; rows_out[j] = through ? through[g] : g.
// No workgroup waits on another inside a launch, every cross-workgroup sum is an integer atomic or a scan with a fixed order, and no
// kernel's result depends on its grid: two calls give the same bits.  Nothing is read back.
#include <algorithm>
#include <cmath>

#include "lgs_common.h"
#include "lgs_philox.h"

namespace lgs {

namespace {

constexpr int kDropScenes = LGS_AUG_MAX_SCENES;
constexpr int kDropBlock = 256;
constexpr int kDropWaves = kDropBlock / 64;
constexpr int kDropIter = kDropTile / kDropBlock;      // rows per thread and tile
constexpr int kDropBins = 1 << 11;
constexpr int kDropBinsPerThread = kDropBins / kDropBlock;
static_assert(kDropTile % kDropBlock == 0 && kDropBins % kDropBlock == 0, "a tile and a histogram are whole rounds of the workgroup");

enum { kKeepAll = 0, kSelect = 1, kKeepNone = 2 };

// the (shift, width) of digit `pass`: 11 + 11 + 10 bits from the top
__host__ __device__ constexpr int digit_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
__host__ __device__ constexpr int digit_bits(int pass) { return pass == 2 ? 10 : 11; }

struct DropScene {          // one per scene, in the workspace
  int64_t left;             // what is left of k_s below the prefix's digits (kSelect: 1 <= k_s < n_s); after the last pick: r_s
  int64_t out0;             // first output row
  uint32_t prefix;          // the digits found so far, in place; after the last pick: T_s
  int32_t mode;
};
static_assert(sizeof(DropScene) == kDropSceneBytes, "dropout_layout sizes the scene records");

struct DropSeeds { uint32_t v[kDropScenes]; };

// the offsets, clamped into a non-decreasing table on [0, n], and the first tile of every scene -> LDS (every workgroup does this)
struct SceneTiles {
  int64_t off[kDropScenes + 1];
  int64_t tile0[kDropScenes + 1];
};
__device__ inline void load_scene_tiles(const int64_t *__restrict__ scene_offsets, int64_t n, int b, SceneTiles &t) {
  if ((int)threadIdx.x <= b) t.off[threadIdx.x] = threadIdx.x == 0 ? 0 : (int)threadIdx.x == b ? n : scene_offsets[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t prev = 0, tiles = 0;
    t.tile0[0] = 0;
    for (int s = 1; s <= b; ++s) {
      const int64_t o = std::min(std::max(t.off[s], prev), n);
      tiles += (o - prev + kDropTile - 1) / kDropTile;
      t.off[s] = o;
      t.tile0[s] = tiles;
      prev = o;
    }
  }
  __syncthreads();
}

// what a tile workgroup knows of its tile
struct TileOf {
  int s;                    // the scene, -1 = this workgroup has no tile
  int64_t first;            // first row of the tile within the scene
  int64_t base;             // first row of the scene in the batch
  int rows;                 // rows of the tile
};
__device__ inline TileOf tile_of(const SceneTiles &t, int b, int64_t tile) {
  TileOf r{-1, 0, 0, 0};
  if (tile >= t.tile0[b]) return r;
  r.s = last_not_above(t.tile0, 1, b, tile);
  r.first = (tile - t.tile0[r.s]) * kDropTile;
  r.base = t.off[r.s];
  r.rows = (int)std::min<int64_t>(kDropTile, t.off[r.s + 1] - r.base - r.first);
  return r;
}

__device__ inline uint32_t drop_key(const int32_t *__restrict__ keys, int64_t g, int64_t i, uint32_t seed_lo, uint32_t seed_hi,
                                    uint32_t scene_seed) {
  if (keys) return (uint32_t)keys[g];
  uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), 0u, (uint32_t)LGS_AUG_STAGE_DROPOUT ^ seed_hi};
  philox4x32_10(c, seed_lo, scene_seed);
  return c[0];
}

__global__ void k_drop_init(const int64_t *__restrict__ scene_offsets, int64_t n, int b, uint32_t apply_mask, double keep,
                            DropScene *__restrict__ scenes, int64_t *__restrict__ offsets_out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t prev = 0, out = 0;
  offsets_out[0] = 0;
  for (int s = 0; s < b; ++s) {
    const int64_t o = s + 1 == b ? n : std::min(std::max(scene_offsets[s + 1], prev), n);
    const int64_t rows = o - prev;
    int64_t k = rows;
    if ((apply_mask >> s) & 1u) k = std::min(std::max((int64_t)floor(__dmul_rn((double)rows, keep)), (int64_t)0), rows);
    DropScene d;
    d.left = k;
    d.out0 = out;
    d.prefix = 0u;
    d.mode = k == rows ? kKeepAll : k == 0 ? kKeepNone : kSelect;
    scenes[s] = d;
    out += k;
    offsets_out[s + 1] = out;
    prev = o;
  }
}

template <int PASS>
__global__ void __launch_bounds__(kDropBlock) k_drop_hist(const int64_t *__restrict__ scene_offsets, int64_t n, int b,
                                                          const DropScene *__restrict__ scenes, const int32_t *__restrict__ keys,
                                                          uint32_t seed_lo, uint32_t seed_hi, DropSeeds seeds,
                                                          unsigned long long *__restrict__ hist) {
  __shared__ SceneTiles tiles;
  __shared__ uint32_t bins[kDropBins];
  load_scene_tiles(scene_offsets, n, b, tiles);
  const TileOf t = tile_of(tiles, b, blockIdx.x);
  if (t.s < 0 || scenes[t.s].mode != kSelect) return;      // block-uniform
  constexpr int shift = digit_shift(PASS), width = digit_bits(PASS), above = shift + width;
  const uint32_t prefix = scenes[t.s].prefix;
  for (int j = threadIdx.x; j < kDropBins; j += kDropBlock) bins[j] = 0u;
  __syncthreads();
#pragma unroll 2
  for (int it = 0; it < kDropIter; ++it) {
    const int li = it * kDropBlock + threadIdx.x;
    if (li < t.rows) {
      const int64_t i = t.first + li;
      const uint32_t key = drop_key(keys, t.base + i, i, seed_lo, seed_hi, seeds.v[t.s]);
      const bool match = above >= 32 || (key >> (above & 31)) == (prefix >> (above & 31));
      if (match) atomicAdd(&bins[(key >> shift) & ((1u << width) - 1u)], 1u);
    }
  }
  __syncthreads();
  unsigned long long *dst = hist + ((int64_t)PASS * b + t.s) * kDropBins;
  for (int j = threadIdx.x; j < kDropBins; j += kDropBlock)
    if (bins[j]) atomicAdd(dst + j, (unsigned long long)bins[j]);
}

// exclusive sum of v over the workgroup's threads in thread order; total = the sum over all of them.  Two barriers.
__device__ inline int64_t block_exclusive(int64_t v, int64_t (&sh)[kDropWaves], int64_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();                 // the previous round's readers are done with sh
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int64_t before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kDropWaves; ++w) {
    if (w < wave) before += sh[w];
    total += sh[w];
  }
  return before + inc - v;
}

template <int PASS>
__global__ void __launch_bounds__(kDropBlock) k_drop_pick(int b, DropScene *__restrict__ scenes,
                                                          const unsigned long long *__restrict__ hist) {
  __shared__ int64_t sh[kDropWaves];
  const int s = blockIdx.x;
  if (s >= b || scenes[s].mode != kSelect) return;
  const int64_t left = scenes[s].left;                     // 1 <= left <= rows under the prefix
  const uint32_t prefix = scenes[s].prefix;
  const unsigned long long *src = hist + ((int64_t)PASS * b + s) * kDropBins + threadIdx.x * kDropBinsPerThread;
  int64_t c[kDropBinsPerThread], mine = 0;
#pragma unroll
  for (int j = 0; j < kDropBinsPerThread; ++j) {
    c[j] = (int64_t)src[j];
    mine += c[j];
  }
  int64_t total;
  int64_t below = block_exclusive(mine, sh, total);      // (its barriers also order every thread's read of the record before the write)
  if (below < left && left <= below + mine) {              // exactly one thread: the bins' running count crosses `left` here
#pragma unroll
    for (int j = 0; j < kDropBinsPerThread; ++j) {
      if (below < left && left <= below + c[j]) {
        scenes[s].prefix = prefix | ((uint32_t)(threadIdx.x * kDropBinsPerThread + j) << digit_shift(PASS));
        scenes[s].left = left - below;
      }
      below += c[j];
    }
  }
}

// which rows of a tile are below the threshold / on it (keep all: every row is below; keep none: no row is either)
__device__ inline void classify(const DropScene &d, uint32_t key, bool valid, bool &lt, bool &eq) {
  lt = valid && (d.mode == kKeepAll || (d.mode == kSelect && key < d.prefix));
  eq = valid && d.mode == kSelect && key == d.prefix;
}

__global__ void __launch_bounds__(kDropBlock) k_drop_count(const int64_t *__restrict__ scene_offsets, int64_t n, int b,
                                                           const DropScene *__restrict__ scenes, const int32_t *__restrict__ keys,
                                                           uint32_t seed_lo, uint32_t seed_hi, DropSeeds seeds,
                                                           int64_t *__restrict__ tile_lt, int64_t *__restrict__ tile_eq) {
  __shared__ SceneTiles tiles;
  __shared__ int sh[2][kDropWaves];
  load_scene_tiles(scene_offsets, n, b, tiles);
  const TileOf t = tile_of(tiles, b, blockIdx.x);
  if (t.s < 0) return;
  const DropScene d = scenes[t.s];
  int n_lt = 0, n_eq = 0;
  if (d.mode == kSelect) {
#pragma unroll 2
    for (int it = 0; it < kDropIter; ++it) {
      const int li = it * kDropBlock + threadIdx.x;
      if (li < t.rows) {
        const int64_t i = t.first + li;
        const uint32_t key = drop_key(keys, t.base + i, i, seed_lo, seed_hi, seeds.v[t.s]);
        n_lt += key < d.prefix;
        n_eq += key == d.prefix;
      }
    }
    n_lt = wave_sum(n_lt);
    n_eq = wave_sum(n_eq);
    if ((threadIdx.x & 63) == 0) {
      sh[0][threadIdx.x >> 6] = n_lt;
      sh[1][threadIdx.x >> 6] = n_eq;
    }
    __syncthreads();
    n_lt = n_eq = 0;
    for (int w = 0; w < kDropWaves; ++w) {
      n_lt += sh[0][w];
      n_eq += sh[1][w];
    }
  } else if (d.mode == kKeepAll) {
    n_lt = t.rows;
  }
  if (threadIdx.x == 0) {
    tile_lt[blockIdx.x] = n_lt;
    tile_eq[blockIdx.x] = n_eq;
  }
}

// in place: (rows below T, rows on T) of every tile -> (first output row, rank of the tile's first tie among the scene's ties)
__global__ void __launch_bounds__(kDropBlock) k_drop_scan(const int64_t *__restrict__ scene_offsets, int64_t n, int b,
                                                          const DropScene *__restrict__ scenes, int64_t *__restrict__ tile_lt,
                                                          int64_t *__restrict__ tile_eq) {
  __shared__ SceneTiles tiles;
  __shared__ int64_t sh[kDropWaves];
  load_scene_tiles(scene_offsets, n, b, tiles);
  const int s = blockIdx.x;
  if (s >= b) return;
  const DropScene d = scenes[s];
  const int64_t r = d.mode == kSelect ? d.left : 0;
  int64_t run_lt = 0, run_eq = 0;
  for (int64_t at = tiles.tile0[s]; at < tiles.tile0[s + 1]; at += kDropBlock) {      // block-uniform trip count
    const int64_t tile = at + threadIdx.x;
    const bool valid = tile < tiles.tile0[s + 1];
    const int64_t lt = valid ? tile_lt[tile] : 0, eq = valid ? tile_eq[tile] : 0;
    int64_t sum_lt, sum_eq;
    const int64_t ex_lt = run_lt + block_exclusive(lt, sh, sum_lt);
    const int64_t ex_eq = run_eq + block_exclusive(eq, sh, sum_eq);
    if (valid) {
      tile_lt[tile] = d.out0 + ex_lt + std::min(ex_eq, r);
      tile_eq[tile] = ex_eq;
    }
    run_lt += sum_lt;
    run_eq += sum_eq;
  }
}

__global__ void __launch_bounds__(kDropBlock) k_drop_write(const int64_t *__restrict__ scene_offsets, int64_t n, int b,
                                                           const DropScene *__restrict__ scenes, const int32_t *__restrict__ keys,
                                                           uint32_t seed_lo, uint32_t seed_hi, DropSeeds seeds,
                                                           const int64_t *__restrict__ tile_out, const int64_t *__restrict__ tile_tie,
                                                           const int64_t *__restrict__ through, int64_t *__restrict__ rows_out) {
  __shared__ SceneTiles tiles;
  __shared__ int sh_eq[kDropWaves], sh_keep[kDropWaves];
  load_scene_tiles(scene_offsets, n, b, tiles);
  const TileOf t = tile_of(tiles, b, blockIdx.x);
  if (t.s < 0) return;
  const DropScene d = scenes[t.s];
  if (d.mode == kKeepNone) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long lower = (1ull << lane) - 1ull;
  const int64_t r = d.mode == kSelect ? d.left : 0;
  int64_t out = tile_out[blockIdx.x], tie = tile_tie[blockIdx.x];
  for (int it = 0; it < kDropIter; ++it) {
    if (it * kDropBlock >= t.rows) break;                   // block-uniform
    const int li = it * kDropBlock + threadIdx.x;
    const bool valid = li < t.rows;
    const int64_t i = t.first + li, g = t.base + i;
    uint32_t key = 0u;
    if (valid && d.mode == kSelect) key = drop_key(keys, g, i, seed_lo, seed_hi, seeds.v[t.s]);
    bool lt, eq;
    classify(d, key, valid, lt, eq);
    // rank of this row among the scene's ties, in row order: lanes of a wave and waves of a workgroup hold ascending rows
    const unsigned long long bal_eq = __ballot(eq);
    if (lane == 0) sh_eq[wave] = __popcll(bal_eq);
    __syncthreads();
    int64_t tie_rank = tie + __popcll(bal_eq & lower);
    int ties = 0;
#pragma unroll
    for (int w = 0; w < kDropWaves; ++w) {
      if (w < wave) tie_rank += sh_eq[w];
      ties += sh_eq[w];
    }
    const bool kept = lt || (eq && tie_rank < r);
    const unsigned long long bal_keep = __ballot(kept);
    if (lane == 0) sh_keep[wave] = __popcll(bal_keep);
    __syncthreads();
    int64_t at = out + __popcll(bal_keep & lower);
    int kept_all = 0;
#pragma unroll
    for (int w = 0; w < kDropWaves; ++w) {
      if (w < wave) at += sh_keep[w];
      kept_all += sh_keep[w];
    }
    if (kept && at >= 0 && at < n) rows_out[at] = through ? through[g] : g;
    out += kept_all;
    tie += ties;
  }
}

inline bool drop_shape_ok(int64_t n, int b) { return n >= 0 && n <= kDropMaxRows && b >= 1 && b <= kDropScenes; }

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_dropout_workspace_bytes(int64_t n, int b) {
  if (!drop_shape_ok(n, b)) return 0;
  return dropout_layout(n, b).total;
}

int lgs_dropout_select(const int64_t *scene_offsets, int64_t n, int b, unsigned int apply_mask, double keep, int64_t seed,
                       const int32_t *scene_seeds, const int32_t *keys, const int64_t *through, void *workspace, int64_t *rows_out,
                       int64_t *offsets_out, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kDropScenes, "lgs_dropout_select: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(keep > 0.0 && keep <= 1.0, "lgs_dropout_select: keep must lie in (0, 1]");
  LGS_REQUIRE(drop_shape_ok(n, b) && scene_offsets && workspace && offsets_out && (n == 0 || rows_out),
              "lgs_dropout_select: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const DropoutWs w = dropout_layout(n, b);
  DropScene *scenes = Layout::at<DropScene>(workspace, w.scenes);
  unsigned long long *hist = Layout::at<unsigned long long>(workspace, w.hist);
  int64_t *tile_lt = Layout::at<int64_t>(workspace, w.tile_lt), *tile_eq = Layout::at<int64_t>(workspace, w.tile_eq);
  const uint32_t mask = b == 32 ? apply_mask : apply_mask & ((1u << b) - 1u);
  LGS_KLAUNCH(k_drop_init, 1, 64, 0, s, scene_offsets, n, b, mask, keep, scenes, offsets_out);
  if (n > 0) {
    DropSeeds seeds;
    for (int i = 0; i < kDropScenes; ++i) seeds.v[i] = (scene_seeds && i < b) ? (uint32_t)scene_seeds[i] : 0u;
    const uint32_t lo = (uint32_t)seed, hi = (uint32_t)((uint64_t)seed >> 32);
    const unsigned tiles = (unsigned)w.tiles;
    if (mask && keep < 1.0) {        // else every scene keeps all of its rows: nothing to select
      LGS_HIP(hipMemsetAsync(hist, 0, (size_t)(w.tile_lt - w.hist), s));
      LGS_KLAUNCH(k_drop_hist<0>, tiles, kDropBlock, 0, s, scene_offsets, n, b, scenes, keys, lo, hi, seeds, hist);
      LGS_KLAUNCH(k_drop_pick<0>, b, kDropBlock, 0, s, b, scenes, hist);
      LGS_KLAUNCH(k_drop_hist<1>, tiles, kDropBlock, 0, s, scene_offsets, n, b, scenes, keys, lo, hi, seeds, hist);
      LGS_KLAUNCH(k_drop_pick<1>, b, kDropBlock, 0, s, b, scenes, hist);
      LGS_KLAUNCH(k_drop_hist<2>, tiles, kDropBlock, 0, s, scene_offsets, n, b, scenes, keys, lo, hi, seeds, hist);
      LGS_KLAUNCH(k_drop_pick<2>, b, kDropBlock, 0, s, b, scenes, hist);
    }
    LGS_KLAUNCH(k_drop_count, tiles, kDropBlock, 0, s, scene_offsets, n, b, scenes, keys, lo, hi, seeds, tile_lt, tile_eq);
    LGS_KLAUNCH(k_drop_scan, b, kDropBlock, 0, s, scene_offsets, n, b, scenes, tile_lt, tile_eq);
    LGS_KLAUNCH(k_drop_write, tiles, kDropBlock, 0, s, scene_offsets, n, b, scenes, keys, lo, hi, seeds, tile_lt, tile_eq, through,
                rows_out);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
