// lgs_augment.hip -- the reference's train-time augmentation chain on the device, gfx950.
//
// Replaces the numpy / scipy transforms of lib/transforms.py that lib/dataset.py:355-389 runs in DataLoader workers:
//   ElasticDistortion (:223-258) before the voxeliser, the voxeliser's per-scene rigid matrix (lib/voxelizer.py:44-74,136-139),
//   RandomHorizontalFlip (:198-220), ChromaticAutoContrast (:42-68), ChromaticTranslation (:22-39), ChromaticJitter (:71-84),
//   ChromaticScale (:87-99) after it.  A batch is b <= 32 scenes concatenated, rows of a scene contiguous, scene_offsets[b + 1] on
//   the device; a row finds its scene by a binary search of that table (5 steps).  No kernel reads anything back to the host.
//
//   k_aug_bounds         per-scene min / max of three columns.  One row per thread (three 4-byte loads of a 12-byte row: a wave
//                        reads 768 contiguous bytes, every cache line whole), wave reduce by shuffles, workgroup reduce in LDS, then
//                        one atomicMin / atomicMax per workgroup, scene and column on order-preserving 32-bit keys.
//   k_elastic_noise      N(0, 1) per (cell, component) of every scene's grid, Philox counter = (cell, component, stage, seed hi),
//                        key = (seed lo, scene seed).  Grid dimensions come from the bounds on the device.
//   k_elastic_field      T^2 per axis (two rounds of zero-padded 3-tap box blurs = weights count(i, j) / 9), one 125-tap pass with the
//                        integer weight cx cy cz accumulated in fp32 and one division by 729.
//   k_elastic_apply      per point: trilinear sample in double, p += sample * magnitude, one rounding; the displaced cloud's bounds
//                        leave through the same workgroup reduce as k_aug_bounds.
//   k_voxelize_batched   k_voxelize with a by-value table of affines.
//   k_coords_flip_shift  c = max - c per (scene, axis) flag, then + shift.
//   k_color_augment      autocontrast, translation, jitter, scale, normalise in double: one read, one rounding, one write per row.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "lgs_common.h"
#include "lgs_philox.h"

namespace lgs {

namespace {

constexpr int kAugScenes = LGS_AUG_MAX_SCENES;
constexpr int kAugBlock = 256;
constexpr int kAugWaves = kAugBlock / 64;
constexpr int kFieldBlocks = 64;              // grid.x of the per-scene grid kernels (they loop over the scene's cells)
constexpr uint32_t kKeyPosInf = 0xFF800000u;  // ord_key(+inf)
constexpr uint32_t kKeyNegInf = 0x007FFFFFu;  // ord_key(-inf)

__device__ inline int scene_of(const int64_t *__restrict__ off, int b, int64_t i) { return last_not_above(off, 1, b, i); }   // of row i

struct SceneSeeds { uint32_t v[kAugScenes]; };
struct AffineTable { double a[kAugScenes][12]; };
struct FlipTable { uint8_t axes[kAugScenes]; int32_t shift[3]; };
struct ColorTable { lgs_color_scene s[kAugScenes]; };

// ---- bounds
__global__ void k_aug_bounds_init(uint32_t *__restrict__ kb, int b, int is_float) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= b * 6) return;
  const bool is_min = (t % 6) < 3;
  kb[t] = is_float ? (is_min ? kKeyPosInf : kKeyNegInf) : (is_min ? 0xFFFFFFFFu : 0u);
}
__global__ void k_aug_bounds_decode(uint32_t *__restrict__ kb, int b, int is_float) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= b * 6) return;
  const uint32_t k = kb[t];
  kb[t] = is_float ? __float_as_uint(ord_key_inv(k)) : (uint32_t)ikey_inv(k);
}

// scene_offsets[b + 1] from the ascending scene ids in column 0 of coords[n, 4]; ids are clamped to [0, b)
__global__ void k_aug_scene_offsets(const int32_t *__restrict__ coords, int64_t n, int b, int64_t *__restrict__ off) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = std::min(std::max(coords[4 * i], 0), b - 1);
  const int prev = i == 0 ? -1 : std::min(std::max(coords[4 * (i - 1)], 0), b - 1);
  for (int s = prev + 1; s <= t; ++s) off[s] = i;
  if (i == n - 1)
    for (int s = t + 1; s <= b; ++s) off[s] = n;
}

// keys lo[3] / hi[3] of this thread's row (valid = it has one, of scene my_scene) -> kb[b, 6]; the block's rows lie in scenes
// s_first .. s_last (block-uniform).  One atomic per workgroup, scene and column; a scene without rows in the block issues none.
__device__ inline void block_bounds_commit(const uint32_t (&lo)[3], const uint32_t (&hi)[3], bool valid, int my_scene, int s_first,
                                           int s_last, uint32_t *__restrict__ kb) {
  __shared__ uint32_t sh[kAugWaves][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = s_first; s <= s_last; ++s) {
    const bool mine = valid && my_scene == s;
    uint32_t v[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = wave_min(mine ? lo[c] : 0xFFFFFFFFu);
      v[3 + c] = wave_max(mine ? hi[c] : 0u);
    }
    if (lane == 0) {
#pragma unroll
      for (int j = 0; j < 6; ++j) sh[wave][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
      const int j = threadIdx.x;
      uint32_t r = sh[0][j];
      for (int w = 1; w < kAugWaves; ++w) r = j < 3 ? std::min(r, sh[w][j]) : std::max(r, sh[w][j]);
      if (j < 3) {
        if (r != 0xFFFFFFFFu) atomicMin(kb + s * 6 + j, r);
      } else {
        if (r != 0u) atomicMax(kb + s * 6 + j, r);
      }
    }
    __syncthreads();
  }
}

template <bool F32>
__global__ void __launch_bounds__(kAugBlock) k_aug_bounds(const void *__restrict__ table, int64_t n, const int64_t *__restrict__ off, int b,
                                                          uint32_t *__restrict__ kb) {
  const int64_t base = (int64_t)blockIdx.x * kAugBlock, i = base + threadIdx.x;
  const int s_first = scene_of(off, b, base), s_last = scene_of(off, b, std::min<int64_t>(base + kAugBlock - 1, n - 1));
  const bool valid = i < n;
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  int my_scene = -1;
  if (valid) {
    my_scene = scene_of(off, b, i);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = F32 ? ord_key(static_cast<const float *>(table)[3 * i + c]) : ikey(static_cast<const int32_t *>(table)[4 * i + 1 + c]);
      hi[c] = lo[c];
    }
  }
  block_bounds_commit(lo, hi, valid, my_scene, s_first, s_last, kb);
}

// ---- elastic distortion
// numpy's floor_divide on float32 (npy_divmodf), a >= 0, b > 0
__device__ inline float npy_floor_divide(float a, float b) {
  float mod = fmodf(a, b);
  float div = __fdiv_rn(__fsub_rn(a, mod), b);
  if (mod != 0.0f && mod < 0.0f) div = __fsub_rn(div, 1.0f);
  if (div == 0.0f) return 0.0f;
  float fd = floorf(div);
  if (__fsub_rn(div, fd) > 0.5f) fd += 1.0f;
  return fd;
}

enum { kGridOk = 0, kGridEmpty = 1, kGridTooLarge = 2 };
// noise_dim = ((max - min) // g).astype(int) + 3 from one scene's bounds, as the reference computes it in float32
__device__ inline int elastic_dims(const float *__restrict__ bnd, float g32, int64_t max_cells, int (&nd)[3]) {
  if (!(bnd[0] <= bnd[3])) return kGridEmpty;
  int64_t cells = 1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float q = npy_floor_divide(__fsub_rn(bnd[3 + a], bnd[a]), g32);
    if (!(q < 1048576.0f)) return kGridTooLarge;      // also inf / NaN extents
    nd[a] = (int)q + 3;
    cells *= nd[a];
    if (cells > max_cells) return kGridTooLarge;
  }
  return kGridOk;
}

__global__ void __launch_bounds__(kAugBlock) k_elastic_noise(const float *__restrict__ bounds, int b, float g32, int64_t max_cells,
                                                             uint32_t apply_mask, uint32_t seed_lo, uint32_t seed_hi, SceneSeeds seeds,
                                                             uint32_t stage, float *__restrict__ noise) {
  const int s = blockIdx.y;
  if (s >= b || !((apply_mask >> s) & 1u)) return;
  int nd[3];
  if (elastic_dims(bounds + s * 6, g32, max_cells, nd) != kGridOk) return;
  const int64_t total = (int64_t)nd[0] * nd[1] * nd[2] * 3;      // <= max_cells * 3
  float *slot = noise + (int64_t)s * max_cells * 3;
  for (int64_t e = (int64_t)blockIdx.x * kAugBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kAugBlock) {
    uint32_t c[4] = {(uint32_t)(e / 3), (uint32_t)(e % 3), stage, seed_hi};
    philox4x32_10(c, seed_lo, seeds.v[s]);
    slot[e] = philox_normal(c[0], c[1]);
  }
}

// |{k in [0, d): |i - k| <= 1 and |k - j| <= 1}|, 9 x the (i, j) entry of the squared tridiagonal(1/3) matrix; |i - j| <= 2
__device__ inline int t2_count(int i, int j, int d) { return std::min(std::min(i, j) + 1, d - 1) - std::max(std::max(i, j) - 1, 0) + 1; }

__global__ void __launch_bounds__(kAugBlock) k_elastic_field(const float *__restrict__ bounds, int b, float g32, int64_t max_cells,
                                                             uint32_t apply_mask, const float *__restrict__ noise,
                                                             float *__restrict__ field, int32_t *__restrict__ status) {
  const int s = blockIdx.y;
  if (s >= b || !((apply_mask >> s) & 1u)) return;
  int nd[3];
  const int st = elastic_dims(bounds + s * 6, g32, max_cells, nd);
  if (st != kGridOk) {
    if (st == kGridTooLarge && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, (int32_t)(1u << s));
    return;
  }
  const int nx = nd[0], ny = nd[1], nz = nd[2];
  const int64_t cells = (int64_t)nx * ny * nz;                    // <= max_cells
  const float *src = noise + (int64_t)s * max_cells * 3;
  float *dst = field + (int64_t)s * max_cells * 3;
  for (int64_t cell = (int64_t)blockIdx.x * kAugBlock + threadIdx.x; cell < cells; cell += (int64_t)gridDim.x * kAugBlock) {
    const int iz = (int)(cell % nz), iy = (int)((cell / nz) % ny), ix = (int)(cell / ((int64_t)nz * ny));
    float acc[3] = {0.f, 0.f, 0.f};
    for (int jx = std::max(ix - 2, 0); jx <= std::min(ix + 2, nx - 1); ++jx) {
      const int cx = t2_count(ix, jx, nx);
      for (int jy = std::max(iy - 2, 0); jy <= std::min(iy + 2, ny - 1); ++jy) {
        const int cxy = cx * t2_count(iy, jy, ny);
        for (int jz = std::max(iz - 2, 0); jz <= std::min(iz + 2, nz - 1); ++jz) {
          const float w = (float)(cxy * t2_count(iz, jz, nz));
          const float *q = src + (((int64_t)jx * ny + jy) * nz + jz) * 3;
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[k] = fmaf(w, q[k], acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[cell * 3 + k] = __fdiv_rn(acc[k], 729.0f);
  }
}

__global__ void __launch_bounds__(kAugBlock) k_elastic_apply(float *__restrict__ pts, int64_t n, const int64_t *__restrict__ off, int b,
                                                             const float *__restrict__ bounds, float g32, double g, double magnitude,
                                                             int64_t max_cells, uint32_t apply_mask, const float *__restrict__ field,
                                                             uint32_t *__restrict__ kb_out) {
  const int64_t base = (int64_t)blockIdx.x * kAugBlock, i = base + threadIdx.x;
  const int s_first = scene_of(off, b, base), s_last = scene_of(off, b, std::min<int64_t>(base + kAugBlock - 1, n - 1));
  const bool valid = i < n;
  uint32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  int s = -1;
  if (valid) {
    s = scene_of(off, b, i);
    float p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    int nd[3];
    if (((apply_mask >> s) & 1u) && elastic_dims(bounds + s * 6, g32, max_cells, nd) == kGridOk) {
      int i0[3];
      double t[3];
      bool inside = true;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double u = ((double)p[a] - ((double)bounds[s * 6 + a] - g)) / g;      // axis a: min - g + k g, k = 0 .. nd - 1
        inside = inside && u >= 0.0 && u <= (double)(nd[a] - 1);
        const int k = std::min(std::max((int)floor(u), 0), nd[a] - 2);
        i0[a] = k;
        t[a] = u - (double)k;
      }
      if (inside) {           // RegularGridInterpolator(bounds_error=0, fill_value=0): nothing is added outside the grid
        const float *f = field + (int64_t)s * max_cells * 3;
        double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
          const int cx = corner >> 2, cy = (corner >> 1) & 1, cz = corner & 1;
          const double w = (cx ? t[0] : 1.0 - t[0]) * (cy ? t[1] : 1.0 - t[1]) * (cz ? t[2] : 1.0 - t[2]);
          const float *q = f + (((int64_t)(i0[0] + cx) * nd[1] + (i0[1] + cy)) * nd[2] + (i0[2] + cz)) * 3;
#pragma unroll
          for (int k = 0; k < 3; ++k) v[k] += w * (double)q[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          p[k] = (float)((double)p[k] + v[k] * magnitude);
          pts[3 * i + k] = p[k];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = ord_key(p[c]);
  }
  block_bounds_commit(lo, hi, valid, s, s_first, s_last, kb_out);
}

// ---- voxelise with one affine per scene: the arithmetic of k_voxelize (lgs_voxel.hip), same order, explicitly rounded
__global__ void __launch_bounds__(kAugBlock) k_voxelize_batched(const float *__restrict__ pts, int64_t n, const int64_t *__restrict__ off, int b,
                                                                AffineTable A, int batch_base, int32_t *__restrict__ coords) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = scene_of(off, b, i);
  const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
  int32_t o[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    o[r] = (int32_t)floor(affine_row(A.a[s] + 4 * r, x, y, z));
  }
  reinterpret_cast<int4 *>(coords)[i] = make_int4(batch_base + s, o[0], o[1], o[2]);
}

__global__ void __launch_bounds__(kAugBlock) k_coords_flip_shift(int32_t *__restrict__ coords, int64_t n, const int64_t *__restrict__ off, int b,
                                                                 const int32_t *__restrict__ bounds, FlipTable T) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = scene_of(off, b, i);
  int4 c = reinterpret_cast<int4 *>(coords)[i];
  const uint32_t ax = T.axes[s];
  if (ax & 1u) c.y = bounds[s * 6 + 3] - c.y;
  if (ax & 2u) c.z = bounds[s * 6 + 4] - c.z;
  if (ax & 4u) c.w = bounds[s * 6 + 5] - c.w;
  c.y += T.shift[0];
  c.z += T.shift[1];
  c.w += T.shift[2];
  reinterpret_cast<int4 *>(coords)[i] = c;
}

__global__ void __launch_bounds__(kAugBlock) k_color_augment(float *__restrict__ colors, int64_t n, const int64_t *__restrict__ off, int b,
                                                             const float *__restrict__ bounds, ColorTable T, float scale, int normalize,
                                                             uint32_t seed_lo, uint32_t seed_hi, const float *__restrict__ noise) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int s = scene_of(off, b, i);
  const lgs_color_scene &P = T.s[s];
  const uint64_t row = (uint64_t)(i - off[s]);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double f = (double)colors[3 * i + c];      // double throughout, one rounding at the store: the pass is bound by its 24 B per row
    if (P.flags & LGS_COLOR_AUTOCONTRAST) {
      const double lo = (double)bounds[s * 6 + c], hi = (double)bounds[s * 6 + 3 + c];
      if (hi != lo) f = (1.0 - (double)P.blend) * f + (double)P.blend * ((f - lo) * (255.0 / (hi - lo)));
    }
    if (P.flags & LGS_COLOR_TRANSLATION) f = fmin(fmax(f + (double)P.translation[c], 0.0), 255.0);
    if (P.flags & LGS_COLOR_JITTER) {
      float z;
      if (noise) {
        z = noise[3 * i + c];
      } else {
        uint32_t k[4] = {(uint32_t)row, (uint32_t)(row >> 32), (uint32_t)c, (uint32_t)LGS_AUG_STAGE_COLOR ^ seed_hi};
        philox4x32_10(k, seed_lo, (uint32_t)P.seed);
        z = philox_normal(k[0], k[1]);
      }
      f = fmin(fmax(f + (double)P.jitter_std * 255.0 * (double)z, 0.0), 255.0);
    }
    f *= (double)scale;
    if (normalize) f = f / 255.0 - 0.5;
    colors[3 * i + c] = (float)f;
  }
}

__global__ void k_debug_philox(const uint32_t *__restrict__ counters, int64_t n, uint32_t k0, uint32_t k1, uint32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t c[4] = {counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3]};
  philox4x32_10(c, k0, k1);
#pragma unroll
  for (int k = 0; k < 4; ++k) out[4 * i + k] = c[k];
}

inline unsigned row_blocks(int64_t n) { return (unsigned)((n + kAugBlock - 1) / kAugBlock); }
inline bool rows_fit(int64_t n) { return (n + kAugBlock - 1) / kAugBlock <= 0x7fffffffll; }

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" {

int lgs_aug_bounds(const void *table, int64_t n, int form, int64_t *scene_offsets, int b, void *bounds, void *stream) {
  LGS_REQUIRE(form == LGS_AUG_F32X3 || form == LGS_AUG_I32X4, "lgs_aug_bounds: form must be LGS_AUG_F32X3 or LGS_AUG_I32X4");
  LGS_REQUIRE(b >= 1 && b <= kAugScenes, "lgs_aug_bounds: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(n >= 0 && rows_fit(n) && scene_offsets && bounds && (n == 0 || table), "lgs_aug_bounds: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int is_float = form == LGS_AUG_F32X3;
  uint32_t *kb = static_cast<uint32_t *>(bounds);
  LGS_KLAUNCH(k_aug_bounds_init, 1, kAugBlock, 0, s, kb, b, is_float);
  if (!is_float) {
    if (n == 0) LGS_HIP(hipMemsetAsync(scene_offsets, 0, sizeof(int64_t) * (b + 1), s));
    else LGS_KLAUNCH(k_aug_scene_offsets, row_blocks(n), kAugBlock, 0, s, static_cast<const int32_t *>(table), n, b, scene_offsets);
  }
  if (n > 0) {
    if (is_float) LGS_KLAUNCH(k_aug_bounds<true>, row_blocks(n), kAugBlock, 0, s, table, n, scene_offsets, b, kb);
    else LGS_KLAUNCH(k_aug_bounds<false>, row_blocks(n), kAugBlock, 0, s, table, n, scene_offsets, b, kb);
  }
  LGS_KLAUNCH(k_aug_bounds_decode, 1, kAugBlock, 0, s, kb, b, is_float);
  LGS_HIP(hipGetLastError());
  return 0;
}

int64_t lgs_elastic_workspace_bytes(int b, int64_t max_cells) {
  if (b < 1 || b > kAugScenes || max_cells < 27 || max_cells > (1ll << 26)) return 0;
  return elastic_layout(b, max_cells).total;
}

int lgs_elastic_distort(float *points, int64_t n, const int64_t *scene_offsets, int b, const float *bounds_in, double granularity,
                        double magnitude, int64_t seed, const int32_t *scene_seeds, int apply_mask, int stage, const float *noise,
                        int64_t max_cells, void *workspace, float *bounds_out, int32_t *status, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kAugScenes, "lgs_elastic_distort: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(max_cells >= 27 && max_cells <= (1ll << 26), "lgs_elastic_distort: 27 <= max_cells <= 2^26");
  LGS_REQUIRE(granularity > 0.0 && std::isfinite(granularity) && std::isfinite(magnitude), "lgs_elastic_distort: bad granularity / magnitude");
  LGS_REQUIRE(n >= 0 && rows_fit(n) && scene_offsets && bounds_in && bounds_out && bounds_in != bounds_out && status && workspace &&
                  (n == 0 || points),
              "lgs_elastic_distort: bad argument");
  LGS_REQUIRE(stage >= 0 && stage < LGS_AUG_STAGE_COLOR, "lgs_elastic_distort: 0 <= stage < LGS_AUG_STAGE_COLOR");
  hipStream_t s = (hipStream_t)stream;
  uint32_t *kb = reinterpret_cast<uint32_t *>(bounds_out);
  LGS_KLAUNCH(k_aug_bounds_init, 1, kAugBlock, 0, s, kb, b, 1);
  if (n > 0) {
    const float g32 = (float)granularity;
    const uint32_t mask = (uint32_t)apply_mask;
    const ElasticWs w = elastic_layout(b, max_cells);
    float *ws_noise = Layout::at<float>(workspace, w.noise), *ws_field = Layout::at<float>(workspace, w.field);
    if (mask) {
      if (!noise) {
        SceneSeeds seeds;
        for (int i = 0; i < kAugScenes; ++i) seeds.v[i] = (scene_seeds && i < b) ? (uint32_t)scene_seeds[i] : 0u;
        LGS_KLAUNCH(k_elastic_noise, dim3(kFieldBlocks, b), kAugBlock, 0, s, bounds_in, b, g32, max_cells, mask, (uint32_t)seed,
                    (uint32_t)((uint64_t)seed >> 32), seeds, (uint32_t)stage, ws_noise);
      }
      LGS_KLAUNCH(k_elastic_field, dim3(kFieldBlocks, b), kAugBlock, 0, s, bounds_in, b, g32, max_cells, mask, noise ? noise : ws_noise,
                  ws_field, status);
    }
    LGS_KLAUNCH(k_elastic_apply, row_blocks(n), kAugBlock, 0, s, points, n, scene_offsets, b, bounds_in, g32, granularity, magnitude,
                max_cells, mask, ws_field, kb);
  }
  LGS_KLAUNCH(k_aug_bounds_decode, 1, kAugBlock, 0, s, kb, b, 1);
  LGS_HIP(hipGetLastError());
  return 0;
}

int lgs_voxelize_batched(const float *points, int64_t n, const int64_t *scene_offsets, int b, const double *affines, int batch_base,
                         int32_t *coords, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kAugScenes, "lgs_voxelize_batched: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(affines && scene_offsets && n >= 0 && rows_fit(n) && (n == 0 || (points && coords)), "lgs_voxelize_batched: bad argument");
  LGS_REQUIRE(batch_base >= 0 && batch_base + b <= 1024, "lgs_voxelize_batched: batch index out of range");
  if (n == 0) return 0;
  AffineTable A;
  std::memset(&A, 0, sizeof(A));
  std::memcpy(&A, affines, sizeof(double) * 12 * b);
  LGS_KLAUNCH(k_voxelize_batched, row_blocks(n), kAugBlock, 0, (hipStream_t)stream, points, n, scene_offsets, b, A, batch_base, coords);
  LGS_HIP(hipGetLastError());
  return 0;
}

int lgs_coords_flip_shift(int32_t *coords, int64_t n, const int64_t *scene_offsets, int b, const int32_t *bounds, const int32_t *flip_axes,
                          const int32_t *shift, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kAugScenes, "lgs_coords_flip_shift: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(flip_axes && scene_offsets && bounds && n >= 0 && rows_fit(n) && (n == 0 || coords), "lgs_coords_flip_shift: bad argument");
  if (n == 0) return 0;
  FlipTable T;
  std::memset(&T, 0, sizeof(T));
  for (int i = 0; i < b; ++i) T.axes[i] = (uint8_t)(flip_axes[i] & 7);
  for (int a = 0; a < 3; ++a) T.shift[a] = shift ? shift[a] : 0;
  LGS_KLAUNCH(k_coords_flip_shift, row_blocks(n), kAugBlock, 0, (hipStream_t)stream, coords, n, scene_offsets, b, bounds, T);
  LGS_HIP(hipGetLastError());
  return 0;
}

int lgs_color_augment(float *colors, int64_t n, const int64_t *scene_offsets, int b, const float *bounds, const lgs_color_scene *scenes,
                      float scale, int normalize, int64_t seed, const float *noise, void *stream) {
  LGS_REQUIRE(b >= 1 && b <= kAugScenes, "lgs_color_augment: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(scenes && scene_offsets && bounds && n >= 0 && rows_fit(n) && (n == 0 || colors), "lgs_color_augment: bad argument");
  if (n == 0) return 0;
  ColorTable T;
  std::memset(&T, 0, sizeof(T));
  std::memcpy(&T, scenes, sizeof(lgs_color_scene) * b);
  LGS_KLAUNCH(k_color_augment, row_blocks(n), kAugBlock, 0, (hipStream_t)stream, colors, n, scene_offsets, b, bounds, T, scale, normalize,
              (uint32_t)seed, (uint32_t)((uint64_t)seed >> 32), noise);
  LGS_HIP(hipGetLastError());
  return 0;
}

int lgs_aug_status(const int32_t *status, int *flags, void *stream) {
  LGS_REQUIRE(status && flags, "lgs_aug_status: null argument");
  int32_t host = 0;
  LGS_HIP(hipMemcpyAsync(&host, status, sizeof(host), hipMemcpyDeviceToHost, (hipStream_t)stream));
  LGS_HIP(hipStreamSynchronize((hipStream_t)stream));
  *flags = (int)host;
  return 0;
}

int lgs_debug_philox(const int32_t *counters, int64_t n, int64_t key, int32_t *out, void *stream) {
  LGS_REQUIRE(n >= 0 && rows_fit(n) && (n == 0 || (counters && out)), "lgs_debug_philox: bad argument");
  if (n == 0) return 0;
  LGS_KLAUNCH(k_debug_philox, row_blocks(n), kAugBlock, 0, (hipStream_t)stream, reinterpret_cast<const uint32_t *>(counters), n,
              (uint32_t)key, (uint32_t)((uint64_t)key >> 32), reinterpret_cast<uint32_t *>(out));
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
