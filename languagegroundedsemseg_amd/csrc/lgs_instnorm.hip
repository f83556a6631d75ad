// lgs_instnorm.hip -- MinkowskiInstanceNorm: BatchNorm with one statistics row per (scene, channel) (gfx950).
//
// Replaces ME.MinkowskiInstanceNorm forward + autograd backward as the reference calls it:
//   /root/reference/models/clip_models.py:408-437 (the 512-channel heads of Res16UNet34Dv2 / Dv3, level 0)
//   /root/reference/models/modules/resnet_block.py:64-70,126-132, models/modules/common.py:17-27 (BasicBlockIN[BN], every level)
//
//   mean[s, c] = avg over the rows of scene s,  var[s, c] = biased variance,  y = (x - mean) / sqrt(var + eps) * weight + bias
//
// A scene is one row of the origin map; its rows are one run of sorted positions of the ORIGIN segment map (lgs_common.h
// SegMap), cut into chunk items of at most kSegChunk rows.  Three launches per direction, two passes over the big tensors:
//   k_in_reduce    one workgroup per chunk item (every item lies in one scene: no per-row branch).  Lane groups own a fixed
//                  channel group and take the item's kInRun-row runs round robin; a run is summed in fp32 in position order
//                  (four rows of loads in flight), runs are added up in double, the lane groups' doubles are folded through LDS
//                  in group order -> part[item][2C] fp32.  forward: sum (x - pivot), sum (x - pivot)^2 with pivot = the scene's
//                  first row in sorted order (never E[x^2] - E[x]^2 about zero); backward: sum dy, sum dy * xhat.
//   k_in_combine   one workgroup per (scene, kInCombCh channels): kInCombSl slices walk the scene's items in item order, all
//                  in double, folded in slice order -> forward stats[scene][2C] = (mean, rstd), backward sums[scene][2C].
//   k_in_apply     ROW-stationary: rows in the caller's order, each read and written once, the scene of a row from
//                  SegMap::row_seg.  A thread owns a fixed channel group (weight / bias loaded once) and reloads the scene's
//                  statistics only when the scene changes from one of its rows to the next.  The backward apply's first
//                  workgroups also fold the scene sums into dweight / dbias, scenes in ascending order.
// No float atomics anywhere: two runs give the same bits.  Everything a call decides on the host comes from instnorm_plan();
// the row accesses, lanes per row, grids and the lift from (dtype, width) to template arguments are lgs_rows.h's.
#include "lgs_rows.h"

namespace lgs {
namespace {

constexpr int kNT = 256;          // threads per workgroup of every kernel here
constexpr int kInRun = 32;        // k_in_reduce: rows summed in fp32 before the sum moves into a double
constexpr int kInCombCh = 16;     // k_in_combine: channels per workgroup ...
constexpr int kInCombSl = 16;     // ... and item slices per channel (kInCombCh * kInCombSl == kNT)
constexpr int kInApplyIters = 16;  // k_in_apply: rows per thread; a workgroup covers (kNT >> lg) * kInApplyIters rows
enum { kInFwd = 0, kInBwd = 1 };

// ---- pass 1 of both directions: one workgroup per chunk item -> part[item][2C]
// DIR == kInFwd: a = x - pivot, (sum a, sum a^2);  kInBwd: xhat = (x - mean) * rstd, (sum dy, sum dy * xhat)
template <typename T, bool VEC, int DIR>
__global__ __launch_bounds__(kNT) void k_in_reduce(SegMap sm, const T *__restrict__ x, const T *__restrict__ dy,
                                                   const float *__restrict__ stats, int c, int lg, float *__restrict__ part) {
  constexpr int V = Width<T, VEC>::V;
  __shared__ double red[2 * kNT * V];   // [2][groups][lanes * V]
  const int32_t u = (int32_t)blockIdx.x;
  const int32_t q = sm.item_seg[u];
  if (q < 0) return;                    // unused slot of the item table (sized by a bound): nothing reads its partial row
  const int32_t s0 = sm.seg_start[q];
  const int32_t s = s0 + (u - sm.item_start[q]) * kSegChunk;
  const int32_t e = min(s + kSegChunk, sm.seg_start[q + 1]);
  const int32_t *fr = sm.fine_row;
  const int lanes = 1 << lg, groups = kNT >> lg;
  const int lane = (int)threadIdx.x & (lanes - 1), grp = (int)threadIdx.x >> lg;
  const int span = V << lg;             // channels one pass of the lanes covers
  const int64_t prow = fr ? fr[s0] : s0;
  for (int c0 = 0; c0 < c; c0 += span) {
    const int col = c0 + lane * V;
    const bool on = col < c;
    double a0[V], a1[V];
#pragma unroll
    for (int i = 0; i < V; ++i) a0[i] = a1[i] = 0.0;
    if (on) {
      float m[V], rs[V];                // forward: the pivot (rs unused); backward: mean and rstd of the scene
      if constexpr (DIR == kInFwd) {
        ldv<V>(x + prow * c + col, m);
      } else {
        ldf<V>(stats + (int64_t)q * 2 * c + col, m);
        ldf<V>(stats + (int64_t)q * 2 * c + c + col, rs);
      }
      for (int32_t r0 = s + grp * kInRun; r0 < e; r0 += groups * kInRun) {
        const int32_t r1 = min(r0 + kInRun, e);
        float f0[V], f1[V];
#pragma unroll
        for (int i = 0; i < V; ++i) f0[i] = f1[i] = 0.f;
        int32_t p = r0;
        for (; p + 4 <= r1; p += 4) {   // four rows in flight, accumulated in position order
          int64_t r[4];
          float v[4][V], g[4][V];
#pragma unroll
          for (int j = 0; j < 4; ++j) r[j] = fr ? fr[p + j] : p + j;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            ldv<V>(x + r[j] * c + col, v[j]);
            if constexpr (DIR == kInBwd) ldv<V>(dy + r[j] * c + col, g[j]);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
              if constexpr (DIR == kInFwd) {
                const float a = v[j][i] - m[i];
                f0[i] += a;
                f1[i] += a * a;
              } else {
                f0[i] += g[j][i];
                f1[i] += g[j][i] * ((v[j][i] - m[i]) * rs[i]);
              }
            }
          }
        }
        for (; p < r1; ++p) {
          const int64_t r = fr ? fr[p] : p;
          float v[V], g[V];
          ldv<V>(x + r * c + col, v);
          if constexpr (DIR == kInBwd) ldv<V>(dy + r * c + col, g);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            if constexpr (DIR == kInFwd) {
              const float a = v[i] - m[i];
              f0[i] += a;
              f1[i] += a * a;
            } else {
              f0[i] += g[i];
              f1[i] += g[i] * ((v[i] - m[i]) * rs[i]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) {
          a0[i] += (double)f0[i];
          a1[i] += (double)f1[i];
        }
      }
    }
    if (c0 > 0) __syncthreads();        // the previous pass's fold has read `red`
#pragma unroll
    for (int i = 0; i < V; ++i) {
      red[grp * span + lane * V + i] = a0[i];
      red[kNT * V + grp * span + lane * V + i] = a1[i];
    }
    __syncthreads();
    for (int t = (int)threadIdx.x; t < 2 * span; t += kNT) {   // fold the lane groups in group order
      const int k = t >= span ? 1 : 0, cc = t - k * span;
      if (c0 + cc < c) {
        double acc = 0.0;
        for (int g = 0; g < groups; ++g) acc += red[k * kNT * V + g * span + cc];
        part[(int64_t)u * 2 * c + k * c + c0 + cc] = (float)acc;
      }
    }
  }
}

// ---- pass 2: scene q folds its items' partial rows in item order, in double
// forward: stats[q] = (mean, rstd) with mean = pivot + S1 / n, var = S2 / n - (S1 / n)^2;  backward: sums[q] = (S1, S2)
template <typename T, int DIR>
__global__ __launch_bounds__(kNT) void k_in_combine(SegMap sm, const float *__restrict__ part, const T *__restrict__ x, int c, float eps,
                                                    float *__restrict__ out) {
  __shared__ double red[2][kInCombSl][kInCombCh];
  const int nb = (c + kInCombCh - 1) / kInCombCh;
  const int32_t q = (int32_t)(blockIdx.x / nb);
  const int col = (int)(blockIdx.x % nb) * kInCombCh + ((int)threadIdx.x & (kInCombCh - 1));
  const int sl = (int)threadIdx.x / kInCombCh;
  const int32_t i0 = sm.item_start[q], i1 = sm.item_start[q + 1];
  double a0 = 0.0, a1 = 0.0;
  if (col < c) {
    int32_t i = i0 + sl;
    for (; i + 3 * kInCombSl < i1; i += 4 * kInCombSl) {   // four items of loads in flight
      float v0[4], v1[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v0[j] = part[(int64_t)(i + j * kInCombSl) * 2 * c + col];
        v1[j] = part[(int64_t)(i + j * kInCombSl) * 2 * c + c + col];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { a0 += (double)v0[j]; a1 += (double)v1[j]; }
    }
    for (; i < i1; i += kInCombSl) {
      a0 += (double)part[(int64_t)i * 2 * c + col];
      a1 += (double)part[(int64_t)i * 2 * c + c + col];
    }
  }
  red[0][sl][threadIdx.x & (kInCombCh - 1)] = a0;
  red[1][sl][threadIdx.x & (kInCombCh - 1)] = a1;
  __syncthreads();
  if (sl != 0 || col >= c) return;
  a0 = a1 = 0.0;
  for (int j = 0; j < kInCombSl; ++j) {
    a0 += red[0][j][threadIdx.x];
    a1 += red[1][j][threadIdx.x];
  }
  if constexpr (DIR == kInFwd) {
    const int32_t s0 = sm.seg_start[q];
    const double n = (double)(sm.seg_start[q + 1] - s0);
    const int64_t prow = sm.fine_row ? sm.fine_row[s0] : s0;
    const double d = a0 / n;
    double var = a1 / n - d * d;
    var = var > 0.0 ? var : 0.0;
    out[(int64_t)q * 2 * c + col] = (float)((double)ld_elem(x + prow * c + col) + d);
    out[(int64_t)q * 2 * c + c + col] = (float)(1.0 / sqrt(var + (double)eps));
  } else {
    out[(int64_t)q * 2 * c + col] = (float)a0;
    out[(int64_t)q * 2 * c + c + col] = (float)a1;
  }
}

// ---- pass 3: row-stationary apply.  forward: y = (x - mean) * rstd * weight + bias
// backward: dx = weight * rstd * (dy - sum_dy / n - xhat * sum_dy_xhat / n); workgroups [0, ceil(c / kNT)) also write
// dweight[c] = sum over scenes of sum_dy_xhat, dbias[c] = sum over scenes of sum_dy (ascending scenes, double)
template <typename T, bool VEC, int DIR>
__global__ __launch_bounds__(kNT) void k_in_apply(SegMap sm, const T *__restrict__ x, const T *__restrict__ dy,
                                                  const float *__restrict__ stats, const float *__restrict__ sums,
                                                  const float *__restrict__ weight, const float *__restrict__ bias, int c, int lg,
                                                  T *__restrict__ out, float *__restrict__ dweight, float *__restrict__ dbias) {
  constexpr int V = Width<T, VEC>::V;
  if constexpr (DIR == kInBwd) {
    const int64_t col = (int64_t)blockIdx.x * kNT + threadIdx.x;
    if (col < c) {
      double dw = 0.0, db = 0.0;
      for (int64_t q = 0; q < sm.n_coarse; ++q) {
        db += (double)sums[q * 2 * c + col];
        dw += (double)sums[q * 2 * c + c + col];
      }
      dweight[col] = (float)dw;
      dbias[col] = (float)db;
    }
  }
  const int lanes = 1 << lg, groups = kNT >> lg;
  const int lane = (int)threadIdx.x & (lanes - 1), grp = (int)threadIdx.x >> lg;
  const int span = V << lg;
  const int64_t base = (int64_t)blockIdx.x * groups * kInApplyIters + grp;
  const int32_t *rs = sm.row_seg;
  for (int col = lane * V; col < c; col += span) {
    float w[V], b[V], m[V], k0[V], k1[V], k2[V];   // forward: k0 = rstd * weight; backward: k0 likewise, k1 = sum_dy / n, k2 = rstd * sum_dy_xhat / n
    ldf<V>(weight + col, w);
    if constexpr (DIR == kInFwd) ldf<V>(bias + col, b);
    int32_t qc = -1;
    for (int it = 0; it < kInApplyIters; it += 4) {   // four rows in flight
      int64_t r[4];
      int32_t q[4];
      float v[4][V], g[4][V];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[j] = base + (int64_t)(it + j) * groups;
        q[j] = r[j] < sm.n_fine ? rs[r[j]] : -1;
        if ((uint32_t)q[j] >= (uint32_t)sm.n_coarse) q[j] = -1;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (q[j] >= 0) {
          ldv<V>(x + r[j] * c + col, v[j]);
          if constexpr (DIR == kInBwd) ldv<V>(dy + r[j] * c + col, g[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (q[j] < 0) continue;
        if (q[j] != qc) {
          qc = q[j];
          float rstd[V];
          ldf<V>(stats + (int64_t)qc * 2 * c + col, m);
          ldf<V>(stats + (int64_t)qc * 2 * c + c + col, rstd);
          if constexpr (DIR == kInBwd) {
            const float inv_n = 1.f / (float)(sm.seg_start[qc + 1] - sm.seg_start[qc]);
            ldf<V>(sums + (int64_t)qc * 2 * c + col, k1);
            ldf<V>(sums + (int64_t)qc * 2 * c + c + col, k2);
#pragma unroll
            for (int i = 0; i < V; ++i) {
              k1[i] = k1[i] * inv_n;
              k2[i] = k2[i] * inv_n * rstd[i];
            }
          }
#pragma unroll
          for (int i = 0; i < V; ++i) k0[i] = rstd[i] * w[i];
        }
        float o[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
          if constexpr (DIR == kInFwd) o[i] = (v[j][i] - m[i]) * k0[i] + b[i];
          else o[i] = k0[i] * (g[j][i] - k1[i] - (v[j][i] - m[i]) * k2[i]);
        }
        stv<V>(out + r[j] * c + col, o);
      }
    }
  }
}

}  // namespace

// Everything an instance-norm call decides on the host, from plain integers (no HIP call): the access width, the lanes per row,
// the grids of the direction's three launches and the workspace regions.  `ptr16`: the feature pointers are 16-byte aligned.
using InstNormPlan = lgs_instnorm_plan_info;
InstNormPlan instnorm_plan(int dir, int64_t n_fine, int64_t n_seg, int64_t n_items, int c, int dtype, bool ptr16) {
  InstNormPlan p = {};
  const int es = esize(dtype);
  p.vec = (c * es) % 16 == 0 && ptr16 ? 1 : 0;
  p.lanes_log2 = lanes_log2(c, p.vec ? 16 / es : 1);
  p.rows_per_apply_block = (kNT >> p.lanes_log2) * kInApplyIters;
  int64_t used = 0;   // the workspace itself is 256-byte aligned (the callers' allocators give that), so `sums` is 16-byte aligned too
  p.partials = take_region(used, n_items * 2 * (int64_t)c * 4);
  if (dir == kInBwd) p.sums = take_region(used, n_seg * 2 * (int64_t)c * 4);
  p.bytes_total = used;
  p.workspace_bytes = align256(n_items * 2 * (int64_t)c * 4) + align256(n_seg * 2 * (int64_t)c * 4);   // the backward layout: the larger one
  if (n_fine > 0 && n_seg > 0) {
    p.reduce_grid = n_items;
    p.combine_grid = n_seg * ((c + kInCombCh - 1) / kInCombCh);
    p.apply_grid = grid_for(n_fine, p.lanes_log2, kInApplyIters);
    if (dir == kInBwd && p.apply_grid < (c + kNT - 1) / kNT) p.apply_grid = (c + kNT - 1) / kNT;   // the dweight / dbias fold
  }
  return p;
}

namespace {

template <typename T, bool VEC>
int forward_t(const SegMap &sm, const InstNormPlan &p, const void *xv, int c, const float *weight, const float *bias, float eps, void *yv,
              float *stats, void *ws, hipStream_t s) {
  const T *x = (const T *)xv;
  float *part = (float *)((char *)ws + p.partials.offset);
  LGS_KLAUNCH((k_in_reduce<T, VEC, kInFwd>), (unsigned)p.reduce_grid, kNT, 0, s, sm, x, nullptr, nullptr, c, p.lanes_log2, part);
  LGS_KLAUNCH((k_in_combine<T, kInFwd>), (unsigned)p.combine_grid, kNT, 0, s, sm, part, x, c, eps, stats);
  LGS_KLAUNCH((k_in_apply<T, VEC, kInFwd>), (unsigned)p.apply_grid, kNT, 0, s, sm, x, nullptr, stats, nullptr, weight, bias, c, p.lanes_log2,
              (T *)yv, nullptr, nullptr);
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool VEC>
int backward_t(const SegMap &sm, const InstNormPlan &p, const void *xv, const void *dyv, int c, const float *weight, const float *stats,
               void *dxv, float *dweight, float *dbias, void *ws, hipStream_t s) {
  const T *x = (const T *)xv, *dy = (const T *)dyv;
  float *part = (float *)((char *)ws + p.partials.offset);
  float *sums = (float *)((char *)ws + p.sums.offset);
  LGS_KLAUNCH((k_in_reduce<T, VEC, kInBwd>), (unsigned)p.reduce_grid, kNT, 0, s, sm, x, dy, stats, c, p.lanes_log2, part);
  LGS_KLAUNCH((k_in_combine<T, kInBwd>), (unsigned)p.combine_grid, kNT, 0, s, sm, part, x, c, 0.f, sums);
  LGS_KLAUNCH((k_in_apply<T, VEC, kInBwd>), (unsigned)p.apply_grid, kNT, 0, s, sm, x, dy, stats, sums, weight, nullptr, c, p.lanes_log2,
              (T *)dxv, dweight, dbias);
  LGS_HIP(hipGetLastError());
  return 0;
}

// what both entry points ask of the segment map
int check_map(const lgs_segmap *h, int c, int dtype, const char *who) {
  LGS_REQUIRE(h && c > 0 && (dtype == LGS_F32 || dtype == LGS_BF16), std::string(who) + ": bad argument");
  LGS_REQUIRE(h->sm.max_len == 0, std::string(who) + ": the segment map's coarse side must be the origin map (one row per scene)");
  return 0;
}

}  // namespace
}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_in_workspace_bytes(const lgs_segmap *h, int c) {
  if (!h || c <= 0 || h->sm.max_len != 0) return 0;
  const SegMap &sm = h->sm;
  return instnorm_plan(kInBwd, sm.n_fine, sm.n_coarse, sm.n_items, c, LGS_F32, true).workspace_bytes;
}

int lgs_in_forward(lgs_segmap *h, const void *x, int c, const float *weight, const float *bias, float eps, void *y, float *stats,
                   int dtype, void *workspace, void *stream) {
  if (check_map(h, c, dtype, "lgs_in_forward")) return 2;
  const SegMap &sm = h->sm;
  if (sm.n_fine == 0 || sm.n_coarse == 0) return 0;
  LGS_REQUIRE(x && y && weight && bias && stats && workspace, "lgs_in_forward: null pointer");
  LGS_REQUIRE(sm.row_seg && sm.item_seg, "lgs_in_forward: the segment map carries no row table");
  hipStream_t s = (hipStream_t)stream;
  if (segmap_wait(h, s)) return 1;
  const InstNormPlan p = instnorm_plan(kInFwd, sm.n_fine, sm.n_coarse, sm.n_items, c, dtype, al16(x) && al16(y) && al16(weight) && al16(bias) && al16(stats));
  return with_row_type(dtype, p.vec, "lgs_in_forward", [&](auto e) {
    using E = decltype(e);
    return forward_t<typename E::T, E::vec>(sm, p, x, c, weight, bias, eps, y, stats, workspace, s);
  });
}

int lgs_in_backward(lgs_segmap *h, const void *x, const void *dy, int c, const float *weight, const float *stats, void *dx,
                    float *dweight, float *dbias, int dtype, void *workspace, void *stream) {
  if (check_map(h, c, dtype, "lgs_in_backward")) return 2;
  const SegMap &sm = h->sm;
  hipStream_t s = (hipStream_t)stream;
  if (sm.n_fine == 0 || sm.n_coarse == 0) {   // no row: the parameter gradients are zero
    if (dweight) LGS_HIP(hipMemsetAsync(dweight, 0, (size_t)c * 4, s));
    if (dbias) LGS_HIP(hipMemsetAsync(dbias, 0, (size_t)c * 4, s));
    return 0;
  }
  LGS_REQUIRE(x && dy && dx && weight && stats && dweight && dbias && workspace, "lgs_in_backward: null pointer");
  LGS_REQUIRE(sm.row_seg && sm.item_seg, "lgs_in_backward: the segment map carries no row table");
  if (segmap_wait(h, s)) return 1;
  const InstNormPlan p = instnorm_plan(kInBwd, sm.n_fine, sm.n_coarse, sm.n_items, c, dtype, al16(x) && al16(dy) && al16(dx) && al16(weight) && al16(stats));
  return with_row_type(dtype, p.vec, "lgs_in_backward", [&](auto e) {
    using E = decltype(e);
    return backward_t<typename E::T, E::vec>(sm, p, x, dy, c, weight, stats, dx, dweight, dbias, workspace, s);
  });
}

// the plan of a call given by plain integers: no HIP call (tests/test_instnorm_cpu.py)
int lgs_debug_instnorm_plan(const lgs_instnorm_plan_query *q, lgs_instnorm_plan_info *out) {
  LGS_REQUIRE(q && out && q->c > 0 && (q->dtype == LGS_F32 || q->dtype == LGS_BF16) && (q->direction == kInFwd || q->direction == kInBwd) &&
                  q->n_fine >= 0 && q->n_seg >= 0 && q->n_items >= 0,
              "lgs_debug_instnorm_plan: bad argument");
  *out = instnorm_plan(q->direction, q->n_fine, q->n_seg, q->n_items, q->c, q->dtype, true);
  return 0;
}

}  // extern "C"
