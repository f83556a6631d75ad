// lgs_supcon.hip -- the supervised point-contrastive loss (PointSupConLoss) on the device, gfx950.
//
// Replaces the body of lib/losses/PointSupConLoss.py:74-154: per class of the batch a mask, three device -> host copies and two
// np.random.choice calls over all N points inside a joblib pool, then pos_samples [N, P, C] and neg_samples [N, K, C] in fp32, both
// normalised, and a bmm.  Three kernels, no LDS, no atomics, no workspace:
//
//   k_supcon_sample   one thread per (row, slot).  A Philox-4x32-10 block keyed by the seed with the counter (row, slot) gives two
//                     64-bit numbers, so the result is a function of (seed, row, slot) alone -- not of the grid.  A positive slot
//                     takes a uniform offset into the segment of the row's class in `order`; a negative slot first finds its class
//                     by a binary search of a uniform integer below the row's total in the cumulative INT64 table
//                     cum[u, c] = sum_{c' <= c} hist[u, c'] * m[c'] * [c' != u], then a uniform offset into the first m[c] entries
//                     (the eligible points) of that class's segment.  Integer weights: a class of weight 0 owns no integer of the
//                     range and is never drawn.  A uniform integer below t is the high word of rand64 * t (bias < t / 2^64).
//   k_supcon_fwd      one wavefront per row: the row and its P + K gathered rows are read once (16-byte loads when a row is a
//                     multiple of 16 bytes, element loads otherwise; a loop over the width), dot products and squared norms (or
//                     squared differences) are summed in fp32 over the wave.  Bytes: (1 + P + K) * N * C * e.
//   k_supcon_bwd      one wavefront per row, element-wise in the row: the same reads, one write of N * C * e.  No reduction -- the
//                     forward left the per-sample similarities / distances and 1 / |row| of every row.
// Sampled rows are constants (the reference detaches them): only the row's own term has a gradient.
#include <algorithm>

#include "lgs_common.h"
#include "lgs_philox.h"

namespace lgs {

namespace {

constexpr int kSupMaxS = 8;            // P and K are 1 .. 8 each
constexpr int kSupWaves = 4;           // rows (wavefronts) per workgroup
constexpr float kNormEps = 1e-12f;     // F.normalize's eps
constexpr float kL2Eps = 1e-7f;        // PointSupConLoss.py:56

// uniform integer in [0, t), t >= 1
__device__ inline int64_t below(uint64_t r, int64_t t) { return (int64_t)__umul64hi(r, (uint64_t)t); }

__global__ void __launch_bounds__(256) k_supcon_sample(const int64_t *__restrict__ labels, int64_t n, int n_labels, int64_t ignore_label,
                                                       const int64_t *__restrict__ cum, const int64_t *__restrict__ order,
                                                       const int64_t *__restrict__ seg_start, const int64_t *__restrict__ cls_count,
                                                       const int64_t *__restrict__ elig_count, int p, int k, uint64_t seed,
                                                       int64_t *__restrict__ pos_idx, int64_t *__restrict__ neg_idx) {
  const int s_all = p + k;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * s_all) return;
  const int64_t row = t / s_all;
  const int slot = (int)(t - row * s_all);
  int64_t *dst = slot < p ? pos_idx + row * p + slot : neg_idx + row * k + (slot - p);
  const int64_t u = labels[row];
  if (u == ignore_label || u < 0 || u >= n_labels) {
    *dst = -1;
    return;
  }
  uint32_t c[4] = {(uint32_t)row, (uint32_t)((uint64_t)row >> 32), (uint32_t)slot, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t r0 = ((uint64_t)c[1] << 32) | c[0], r1 = ((uint64_t)c[3] << 32) | c[2];
  int64_t cls = u, members = cls_count[u];
  if (slot >= p) {
    const int64_t *row_cum = cum + u * n_labels;
    const int64_t total = row_cum[n_labels - 1];
    if (total <= 0) {       // no eligible point of another class in the batch
      *dst = -1;
      return;
    }
    const int64_t x = below(r0, total);
    cls = upper_bound(row_cum, 0, n_labels - 1, x);     // the first class whose cumulative weight exceeds x; cum[n_labels - 1] = total > x
    members = elig_count[cls];
  }
  if (members <= 0) {       // (cannot happen with tables built from these labels)
    *dst = -1;
    return;
  }
  const int64_t at = std::min<int64_t>(std::max<int64_t>(seg_start[cls] + below(r1, members), 0), n - 1);
  *dst = order[at];
}

// ---- row access: W elements per lane and step, as fp32
template <typename T, bool VEC> struct SupRow;
template <> struct SupRow<float, true> {
  static constexpr int W = 4;
  __device__ static void load(const float *p, float (&v)[4]) { const float4 x = *reinterpret_cast<const float4 *>(p); v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w; }
  __device__ static void store(float *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct SupRow<bf16_t, true> {
  static constexpr int W = 8;
  __device__ static void load(const bf16_t *p, float (&v)[8]) {
    const uint4 x = *reinterpret_cast<const uint4 *>(p);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = bf16_to_f32((uint16_t)(w[i] & 0xffff)); v[2 * i + 1] = bf16_to_f32((uint16_t)(w[i] >> 16)); }
  }
  __device__ static void store(bf16_t *p, const float (&v)[8]) {
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f32_to_bf16(v[2 * i]) | ((uint32_t)f32_to_bf16(v[2 * i + 1]) << 16);
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  }
};
template <> struct SupRow<float, false> {
  static constexpr int W = 1;
  __device__ static void load(const float *p, float (&v)[1]) { v[0] = *p; }
  __device__ static void store(float *p, const float (&v)[1]) { *p = v[0]; }
};
template <> struct SupRow<bf16_t, false> {
  static constexpr int W = 1;
  __device__ static void load(const bf16_t *p, float (&v)[1]) { v[0] = bf16_to_f32(*p); }
  __device__ static void store(bf16_t *p, const float (&v)[1]) { *p = f32_to_bf16(v[0]); }
};

// sample index of slot j of `row` (positives first), -1 for "no sample"; anything outside [0, n) is no sample
__device__ inline int64_t slot_index(const int64_t *pos_idx, int p, const int64_t *neg_idx, int k, int64_t row, int j, int64_t n) {
  const int64_t i = j < p ? pos_idx[row * p + j] : neg_idx[row * k + (j - p)];
  return (i >= 0 && i < n) ? i : -1;
}

// COS: sim[row, j] = <a^, b^_j>;  else sim[row, j] = sqrt(|a - b_j|^2 + 1e-7)
template <typename T, bool VEC, bool COS>
__global__ void __launch_bounds__(64 * kSupWaves) k_supcon_fwd(const T *__restrict__ feat, int64_t n, int c, const int64_t *__restrict__ labels,
                                                              const int64_t *__restrict__ pos_idx, int p, const int64_t *__restrict__ neg_idx,
                                                              int k, int64_t ignore_label, int n_labels, float *__restrict__ d_pos,
                                                              float *__restrict__ d_neg, float *__restrict__ sim, float *__restrict__ inv_norm) {
  using R = SupRow<T, VEC>;
  constexpr int W = R::W;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kSupWaves + (threadIdx.x >> 6);
  if (row >= n) return;                       // wave-uniform
  const int s_all = p + k;
  const int64_t lab = labels[row];
  const bool counted = lab != ignore_label && lab >= 0 && lab < n_labels;
  const T *a_row = feat + row * c;
  float na2 = 0.f;
  float acc[2 * kSupMaxS], nb2[2 * kSupMaxS];
#pragma unroll
  for (int j = 0; j < 2 * kSupMaxS; ++j) acc[j] = nb2[j] = 0.f;
  int64_t idx[2 * kSupMaxS];
#pragma unroll
  for (int j = 0; j < 2 * kSupMaxS; ++j) idx[j] = (counted && j < s_all) ? slot_index(pos_idx, p, neg_idx, k, row, j, n) : -1;
  for (int c0 = lane * W; c0 < c; c0 += 64 * W) {
    float a[W];
    R::load(a_row + c0, a);
#pragma unroll
    for (int i = 0; i < W; ++i) na2 += a[i] * a[i];
    if (!counted) continue;
    // four gathered rows in flight per step
#pragma unroll
    for (int j0 = 0; j0 < 2 * kSupMaxS; j0 += 4) {
      if (j0 >= s_all) break;
      float b[4][W];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (idx[j0 + t] >= 0) {
          R::load(feat + idx[j0 + t] * c + c0, b[t]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i) b[t][i] = 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
          if (COS) {
            acc[j0 + t] += a[i] * b[t][i];
            nb2[j0 + t] += b[t][i] * b[t][i];
          } else {
            const float d = a[i] - b[t][i];
            acc[j0 + t] += d * d;
          }
        }
      }
    }
  }
  na2 = wave_sum(na2);
  const float inv_a = 1.0f / fmaxf(sqrtf(na2), kNormEps);
  float sp = 0.f, sn = 0.f;
#pragma unroll
  for (int j = 0; j < 2 * kSupMaxS; ++j) {
    if (j >= s_all) break;
    float v = 0.f;
    if (counted) {
      const float s = wave_sum(acc[j]);
      if (COS) {
        const float inv_b = 1.0f / fmaxf(sqrtf(wave_sum(nb2[j])), kNormEps);
        v = s * inv_a * inv_b;
      } else {
        v = sqrtf(s + kL2Eps);
      }
    }
    acc[j] = v;
    if (j < p) sp += v; else sn += v;
  }
  if (lane == 0) {
    inv_norm[row] = inv_a;
    float dp = 0.f, dn = 0.f;
    if (counted) {
      dp = COS ? 1.0f - sp / (float)p : sp / (float)p;
      dn = COS ? 1.0f - sn / (float)k : sn / (float)k;
    }
    d_pos[row] = dp;
    d_neg[row] = dn;
  }
  // sim[row, j]: lane j stores slot j (s_all <= 16)
#pragma unroll
  for (int j = 0; j < 2 * kSupMaxS; ++j)
    if (j < s_all && lane == j) sim[row * s_all + j] = acc[j];
}

// COS: gf = inv|a| * sum_j gs_j (b^_j - s_j a^),  gs_j = -g_dpos / P | -g_dneg / K,  b^_j = b_j * inv_norm[idx_j]
//      (a row with |a| <= 1e-12 is a^ = a / 1e-12: the projection term is absent, as in F.normalize's clamp)
// else: gf = sum_j g_j (a - b_j) / (S dist_j)
template <typename T, bool VEC, bool COS>
__global__ void __launch_bounds__(64 * kSupWaves) k_supcon_bwd(const T *__restrict__ feat, int64_t n, int c, const int64_t *__restrict__ labels,
                                                              const int64_t *__restrict__ pos_idx, int p, const int64_t *__restrict__ neg_idx,
                                                              int k, int64_t ignore_label, int n_labels, const float *__restrict__ sim,
                                                              const float *__restrict__ inv_norm, const float *__restrict__ g_dpos,
                                                              const float *__restrict__ g_dneg, T *__restrict__ grad_feat) {
  using R = SupRow<T, VEC>;
  constexpr int W = R::W;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kSupWaves + (threadIdx.x >> 6);
  if (row >= n) return;                       // wave-uniform
  const int s_all = p + k;
  const int64_t lab = labels[row];
  const bool counted = lab != ignore_label && lab >= 0 && lab < n_labels;
  T *g_row = grad_feat + row * c;
  if (!counted) {
    float z[W];
#pragma unroll
    for (int i = 0; i < W; ++i) z[i] = 0.f;
    for (int c0 = lane * W; c0 < c; c0 += 64 * W) R::store(g_row + c0, z);
    return;
  }
  const float gp = (g_dpos ? g_dpos[row] : 0.f) / (float)p, gn = (g_dneg ? g_dneg[row] : 0.f) / (float)k;
  const float inv_a = inv_norm[row];
  int64_t idx[2 * kSupMaxS];
  float wb[2 * kSupMaxS];      // COS: factor of b_j;  else: factor of a - b_j
  float wa = 0.f;              // COS: factor of a
#pragma unroll
  for (int j = 0; j < 2 * kSupMaxS; ++j) {
    idx[j] = -1;
    wb[j] = 0.f;
    if (j >= s_all) continue;
    idx[j] = slot_index(pos_idx, p, neg_idx, k, row, j, n);
    const float g = j < p ? gp : gn;
    const float s = sim[row * s_all + j];
    if (COS) {
      wb[j] = idx[j] >= 0 ? -g * inv_norm[idx[j]] * inv_a : 0.f;
      wa += g * s;
    } else {
      wb[j] = g / s;                      // s = dist_j >= sqrt(1e-7); applied to the difference a - b_j (a row that samples itself
                                          // has dist_j = 3e-4: factoring a out would cancel 3000 |a| against itself)
    }
  }
  if (COS) wa = inv_a < 1.0f / kNormEps ? wa * inv_a * inv_a : 0.f;
  const T *a_row = feat + row * c;
  for (int c0 = lane * W; c0 < c; c0 += 64 * W) {
    float a[W], out[W];
    R::load(a_row + c0, a);
#pragma unroll
    for (int i = 0; i < W; ++i) out[i] = COS ? wa * a[i] : 0.f;
#pragma unroll
    for (int j0 = 0; j0 < 2 * kSupMaxS; j0 += 4) {
      if (j0 >= s_all) break;
      float b[4][W];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (idx[j0 + t] >= 0) {
          R::load(feat + idx[j0 + t] * c + c0, b[t]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i) b[t][i] = 0.f;
        }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < W; ++i) out[i] += COS ? wb[j0 + t] * b[t][i] : wb[j0 + t] * (a[i] - b[t][i]);
    }
    R::store(g_row + c0, out);
  }
}

inline bool sup_vec_ok(const void *a, const void *b, int c, int dtype) {
  return ((int64_t)c * esize(dtype)) % 16 == 0 && ((uintptr_t)a % 16) == 0 && (!b || ((uintptr_t)b % 16) == 0);
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" int lgs_supcon_sample(const int64_t *labels, int64_t n, int n_labels, int64_t ignore_label, const int64_t *cum,
                                 const int64_t *order, const int64_t *seg_start, const int64_t *cls_count, const int64_t *elig_count,
                                 int p, int k, int64_t seed, int64_t *pos_idx, int64_t *neg_idx, void *stream) {
  LGS_REQUIRE(n >= 0 && n_labels >= 1, "lgs_supcon_sample: bad sizes");
  LGS_REQUIRE(p >= 1 && p <= kSupMaxS && k >= 1 && k <= kSupMaxS, "lgs_supcon_sample: P and K must be 1 .. 8");
  if (n == 0) return 0;
  LGS_REQUIRE(labels && cum && order && seg_start && cls_count && elig_count && pos_idx && neg_idx, "lgs_supcon_sample: null argument");
  const int64_t threads = n * (p + k);
  LGS_REQUIRE((threads + 255) / 256 <= 0x7fffffffll, "lgs_supcon_sample: too many rows");
  LGS_KLAUNCH(k_supcon_sample, (unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream, labels, n, n_labels, ignore_label, cum, order,
              seg_start, cls_count, elig_count, p, k, (uint64_t)seed, pos_idx, neg_idx);
  LGS_HIP(hipGetLastError());
  return 0;
}

#define LGS_SUP_DISPATCH(LAUNCH)                                                          \
  do {                                                                                    \
    if (dtype == LGS_F32) {                                                               \
      if (vec) { if (cos) LAUNCH(float, true, true); else LAUNCH(float, true, false); }    \
      else     { if (cos) LAUNCH(float, false, true); else LAUNCH(float, false, false); }  \
    } else {                                                                              \
      if (vec) { if (cos) LAUNCH(bf16_t, true, true); else LAUNCH(bf16_t, true, false); }  \
      else     { if (cos) LAUNCH(bf16_t, false, true); else LAUNCH(bf16_t, false, false); }\
    }                                                                                     \
  } while (0)

extern "C" int lgs_supcon_forward(const void *feat, int64_t n, int c, const int64_t *labels, const int64_t *pos_idx, int p,
                                  const int64_t *neg_idx, int k, int64_t ignore_label, int n_labels, int distance, float *d_pos,
                                  float *d_neg, float *sim, float *inv_norm, int dtype, void *stream) {
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_supcon_forward: unknown dtype");
  LGS_REQUIRE(distance == LGS_SUPCON_COS || distance == LGS_SUPCON_L2, "lgs_supcon_forward: distance must be LGS_SUPCON_COS or LGS_SUPCON_L2");
  LGS_REQUIRE(n >= 0 && c >= 1 && n_labels >= 1, "lgs_supcon_forward: bad sizes");
  LGS_REQUIRE(p >= 1 && p <= kSupMaxS && k >= 1 && k <= kSupMaxS, "lgs_supcon_forward: P and K must be 1 .. 8");
  if (n == 0) return 0;
  LGS_REQUIRE(feat && labels && pos_idx && neg_idx && d_pos && d_neg && sim && inv_norm, "lgs_supcon_forward: null argument");
  LGS_REQUIRE((n + kSupWaves - 1) / kSupWaves <= 0x7fffffffll, "lgs_supcon_forward: too many rows");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)((n + kSupWaves - 1) / kSupWaves);
  const bool vec = sup_vec_ok(feat, nullptr, c, dtype), cos = distance == LGS_SUPCON_COS;
#define LGS_SUP_FWD(T_, V_, C_)                                                                                                    \
  LGS_KLAUNCH((k_supcon_fwd<T_, V_, C_>), grid, 64 * kSupWaves, 0, s, (const T_ *)feat, n, c, labels, pos_idx, p, neg_idx, k, ignore_label, \
              n_labels, d_pos, d_neg, sim, inv_norm)
  LGS_SUP_DISPATCH(LGS_SUP_FWD);
#undef LGS_SUP_FWD
  LGS_HIP(hipGetLastError());
  return 0;
}

extern "C" int lgs_supcon_backward(const void *feat, int64_t n, int c, const int64_t *labels, const int64_t *pos_idx, int p,
                                   const int64_t *neg_idx, int k, int64_t ignore_label, int n_labels, int distance, const float *sim,
                                   const float *inv_norm, const float *g_dpos, const float *g_dneg, void *grad_feat, int dtype,
                                   void *stream) {
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_supcon_backward: unknown dtype");
  LGS_REQUIRE(distance == LGS_SUPCON_COS || distance == LGS_SUPCON_L2, "lgs_supcon_backward: distance must be LGS_SUPCON_COS or LGS_SUPCON_L2");
  LGS_REQUIRE(n >= 0 && c >= 1 && n_labels >= 1, "lgs_supcon_backward: bad sizes");
  LGS_REQUIRE(p >= 1 && p <= kSupMaxS && k >= 1 && k <= kSupMaxS, "lgs_supcon_backward: P and K must be 1 .. 8");
  if (n == 0) return 0;
  LGS_REQUIRE(feat && labels && pos_idx && neg_idx && sim && inv_norm && grad_feat, "lgs_supcon_backward: null argument");
  LGS_REQUIRE((n + kSupWaves - 1) / kSupWaves <= 0x7fffffffll, "lgs_supcon_backward: too many rows");
  hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)((n + kSupWaves - 1) / kSupWaves);
  const bool vec = sup_vec_ok(feat, grad_feat, c, dtype), cos = distance == LGS_SUPCON_COS;
#define LGS_SUP_BWD(T_, V_, C_)                                                                                                    \
  LGS_KLAUNCH((k_supcon_bwd<T_, V_, C_>), grid, 64 * kSupWaves, 0, s, (const T_ *)feat, n, c, labels, pos_idx, p, neg_idx, k, ignore_label, \
              n_labels, sim, inv_norm, g_dpos, g_dneg, (T_ *)grad_feat)
  LGS_SUP_DISPATCH(LGS_SUP_BWD);
#undef LGS_SUP_BWD
  LGS_HIP(hipGetLastError());
  return 0;
}
