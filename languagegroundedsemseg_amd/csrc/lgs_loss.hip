// lgs_loss.hip -- fused softmax cross-entropy (forward + gradient in one pass) over [N, C] logits, gfx950.
//
// Replaces nn.CrossEntropyLoss(ignore_index=-1) on the [N,200] logits of the fine-tune step
//   /root/reference/lib/train_test/pl_BaselineTrainer.py:94-99,350
// HBM-bound: logits are read once (16-byte loads, half a wavefront per row), the per-row loss and the
// gradient (softmax - onehot) * scale are written in the same pass; ignored rows produce 0 / zeros.
#include "lgs_classrows.h"

namespace lgs {

// The access shape of lgs_classrows.h (half a wave per row, R rows per half-wave with every load issued first, Q x R = 4) plus the
// per-row lse - z_l and the gradient (softmax - onehot) * scale.  Element-wise rows pad with -3e38 -> exp = 0.
template <typename T, int Q, int R>
__global__ __launch_bounds__(256) void k_ce_fwd_bwd(const T *__restrict__ logits, int64_t n, int c, const int64_t *__restrict__ labels,
                                                    int64_t ignore_index, const float *__restrict__ scale_ptr,
                                                    const float *__restrict__ row_scale, float *__restrict__ loss_rows,
                                                    T *__restrict__ dlogits) {
  constexpr int W = Width<T>::V;
  const int lane = threadIdx.x & 31;  // half-wave per row group
  const int64_t row0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5) * R;
  if (row0 >= n) return;
  // class counts that are not a multiple of the 16-byte width (e.g. the 20 ScanNet classes in bf16) take
  // element-wise loads / stores for their rows: kernel-uniform branch, padding lanes hold -inf -> exp = 0
  const bool vec = (c % W) == 0;
  const int nchunk = (c + W - 1) / W;
  float v[R][Q][W];
  int64_t labs[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    labs[r] = row < n ? labels[row] : -1;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk && row < n) {
        if (vec) {
          ldv<W>(logits + row * c + ch * W, v[r][q]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i) v[r][q][i] = ch * W + i < c ? ld_elem(logits + row * c + ch * W + i) : -3.0e38f;
        }
      }
    }
  }
  const float scale0 = dlogits ? *scale_ptr : 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    if (row >= n) break;              // (uniform per half-wave: the shuffles below stay inside it)
    const int64_t lab = labs[r];
    const bool ignored = (lab == ignore_index) || lab < 0 || lab >= c;
    const int lab32 = ignored ? -1 : (int)lab;          // (32-bit compares against compile-time element offsets below)
    float mx = -3.0e38f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk) {
#pragma unroll
        for (int i = 0; i < W; ++i) mx = fmaxf(mx, v[r][q][i]);
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 32));
    float se = 0.f, xl = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk) {
        const int rel = lab32 - ch * W;
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const float e = __expf(v[r][q][i] - mx);
          se += e;
          if (i == rel) xl = v[r][q][i];
          v[r][q][i] = e;
        }
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { se += __shfl_xor(se, o, 32); xl += __shfl_xor(xl, o, 32); }
    const float lse = mx + __logf(se);
    if (loss_rows && lane == 0) loss_rows[row] = ignored ? 0.f : (lse - xl);
    if (!dlogits) continue;   // loss only (the gradient is produced by a second call in the backward pass)
    // row_scale: per-row upstream gradient of a reduction='none' loss (balanced category sampling: mask / N), times *scale_ptr
    const float scale = ignored ? 0.f : (row_scale ? scale0 * row_scale[row] : scale0);
    const float inv = scale / se;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk) {
        const int rel = lab32 - ch * W;
#pragma unroll
        for (int i = 0; i < W; ++i) {
          float g = v[r][q][i] * inv;
          if (i == rel) g -= scale;
          v[r][q][i] = g;
        }
        if (vec) {
          stv<W>(dlogits + row * c + ch * W, v[r][q]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i)
            if (ch * W + i < c) stv<1>(dlogits + row * c + ch * W + i, &v[r][q][i]);
        }
      }
    }
  }
}

// rows the mean cross-entropy counts: integer atomics, one per workgroup -> deterministic
__global__ __launch_bounds__(256) void k_ce_count_valid(const int64_t *__restrict__ labels, int64_t n, int c, int64_t ignore_index,
                                                         int32_t *__restrict__ count) {
  __shared__ int32_t l_cnt;
  if (threadIdx.x == 0) l_cnt = 0;
  __syncthreads();
  int32_t mine = 0;
  const int64_t base = (int64_t)blockIdx.x * 256 * 8;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t r = base + (int64_t)i * 256 + threadIdx.x;
    if (r < n) {
      const int64_t lab = labels[r];
      mine += (lab != ignore_index && lab >= 0 && lab < c) ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&l_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0 && l_cnt) atomicAdd(count, l_cnt);
}

// head / common / tail statistics of the per-point losses (lib/losses/utils.py:69-72: loss[loss_items[:, g]] for the trainer's three
// meters, pl_BaselineTrainer.py:353-355) without the boolean-index gathers: per workgroup the sums and counts of the three groups
// -> partial[block][6]; the caller adds the <= 1024 rows up (deterministic, no float atomics).  One streaming pass: 12 B per point.
__global__ __launch_bounds__(256) void k_split_stats(const float *__restrict__ loss, const int64_t *__restrict__ labels, int64_t n,
                                                     const int32_t *__restrict__ group_of_class, int n_classes, int64_t ignore_index,
                                                     float *__restrict__ partial) {
  __shared__ float l_acc[4][6];
  float sum[3] = {0.f, 0.f, 0.f}, cnt[3] = {0.f, 0.f, 0.f};
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const int64_t lab = labels[r];
    if (lab == ignore_index || lab < 0 || lab >= n_classes) continue;
    const int g = group_of_class[lab];
    const float v = loss[r];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sum[k] += g == k ? v : 0.f;
      cnt[k] += g == k ? 1.f : 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      sum[k] += __shfl_down(sum[k], o, 64);
      cnt[k] += __shfl_down(cnt[k], o, 64);
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { l_acc[wave][2 * k] = sum[k]; l_acc[wave][2 * k + 1] = cnt[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 6)
    partial[(int64_t)blockIdx.x * 6 + threadIdx.x] = l_acc[0][threadIdx.x] + l_acc[1][threadIdx.x] + l_acc[2][threadIdx.x] + l_acc[3][threadIdx.x];
}

}  // namespace lgs

using namespace lgs;

extern "C" int lgs_split_stats(const float *loss_rows, const int64_t *labels, int64_t n, const int32_t *group_of_class, int n_classes,
                               int64_t ignore_index, float *partial, int partial_rows, void *stream) {
  LGS_REQUIRE(partial && group_of_class && n >= 0 && n_classes >= 1 && partial_rows >= 1 && partial_rows <= 1024 &&
                  ((loss_rows && labels) || n == 0),
              "lgs_split_stats: bad argument");
  LGS_KLAUNCH(k_split_stats, (unsigned)partial_rows, 256, 0, (hipStream_t)stream, loss_rows, labels, n, group_of_class, n_classes,
              ignore_index, partial);
  LGS_HIP(hipGetLastError());
  return 0;
}

extern "C" int lgs_ce_forward_backward_rows(const void *logits, int64_t n, int c, const int64_t *labels, int64_t ignore_index,
                                            const float *scale, const float *row_scale, float *loss_rows, void *dlogits, int dtype,
                                            void *stream) {
  LGS_REQUIRE(logits && labels && scale && (loss_rows || dlogits), "lgs_ce_forward_backward: null argument");
  int q;
  if (int rc = class_shape(c, dtype, "lgs_ce_forward_backward", &q)) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int rc = with_class_rows<1>(dtype, q, 0, "lgs_ce_forward_backward", [&](auto e, auto) {
    using E = decltype(e);
    LGS_KLAUNCH((k_ce_fwd_bwd<typename E::T, E::Q, E::R>), (unsigned)e.tiles(n), 256, 0, s, e.in(logits), n, c, labels, ignore_index, scale,
                row_scale, loss_rows, e.out(dlogits));
    return 0;
  });
  if (rc) return rc;
  LGS_HIP(hipGetLastError());
  return 0;
}

int lgs_ce_forward_backward(const void *logits, int64_t n, int c, const int64_t *labels, int64_t ignore_index,
                            const float *scale, float *loss_rows, void *dlogits, int dtype, void *stream) {
  return lgs_ce_forward_backward_rows(logits, n, c, labels, ignore_index, scale, nullptr, loss_rows, dlogits, dtype, stream);
}

int lgs_ce_count_valid(const int64_t *labels, int64_t n, int c, int64_t ignore_index, int32_t *count, void *stream) {
  LGS_REQUIRE(count && (labels || n == 0) && n >= 0 && c >= 1, "lgs_ce_count_valid: bad argument");
  hipStream_t s = (hipStream_t)stream;
  LGS_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), s));
  if (n == 0) return 0;
  LGS_KLAUNCH(k_ce_count_valid, (unsigned)((n + 2047) / 2048), 256, 0, s, labels, n, c, ignore_index, count);
  LGS_HIP(hipGetLastError());
  return 0;
}

// ---- focal loss and class-weighted cross-entropy (lib/losses/FocalLoss.py, lib/utils.py:112-118 `loss_by_name`)
//   L = -a u^gamma log(pt),   dL/dz_j = coef (p_j - [j == l]),   coef = a (u^gamma - gamma pt u^(gamma-1) log(pt))
// with p = softmax(z), pt = p_l, u = 1 - pt, a = alpha[l] (1 without a table).  gamma == 0 is nn.CrossEntropyLoss(weight=alpha).
// The access shape of lgs_classrows.h like k_ce_fwd_bwd, the same two modes (loss_rows only / dlogits only) and the same bytes, plus
// alpha[label]: 4 B per row from a [C] table that stays in L2.  What differs is the per-row scalar part:
//   u       = se_excl / se, the exponential sum WITHOUT the label's term over the full one, accumulated in the same pass: never
//             1 - exp(log pt), which is 0 from pt = 1 - 6e-8 on;
//   log(pt) = log1p(-u) while u < 1/2 (the label dominates: (z_l - max) - log(se) is 0 - log(1 + 1e-11) = 0 there), else
//             (z_l - max) - log(se) (pt small: 1 - u would cancel);
//   the label's gradient entry is -coef u, not coef (pt - 1);
//   u^gamma: GM = 0 -> 1 (no pow), GM = 2 -> u u, GM = 1 -> exp2(gamma log2(u)); u^(gamma-1) = u^gamma / u; u == 0 takes the limit
//             (loss 0, coef = a for gamma == 0, else 0) where the reference's autograd gives 0^(gamma-1) = NaN for gamma < 1.
namespace lgs {

template <typename T, int Q, int R, int GM>
__global__ __launch_bounds__(256) void k_focal_fwd_bwd(const T *__restrict__ logits, int64_t n, int c, const int64_t *__restrict__ labels,
                                                       int64_t ignore_index, const float *__restrict__ alpha, float gamma,
                                                       const float *__restrict__ scale_ptr, const float *__restrict__ row_scale,
                                                       float *__restrict__ loss_rows, T *__restrict__ dlogits) {
  constexpr int W = Width<T>::V;
  const int lane = threadIdx.x & 31;  // half-wave per row group
  const int64_t row0 = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 5) * R;
  if (row0 >= n) return;
  const bool vec = (c % W) == 0;      // kernel-uniform, as in k_ce_fwd_bwd: padding lanes of the element-wise rows hold -3e38 -> exp = 0
  const int nchunk = (c + W - 1) / W;
  float v[R][Q][W];
  int lab32s[R];
  float as[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    const int64_t lab = row < n ? labels[row] : -1;
    const bool ignored = (lab == ignore_index) || lab < 0 || lab >= c;
    lab32s[r] = ignored ? -1 : (int)lab;
    as[r] = (alpha && !ignored) ? alpha[lab] : 1.f;    // (the only read of the table: at a label inside [0, C))
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk && row < n) {
        if (vec) {
          ldv<W>(logits + row * c + ch * W, v[r][q]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i) v[r][q][i] = ch * W + i < c ? ld_elem(logits + row * c + ch * W + i) : -3.0e38f;
        }
      }
    }
  }
  const float scale0 = dlogits ? *scale_ptr : 0.f;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    if (row >= n) break;              // (uniform per half-wave: the shuffles below stay inside it)
    const int lab32 = lab32s[r];
    const bool ignored = lab32 < 0;
    float mx = -3.0e38f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk) {
#pragma unroll
        for (int i = 0; i < W; ++i) mx = fmaxf(mx, v[r][q][i]);
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 32));
    float se = 0.f, sx = 0.f, xl = 0.f;     // sx: the sum without the label's term
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk) {
        const int rel = lab32 - ch * W;
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const float e = __expf(v[r][q][i] - mx);
          se += e;
          sx += i == rel ? 0.f : e;
          if (i == rel) xl = v[r][q][i];
          v[r][q][i] = e;
        }
      }
    }
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) { se += __shfl_xor(se, o, 32); sx += __shfl_xor(sx, o, 32); xl += __shfl_xor(xl, o, 32); }
    const float a = as[r];
    const float rse = 1.f / se;
    const float u = sx * rse;
    const float log_pt = u < 0.5f ? log1pf(-u) : (xl - mx) - __logf(se);
    float loss, coef;
    if constexpr (GM == 0) {
      loss = -a * log_pt;
      coef = a;
    } else if constexpr (GM == 2) {
      const float pt = __expf(xl - mx) * rse;
      loss = -a * u * u * log_pt;
      coef = a * (u * u - 2.f * pt * u * log_pt);
    } else {
      const float pt = __expf(xl - mx) * rse;
      const float ug = exp2f(gamma * __log2f(u));
      loss = u > 0.f ? -a * ug * log_pt : 0.f;
      coef = u > 0.f ? a * (ug - gamma * pt * (ug / u) * log_pt) : 0.f;
    }
    if (loss_rows && lane == 0) loss_rows[row] = ignored ? 0.f : loss;
    if (!dlogits) continue;   // loss only (the gradient is produced by a second call in the backward pass)
    // ignored rows: an exact 0 whatever coef came out of a row without a label (its pt is exp(-max) / se)
    const float cs = ignored ? 0.f : coef * (row_scale ? scale0 * row_scale[row] : scale0);
    const float inv = cs * rse, at_label = -cs * u;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int ch = q * 32 + lane;
      if (ch < nchunk) {
        const int rel = lab32 - ch * W;
#pragma unroll
        for (int i = 0; i < W; ++i) v[r][q][i] = i == rel ? at_label : v[r][q][i] * inv;
        if (vec) {
          stv<W>(dlogits + row * c + ch * W, v[r][q]);
        } else {
#pragma unroll
          for (int i = 0; i < W; ++i)
            if (ch * W + i < c) stv<1>(dlogits + row * c + ch * W + i, &v[r][q][i]);
        }
      }
    }
  }
}

// sum of alpha[label] over the counted rows: the denominator of nn.CrossEntropyLoss(weight=alpha) 'mean'.  Per workgroup one float
// -> partial[block]; the caller adds the <= 1024 rows up in fixed order (the pattern of k_split_stats: deterministic, no float atomics)
__global__ __launch_bounds__(256) void k_ce_weight_sum(const int64_t *__restrict__ labels, int64_t n, int c, int64_t ignore_index,
                                                        const float *__restrict__ alpha, float *__restrict__ partial) {
  __shared__ float l_acc[4];
  float sum = 0.f;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const int64_t lab = labels[r];
    if (lab == ignore_index || lab < 0 || lab >= c) continue;
    sum += alpha[lab];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if ((threadIdx.x & 63) == 0) l_acc[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = l_acc[0] + l_acc[1] + l_acc[2] + l_acc[3];
}

}  // namespace lgs

extern "C" int lgs_focal_forward_backward(const void *logits, int64_t n, int c, const int64_t *labels, int64_t ignore_index,
                                          const float *alpha, float gamma, const float *scale, const float *row_scale,
                                          float *loss_rows, void *dlogits, int dtype, void *stream) {
  LGS_REQUIRE(logits && labels && scale && (loss_rows || dlogits), "lgs_focal_forward_backward: null argument");
  LGS_REQUIRE(gamma >= 0.f, "lgs_focal_forward_backward: gamma must be >= 0");
  int q;
  if (int rc = class_shape(c, dtype, "lgs_focal_forward_backward", &q)) return rc;
  LGS_REQUIRE(n >= 0, "lgs_focal_forward_backward: negative row count");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  // GM: 0 = weighted cross-entropy, 2 = u u, 1 = any other gamma
  const int rc = with_class_rows<3>(dtype, q, gamma == 0.f ? 0 : gamma == 2.f ? 2 : 1, "lgs_focal_forward_backward", [&](auto e, auto gm) {
    using E = decltype(e);
    LGS_KLAUNCH((k_focal_fwd_bwd<typename E::T, E::Q, E::R, decltype(gm)::value>), (unsigned)e.tiles(n), 256, 0, s, e.in(logits), n, c,
                labels, ignore_index, alpha, gamma, scale, row_scale, loss_rows, e.out(dlogits));
    return 0;
  });
  if (rc) return rc;
  LGS_HIP(hipGetLastError());
  return 0;
}

extern "C" int lgs_ce_weight_sum(const int64_t *labels, int64_t n, int c, int64_t ignore_index, const float *alpha, float *partial,
                                 int partial_rows, void *stream) {
  LGS_REQUIRE(partial && alpha && n >= 0 && c >= 1 && partial_rows >= 1 && partial_rows <= 1024 && (labels || n == 0),
              "lgs_ce_weight_sum: bad argument");
  LGS_KLAUNCH(k_ce_weight_sum, (unsigned)partial_rows, 256, 0, (hipStream_t)stream, labels, n, c, ignore_index, alpha, partial);
  LGS_HIP(hipGetLastError());
  return 0;
}

// ---- backward of the fused CLIP text-anchor loss (lgs_clip_loss_forward)
//   /root/reference/lib/losses/ContrastiveLanguageLoss.py:73-95 (feat_dist, cos branch) through autograd:
// only 1 + K entries of a row of S = f^ . T^^T carry gradient, so instead of two dense [N, A] x [A, C] products
//   gf = ( sum_j gs_j t^_j  -  (sum_j gs_j s_j) f^ ) / |f|,      gs_pos = -g_dpos,  gs_neg_j = -g_dneg / K
// is a pure streaming pass: read f once, gather 1 + K normalised anchor rows (L2-resident table), write gf once.
// sum_j gs_j s_j needs only s_pos = 1 - d_pos and mean_j s_neg_j = 1 - d_neg, both saved by the forward.
namespace lgs {
template <typename T>
__global__ __launch_bounds__(256) void k_clip_loss_bwd(const T *__restrict__ feat, int64_t n, int c, const float *__restrict__ tn,
                                                       int n_anchor, const int64_t *__restrict__ labels,
                                                       const int64_t *__restrict__ neg, int k_neg, int64_t ignore,
                                                       const float *__restrict__ inv_norm, const float *__restrict__ d_pos,
                                                       const float *__restrict__ d_neg, const float *__restrict__ g_dpos,
                                                       const float *__restrict__ g_dneg, T *__restrict__ gf) {
  constexpr int W = Width<T>::V;
  const int G = c / W;                       // 16-byte channel groups per row
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = idx / G;
  const int g = (int)(idx - row * G);
  if (row >= n) return;
  float fv[W], out[W];
  ldv<W>(feat + row * c + g * W, fv);
  const int64_t lab = labels[row];
  const bool valid = lab != ignore && lab >= 0 && lab < n_anchor;
#pragma unroll
  for (int i = 0; i < W; ++i) out[i] = 0.f;
  if (valid) {
    const float inv = inv_norm[row];
    const float gp = g_dpos ? -g_dpos[row] : 0.f;
    const float gn = g_dneg ? -g_dneg[row] / (float)k_neg : 0.f;
    const float sigma = gp * (1.f - d_pos[row]) + gn * (float)k_neg * (1.f - d_neg[row]);
    const float *tp = tn + lab * c + g * W;
#pragma unroll
    for (int i = 0; i < W; i += 4) {
      const float4 t = *reinterpret_cast<const float4 *>(tp + i);
      out[i] = gp * t.x; out[i + 1] = gp * t.y; out[i + 2] = gp * t.z; out[i + 3] = gp * t.w;
    }
    for (int j = 0; j < k_neg; ++j) {
      const int64_t a = neg[row * k_neg + j];
      if (a < 0 || a >= n_anchor) continue;
      const float *tq = tn + a * c + g * W;
#pragma unroll
      for (int i = 0; i < W; i += 4) {
        const float4 t = *reinterpret_cast<const float4 *>(tq + i);
        out[i] += gn * t.x; out[i + 1] += gn * t.y; out[i + 2] += gn * t.z; out[i + 3] += gn * t.w;
      }
    }
    const float si = sigma * inv;
#pragma unroll
    for (int i = 0; i < W; ++i) out[i] = (out[i] - si * fv[i]) * inv;
  }
  stv<W>(gf + row * c + g * W, out);
}
}  // namespace lgs

extern "C" int lgs_clip_loss_backward(const void *feat, int64_t n, int c, const float *anchors_n, int n_anchor,
                                      const int64_t *labels, const int64_t *neg, int k_neg, int64_t ignore_label,
                                      const float *inv_norm_f, const float *d_pos, const float *d_neg, const float *g_dpos,
                                      const float *g_dneg, void *grad_feat, int dtype, void *stream) {
  LGS_REQUIRE(feat && anchors_n && labels && neg && inv_norm_f && d_pos && d_neg && grad_feat, "lgs_clip_loss_backward: null argument");
  const int W = dtype == LGS_BF16 ? 8 : 4;
  LGS_REQUIRE(c % W == 0 && k_neg >= 1, "lgs_clip_loss_backward: feature dim must be a multiple of the 16-byte load width");
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t threads = n * (int64_t)(c / W);
  const unsigned blocks = (unsigned)((threads + 255) / 256);
  if (dtype == LGS_F32)
    LGS_KLAUNCH((k_clip_loss_bwd<float>), blocks, 256, 0, s, (const float *)feat, n, c, anchors_n, n_anchor, labels, neg, k_neg,
                       ignore_label, inv_norm_f, d_pos, d_neg, g_dpos, g_dneg, (float *)grad_feat);
  else if (dtype == LGS_BF16)
    LGS_KLAUNCH((k_clip_loss_bwd<bf16_t>), blocks, 256, 0, s, (const bf16_t *)feat, n, c, anchors_n, n_anchor, labels, neg,
                       k_neg, ignore_label, inv_norm_f, d_pos, d_neg, g_dpos, g_dneg, (bf16_t *)grad_feat);
  else
    LGS_REQUIRE(false, "lgs_clip_loss_backward: unknown dtype");
  LGS_HIP(hipGetLastError());
  return 0;
}

// ---- fused SGD step on a flat bucket (torch.optim.SGD's rule, /root/reference/lib/solvers.py: momentum 0.9,
// dampening 0.1, weight decay 1e-4): d = g + wd * p;  buf = first ? d : m * buf + (1 - damp) * d;  p -= lr * mask * buf
// one pass over the bucket instead of four elementwise kernels
namespace lgs {
__global__ void k_sgd_step(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ buf,
                           const float *__restrict__ mask, int64_t n, float lr, float momentum, float dampening, float wd,
                           int first) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n) {
    float4 pv = *reinterpret_cast<float4 *>(p + i);
    const float4 gv = *reinterpret_cast<const float4 *>(g + i);
    float4 bv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<float4 *>(buf + i);
    float4 mv = mask ? *reinterpret_cast<const float4 *>(mask + i) : make_float4(1.f, 1.f, 1.f, 1.f);
    float d;
#define LGS_SGD1(c)                                                                  \
    d = gv.c + wd * pv.c;                                                             \
    bv.c = momentum != 0.f ? (first ? d : momentum * bv.c + (1.f - dampening) * d) : d; \
    pv.c -= lr * mv.c * bv.c;
    LGS_SGD1(x) LGS_SGD1(y) LGS_SGD1(z) LGS_SGD1(w)
#undef LGS_SGD1
    if (momentum != 0.f) *reinterpret_cast<float4 *>(buf + i) = bv;
    *reinterpret_cast<float4 *>(p + i) = pv;
  } else {
    for (int64_t j = i; j < n; ++j) {
      const float d = g[j] + wd * p[j];
      float b = momentum != 0.f ? (first ? d : momentum * buf[j] + (1.f - dampening) * d) : d;
      if (momentum != 0.f) buf[j] = b;
      p[j] -= lr * (mask ? mask[j] : 1.f) * b;
    }
  }
}
}  // namespace lgs

extern "C" int lgs_sgd_step(float *params, const float *grads, float *momentum_buf, const float *mask, int64_t n, float lr,
                            float momentum, float dampening, float weight_decay, int first_step, void *stream) {
  LGS_REQUIRE(n >= 0 && (n == 0 || (params && grads && (momentum == 0.f || momentum_buf))), "lgs_sgd_step: bad argument");
  LGS_REQUIRE(((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(momentum_buf) |
                reinterpret_cast<uintptr_t>(mask)) & 15u) == 0, "lgs_sgd_step: buffers must be 16-byte aligned");
  if (n == 0) return 0;
  const int64_t threads = (n + 3) / 4;
  LGS_KLAUNCH(lgs::k_sgd_step, (unsigned)((threads + 255) / 256), 256, 0, (hipStream_t)stream, params, grads, momentum_buf,
                     mask, n, lr, momentum, dampening, weight_decay, first_step);
  LGS_HIP(hipGetLastError());
  return 0;
}
