// lgs_normmath.h -- the arithmetic of the BatchNorm kernels (lgs_norm.hip), each expression once.
//
// Contraction is off in this header and in lgs_norm.hip: where a multiply and an add are one rounding it says so with an explicit
// fma, so the forward output and the ReLU mask the backward recomputes from x are the same bits by construction, the pair kernels
// are the single kernels' arithmetic by construction, and no compiler choice moves a result.  Which operations are fused is what
// the code objects computed before this header existed (profiles/norm_arith.txt has the table).
#pragma once
#include "lgs_common.h"

namespace lgs {
#if defined(__HIPCC__)
#pragma clang fp contract(off)

// ---- per element
// the forward output before the residual add and the ReLU; the backward's mode-2 mask is the sign of this same value
__device__ inline float bn_out(float x, float mean, float sc, float bt) { return __builtin_fmaf(x - mean, sc, bt); }

// dx = gi * (dy' - m1 - xhat * m2).  FMA: the last two operations are one fma.  They are everywhere but in the fp32 instance of the
// three-launch apply (and the pair kernel that stands for it), whose code object rounded the product.
enum BwdKernel { kBwdThree, kBwdFold, kBwdFused };
template <typename T, BwdKernel K> constexpr bool kDxFma = !(K == kBwdThree && sizeof(T) == 4);
template <bool FMA> __device__ inline float bn_dx(float x, float g, float mean, float istd, float gi, float m1, float m2) {
  const float xh = (x - mean) * istd, u = g - m1;
  return gi * (FMA ? __builtin_fmaf(-xh, m2, u) : u - xh * m2);
}

// one row's contribution to the column sums.  Forward: about the pivot.  Backward: g is the masked gradient.
__device__ inline void bn_acc_fwd(float x, float pivot, float &s0, float &s1) {
  const float d = x - pivot;
  s0 += d; s1 = __builtin_fmaf(d, d, s1);
}
__device__ inline void bn_acc_bwd(float g, float x, float mean, float istd, float &s0, float &s1) {
  s0 += g; s1 = __builtin_fmaf(g * (x - mean), istd, s1);
}

// ---- per channel, in double: the statistics from the two column sums about the pivot
__device__ inline double bn_shift(double s, int64_t n) { return n > 0 ? s / (double)n : 0.0; }      // mean - pivot
struct BnMoments { double mean, var; float istd; };       // mean and var stay double: the running statistics take them so
__device__ inline BnMoments bn_finish(double s, double ss, int64_t n, double pivot, float eps) {
  const double dm = bn_shift(s, n);
  double var = n > 0 ? __builtin_fma(-dm, dm, ss / (double)n) : 0.0;
  if (var < 0.0) var = 0.0;
  return {pivot + dm, var, (float)(1.0 / sqrt(var + (double)eps))};
}
__device__ inline void bn_update_running(float &running_mean, float &running_var, float momentum, double mean, double unbiased) {
  running_mean = (float)__builtin_fma((double)momentum, mean, (1.0 - momentum) * running_mean);
  running_var = (float)__builtin_fma((double)momentum, unbiased, (1.0 - momentum) * running_var);
}
__device__ inline void bn_update_running(float &running_mean, float &running_var, float momentum, const BnMoments &m, int64_t n) {
  bn_update_running(running_mean, running_var, momentum, m.mean, n > 1 ? m.var * (double)n / (double)(n - 1) : m.var);
}

// ---- the per-channel constants a thread keeps for its W channels [ch0, ch0 + W)
template <int W> struct BnFwdConsts {
  float mean[W], sc[W], bt[W];
  __device__ void set(int k, float m, float istd, float gamma, float beta) { mean[k] = m; sc[k] = istd * gamma; bt[k] = beta; }
  // M::ld: how a statistic is read (a plain load, or the agent-scope load of a kernel whose other workgroups wrote it)
  template <typename M> __device__ void load(const float *stats, const float *gamma, const float *beta, int c, int ch0) {
#pragma unroll
    for (int k = 0; k < W; ++k) set(k, M::ld(stats + ch0 + k), M::ld(stats + c + ch0 + k), gamma[ch0 + k], beta[ch0 + k]);
  }
  __device__ float out(int k, float x) const { return bn_out(x, mean[k], sc[k], bt[k]); }
};
template <int W> struct BnBwdConsts {
  float mean[W], istd[W], sc[W], bt[W], gi[W], m1[W], m2[W];
  // what the column sums and the mode-2 mask need (relu == 2: gamma and beta are read; otherwise they may be NULL)
  __device__ void norm(int k, const float *stats, const float *gamma, const float *beta, int c, int ch, int relu) {
    mean[k] = stats[ch]; istd[k] = stats[c + ch];
    sc[k] = istd[k] * (relu == 2 ? gamma[ch] : 0.f);
    bt[k] = relu == 2 ? beta[ch] : 0.f;
  }
  __device__ void load_norm(const float *stats, const float *gamma, const float *beta, int c, int ch0, int relu) {
#pragma unroll
    for (int k = 0; k < W; ++k) norm(k, stats, gamma, beta, c, ch0 + k, relu);
  }
  // ... and what dx needs on top.  s, ss: the two column sums of the W channels, as the fold stored them (read from the `sums` row,
  // plainly or at agent scope, or taken from the workgroup's own fold of the partial rows)
  __device__ void load(const float *stats, const float *gamma, const float *beta, int c, int ch0, int relu, float inv_n,
                       const float (&s)[W], const float (&ss)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      norm(k, stats, gamma, beta, c, ch0 + k, relu);
      gi[k] = gamma[ch0 + k] * istd[k];
      m1[k] = s[k] * inv_n; m2[k] = ss[k] * inv_n;
    }
  }
  // the forward output again (without the residual): relu mode 2 masks dy by its sign.  The two select loops (mode 1 by the stored
  // output, mode 2 by this) stay at their sites: as one function over a row's arrays this compiler shared the last element's select
  // between the modes and lost its mode-1 operand in the column reductions (tests/test_gpu_norm_bits.py, every mode-1 case).
  __device__ float out(int k, float x) const { return bn_out(x, mean[k], sc[k], bt[k]); }
  template <bool FMA> __device__ float dx(int k, float x, float g) const { return bn_dx<FMA>(x, g, mean[k], istd[k], gi[k], m1[k], m2[k]); }
};
#endif
}  // namespace lgs
