// lgs_norm.hip -- fused BatchNorm (+ residual add) (+ ReLU) over sparse-tensor rows, gfx950.
//
// Replaces ME.MinkowskiBatchNorm (.bn = nn.BatchNorm1d on .F), MinkowskiReLU and `out += residual`
//   /root/reference/models/modules/common.py:17-19          get_norm()
//   /root/reference/models/modules/resnet_block.py:41-57     conv -> norm -> relu -> conv -> norm -> += -> relu
//   /root/reference/models/res16unet.py:196-270              conv -> bn -> relu chains
//
// Pure HBM-bound streaming work: features are [N, C] row-major with C in
// {32..512}; a thread owns a fixed group of 4 (fp32) or 8 (bf16) adjacent channels = one 16-byte
// access (ldv / stv / stv_nt of lgs_rows.h, always at full width: C is a multiple of it) and walks rows,
// so every wave instruction is a fully coalesced 1 KiB access.  Statistics
// are reduced per block in LDS, then across blocks through a [blocks, 2C] fp32 scratch that a small fold
// kernel sums in a fixed order (double accumulation) -> deterministic, no float atomics.
// Passes over a [N, C] tensor per call (`three` / `fold` paths): forward 3 (read x twice, write y; 4 with a residual), backward 5
// (x, dy twice, dx written), 7 with a ReLU mask from y and a residual gradient out -- the reduce launch writes the masked
// gradient and the apply reads it back, so y is read and dy masked once.  The two norms that meet at the residual add of a
// downsample block share their passes (lgs_bn_forward_pair / lgs_bn_backward_pair, below): 5 forward and 10 backward for both.
// Every floating-point expression of these kernels is a function of lgs_normmath.h; contraction is off here as it is there.
#include "lgs_normmath.h"
#include "lgs_rows.h"
#include <algorithm>
#include <atomic>
#include <mutex>

#pragma clang fp contract(off)

namespace lgs {

constexpr int kNT = 256;

// a value as it reads back after a store in T (bf16: rounded; fp32: itself)
template <typename T> __device__ inline float stored_value(float x);
template <> __device__ inline float stored_value<float>(float x) { return x; }
template <> __device__ inline float stored_value<bf16_t>(float x) { return bf16_to_f32(f32_to_bf16(x)); }

// How a float that crosses workgroups is moved.  Between launches: plainly.  Inside a fused kernel (scratch rows, statistics):
// with agent-scope accesses (sc1: coherent across the eight XCDs' L2s) instead of fencing -- a release / acquire fence at agent
// scope writes back and invalidates the whole L2 of the XCD, and 512 workgroups doing that twice cost 0.24 ms per launch.
__device__ inline void st_coh(float *p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline float ld_coh(const float *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <bool COH> struct Mem {
  __device__ static float ld(const float *p) { if constexpr (COH) return ld_coh(p); else return *p; }
  __device__ static void st(float *p, float v) { if constexpr (COH) st_coh(p, v); else *p = v; }
};
// the 16-byte row store, non-temporal or not
template <bool NT, int W, typename T> __device__ inline void store_row(T *p, const float *v) {
  if constexpr (NT) stv_nt<W>(p, v); else stv<W>(p, v);
}

// Column reduction of up to two per-element quantities.  MODE 0: (x - pivot, (x - pivot)^2)  [forward statistics]
// MODE 1: (dy', dy' * xhat) where dy' = dy masked by (y > 0) when relu  [backward reductions]
// Each block handles a contiguous slab of rows; thread layout: cg = tid % G channel groups, rl = tid / G.
// out: scratch[blocks][2][C]
// relu: 0 = none, 1 = mask from the saved output y (needed when a residual was added), 2 = mask recomputed from x
// as (xhat * gamma + beta > 0) -- one tensor read fewer.
// gout (MODE 1, may be NULL): the masked gradient dy' is also written there, [n, c] contiguous -- exact in T (it is dy or 0), so
// the apply launch can read it back instead of masking dy a second time.
// PAIR (MODE 1): a second norm xb / stats_b (no ReLU of its own) receives the same dy': its two sums go to scratch_b; every
// operand is read once, and each norm's sums are taken exactly as a launch of its own would take them.
template <typename T, int MODE, bool PAIR>
__device__ inline void colreduce_rows(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ dy,
                                      const float *__restrict__ stats, const float *__restrict__ gamma,
                                      const float *__restrict__ beta, int64_t n, int c, int relu,
                                      int64_t rows_per_block, float *__restrict__ scratch, int64_t dy_ld, int64_t y_ld,
                                      T *__restrict__ gout, const T *__restrict__ xb, const float *__restrict__ stats_b,
                                      float *__restrict__ scratch_b) {
  static_assert(!PAIR || MODE == 1, "the forward pair reduces its two inputs in separate workgroups");
  constexpr int W = Width<T>::V;
  const int G = c / W;              // channel groups per row
  const int RL = kNT / G;           // rows in flight per block iteration (G <= 256)
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  const bool active = rl < RL;
  float s0[W], s1[W], q0[W], q1[W];          // q: the second norm's sums
#pragma unroll
  for (int i = 0; i < W; ++i) s0[i] = s1[i] = q0[i] = q1[i] = 0.f;
  float pivot[W];
  BnBwdConsts<W> k, kb;
  if (MODE == 1) {
    k.load_norm(stats, gamma, beta, c, cg * W, relu);
    if constexpr (PAIR) kb.load_norm(stats_b, nullptr, nullptr, c, cg * W, 0);
  } else {
    // forward statistics are accumulated about a per-channel pivot (row 0, the same for every block) so that
    // var = E[(x-k)^2] - E[x-k]^2 does not cancel catastrophically when |mean| >> std
    if (n > 0) ldv<W>(x + cg * W, pivot);
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(r0 + rows_per_block, n);
  if (active) {
    int64_t r = r0 + rl;
    // U rows per thread are in flight before the first is consumed (a streaming reduction needs ~50 KB of loads in
    // flight per CU to cover the HBM latency); sums are then taken in row order, i.e. exactly as a 1-row loop would
    constexpr int U = MODE == 0 ? 4 : 2;
    auto accumulate = [&](const float (&xv)[W], float (&gv)[W], const float (&yv)[W], const float (&xbv)[W], int64_t row) __attribute__((always_inline)) {
      if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < W; ++i) bn_acc_fwd(xv[i], pivot[i], s0[i], s1[i]);
      } else {
        if (relu == 1) {
#pragma unroll
          for (int i = 0; i < W; ++i) gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
        } else if (relu == 2) {
#pragma unroll
          for (int i = 0; i < W; ++i) gv[i] = k.out(i, xv[i]) > 0.f ? gv[i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < W; ++i) bn_acc_bwd(gv[i], xv[i], k.mean[i], k.istd[i], s0[i], s1[i]);
        if constexpr (PAIR) {
#pragma unroll
          for (int i = 0; i < W; ++i) bn_acc_bwd(gv[i], xbv[i], kb.mean[i], kb.istd[i], q0[i], q1[i]);
        }
        if (gout) stv<W>(gout + row * c + cg * W, gv);
      }
    };
    for (; r + (U - 1) * RL < r1; r += U * RL) {
      float xv[U][W], gv[U][W], yv[U][W], xbv[U][W];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t o = (r + u * RL) * c + cg * W;
        ldv<W>(x + o, xv[u]);
        if (MODE == 1) {
          ldv<W>(dy + (r + u * RL) * dy_ld + cg * W, gv[u]);
          if (relu == 1) ldv<W>(y + (r + u * RL) * y_ld + cg * W, yv[u]);
          if constexpr (PAIR) ldv<W>(xb + o, xbv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) accumulate(xv[u], gv[u], yv[u], xbv[u], r + u * RL);
    }
    for (; r < r1; r += RL) {
      float xv[W], gv[W], yv[W], xbv[W];
      const int64_t o = r * c + cg * W;
      ldv<W>(x + o, xv);
      if (MODE == 1) {
        ldv<W>(dy + r * dy_ld + cg * W, gv);
        if (relu == 1) ldv<W>(y + r * y_ld + cg * W, yv);
        if constexpr (PAIR) ldv<W>(xb + o, xbv);
      }
      accumulate(xv, gv, yv, xbv, r);
    }
  }
  // block reduction over rl through LDS
  __shared__ float red[2][kNT][8];
#pragma unroll
  for (int i = 0; i < W; ++i) { red[0][threadIdx.x][i] = s0[i]; red[1][threadIdx.x][i] = s1[i]; }
  __syncthreads();
  if (rl == 0) {
    for (int j = 1; j < RL; ++j) {
#pragma unroll
      for (int i = 0; i < W; ++i) { s0[i] += red[0][j * G + cg][i]; s1[i] += red[1][j * G + cg][i]; }
    }
    float *dst = scratch + (int64_t)blockIdx.x * 2 * c;
#pragma unroll
    for (int i = 0; i < W; ++i) { dst[cg * W + i] = s0[i]; dst[c + cg * W + i] = s1[i]; }
  }
  if constexpr (PAIR) {       // the same block reduction for the second norm's sums, through the same LDS
    __syncthreads();
#pragma unroll
    for (int i = 0; i < W; ++i) { red[0][threadIdx.x][i] = q0[i]; red[1][threadIdx.x][i] = q1[i]; }
    __syncthreads();
    if (rl == 0) {
      for (int j = 1; j < RL; ++j) {
#pragma unroll
        for (int i = 0; i < W; ++i) { q0[i] += red[0][j * G + cg][i]; q1[i] += red[1][j * G + cg][i]; }
      }
      float *dst = scratch_b + (int64_t)blockIdx.x * 2 * c;
#pragma unroll
      for (int i = 0; i < W; ++i) { dst[cg * W + i] = q0[i]; dst[c + cg * W + i] = q1[i]; }
    }
  }
}
template <typename T, int MODE>
__global__ __launch_bounds__(kNT) void k_colreduce(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ dy,
                                                   const float *__restrict__ stats, const float *__restrict__ gamma,
                                                   const float *__restrict__ beta, int64_t n, int c, int relu,
                                                   int64_t rows_per_block, float *__restrict__ scratch, int64_t dy_ld, int64_t y_ld,
                                                   T *__restrict__ gout) {
  colreduce_rows<T, MODE, false>(x, y, dy, stats, gamma, beta, n, c, relu, rows_per_block, scratch, dy_ld, y_ld, gout, nullptr, nullptr, nullptr);
}
// the two norms of a pair in one launch.  MODE 0: blockIdx.y picks the norm (two independent reductions, each exactly k_colreduce<T, 0>);
// MODE 1: both norms' sums from one read of xa, ya, dy, xb
template <typename T, int MODE>
__global__ __launch_bounds__(kNT) void k_colreduce_pair(const T *__restrict__ xa, const T *__restrict__ ya, const T *__restrict__ dy,
                                                        const float *__restrict__ stats_a, const float *__restrict__ gamma_a,
                                                        const float *__restrict__ beta_a, int64_t n, int c, int relu,
                                                        int64_t rows_per_block, float *__restrict__ scratch_a, int64_t dy_ld, int64_t y_ld,
                                                        T *__restrict__ gout, const T *__restrict__ xb, const float *__restrict__ stats_b,
                                                        float *__restrict__ scratch_b) {
  if constexpr (MODE == 0)
    colreduce_rows<T, 0, false>(blockIdx.y ? xb : xa, nullptr, nullptr, nullptr, nullptr, nullptr, n, c, 0, rows_per_block,
                                blockIdx.y ? scratch_b : scratch_a, c, c, nullptr, nullptr, nullptr, nullptr);
  else
    colreduce_rows<T, 1, true>(xa, ya, dy, stats_a, gamma_a, beta_a, n, c, relu, rows_per_block, scratch_a, dy_ld, y_ld, gout, xb, stats_b, scratch_b);
}

// fold the per-block partials (fixed order, deterministic) and finish: forward -> mean / invstd / running stats,
// backward -> dbeta = sum dy', dgamma = sum dy' xhat.  Block = 16 channels x 16 partial-slices: a thread sums every
// 16th partial with eight independent loads in flight (the fold is a pure latency chain: 4 slices of 128 dependent
// steps took 13 us per BatchNorm, twice per layer), slices are combined through LDS in slice order.
// COH (here and below): the step runs inside a fused kernel, on rows other workgroups of the same launch wrote and for them to read.
constexpr int kFoldCh = 16, kFoldSl = 16;
template <bool COH>
__device__ inline void fold_sums(const float *scratch, int nblocks, int c, int ch, int part, double &s, double &ss, double (*red)[2][kFoldCh]) {
  s = 0.0; ss = 0.0;
  if (ch < c) {
#pragma unroll 8
    for (int b = part; b < nblocks; b += kFoldSl) { s += Mem<COH>::ld(scratch + (int64_t)b * 2 * c + ch); ss += Mem<COH>::ld(scratch + (int64_t)b * 2 * c + c + ch); }
  }
  red[part][0][threadIdx.x % kFoldCh] = s;
  red[part][1][threadIdx.x % kFoldCh] = ss;
  __syncthreads();
  if (part == 0) {
    for (int q = 1; q < kFoldSl; ++q) { s += red[q][0][threadIdx.x % kFoldCh]; ss += red[q][1][threadIdx.x % kFoldCh]; }
  }
}
// statistics that arrive as per-tile partial rows from the conv epilogue (BnEpi): fold groups of rows into <= 128 rows
// of the same [row][2][C] layout, fixed order (deterministic).  Rows [r0, r1) of `part` -> out_row
constexpr int kPartialFoldRows = 128;
template <bool COH>
__device__ inline void partial_reduce_rows(const float *part, int r0, int r1, int c2, float *out_row) {
  for (int col = threadIdx.x; col < c2; col += blockDim.x) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
      a0 += part[(int64_t)(r + 0) * c2 + col]; a1 += part[(int64_t)(r + 1) * c2 + col];
      a2 += part[(int64_t)(r + 2) * c2 + col]; a3 += part[(int64_t)(r + 3) * c2 + col];
    }
    for (; r < r1; ++r) a0 += part[(int64_t)r * c2 + col];
    Mem<COH>::st(out_row + col, (a0 + a1) + (a2 + a3));
  }
}
__global__ __launch_bounds__(256) void k_partial_reduce(const float *__restrict__ part, int rows, int c2, int rows_per_block,
                                                        float *__restrict__ out) {
  const int r0 = blockIdx.x * rows_per_block;
  partial_reduce_rows<false>(part, r0, min(r0 + rows_per_block, rows), c2, out + (int64_t)blockIdx.x * c2);
}

// the per-channel pivot of forward sums.  pivot_mode 0: row 0 of x (k_colreduce<0>); 1: pivot_ptr[ch] (or 0 if NULL) -- conv-epilogue partials
template <typename T> __device__ inline double fold_pivot(const T *x, int64_t n, int ch, int pivot_mode, const float *pivot_ptr) {
  return pivot_mode ? (pivot_ptr ? (double)pivot_ptr[ch] : 0.0) : (n > 0 ? (double)ld_elem(x + ch) : 0.0);
}
// channels [fb * kFoldCh, +kFoldCh): fold, finish, save the statistics, update the running statistics
template <typename T, bool COH>
__device__ inline void fold_fwd_body(const float *scratch, const T *x, int fb, int nblocks, int c, int64_t n, float eps, float momentum,
                                     float *running_mean, float *running_var, float *stats, int pivot_mode, const float *pivot_ptr) {
  __shared__ double red[kFoldSl][2][kFoldCh];
  const int ch = fb * kFoldCh + (threadIdx.x % kFoldCh), part = threadIdx.x / kFoldCh;
  double s, ss;
  fold_sums<COH>(scratch, nblocks, c, ch, part, s, ss, red);
  if (part != 0 || ch >= c) return;
  const BnMoments m = bn_finish(s, ss, n, fold_pivot(x, n, ch, pivot_mode, pivot_ptr), eps);
  Mem<COH>::st(stats + ch, (float)m.mean);
  Mem<COH>::st(stats + c + ch, m.istd);
  if (running_mean) bn_update_running(running_mean[ch], running_var[ch], momentum, m, n);
}
__device__ inline void count_batch(long long *nbt) {          // nn.BatchNorm1d.num_batches_tracked
  if (nbt && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
}
template <typename T>
__global__ __launch_bounds__(256) void k_fold_fwd(const float *__restrict__ scratch, const T *__restrict__ x, int nblocks, int c,
                                                  int64_t n, float eps, float momentum, float *__restrict__ running_mean,
                                                  float *__restrict__ running_var, long long *__restrict__ nbt,
                                                  float *__restrict__ stats, int pivot_mode, const float *__restrict__ pivot_ptr) {
  count_batch(nbt);
  fold_fwd_body<T, false>(scratch, x, blockIdx.x, nblocks, c, n, eps, momentum, running_mean, running_var, stats, pivot_mode, pivot_ptr);
}
// one norm of a forward pair as the kernels see it: input, parameters, buffers, and where its partial rows / statistics lie
template <typename T> struct PairFwdNorm {
  const T *x;
  const float *gamma, *beta;
  float *running_mean, *running_var;
  long long *nbt;
  float *stats;
  const float *scratch;
  float eps, momentum;
};
// k_fold_fwd for the two norms of a pair: blockIdx.y picks the norm
template <typename T>
__global__ __launch_bounds__(256) void k_fold_fwd_pair(PairFwdNorm<T> a, PairFwdNorm<T> b, int nblocks, int c, int64_t n) {
  const PairFwdNorm<T> &p = blockIdx.y ? b : a;
  count_batch(p.nbt);
  fold_fwd_body<T, false>(p.scratch, p.x, blockIdx.x, nblocks, c, n, p.eps, p.momentum, p.running_mean, p.running_var, p.stats, 0, nullptr);
}
// split API (SyncBN): local mean and M2 = sum (x - mean)^2, to be combined across ranks with Chan's formula
template <typename T>
__global__ __launch_bounds__(256) void k_fold_stats(const float *__restrict__ scratch, const T *__restrict__ x, int nblocks, int c,
                                                    int64_t n, float *__restrict__ mean_m2, int pivot_mode,
                                                    const float *__restrict__ pivot_ptr) {
  __shared__ double red[kFoldSl][2][kFoldCh];
  const int ch = blockIdx.x * kFoldCh + (threadIdx.x % kFoldCh), part = threadIdx.x / kFoldCh;
  double s, ss;
  fold_sums<false>(scratch, nblocks, c, ch, part, s, ss, red);
  if (part != 0 || ch >= c) return;
  const double dm = bn_shift(s, n);
  double m2 = __builtin_fma(-dm, (double)n * dm, ss);
  if (m2 < 0.0) m2 = 0.0;
  mean_m2[ch] = (float)(fold_pivot(x, n, ch, pivot_mode, pivot_ptr) + dm);
  mean_m2[c + ch] = (float)m2;
  if (ch == 0) mean_m2[2 * c] = (float)n;   // [mean | M2 | count]: one packed all-gather per layer
}

// channels [fb * kFoldCh, +kFoldCh): dbeta = sum dy', dgamma = sum dy' xhat, and both again as the `sums` row of the apply
template <bool COH>
__device__ inline void fold_bwd_body(const float *scratch, int fb, int nblocks, int c, float *dgamma, float *dbeta, float *sums) {
  __shared__ double red[kFoldSl][2][kFoldCh];
  const int ch = fb * kFoldCh + (threadIdx.x % kFoldCh), part = threadIdx.x / kFoldCh;
  double s, ss;
  fold_sums<COH>(scratch, nblocks, c, ch, part, s, ss, red);
  if (part != 0 || ch >= c) return;
  dbeta[ch] = (float)s;
  dgamma[ch] = (float)ss;
  Mem<COH>::st(sums + ch, (float)s);
  Mem<COH>::st(sums + c + ch, (float)ss);
}
__global__ __launch_bounds__(256) void k_fold_bwd(const float *__restrict__ scratch, int nblocks, int c, float *__restrict__ dgamma,
                                                  float *__restrict__ dbeta, float *__restrict__ sums) {
  fold_bwd_body<false>(scratch, blockIdx.x, nblocks, c, dgamma, dbeta, sums);
}
// k_fold_bwd for the two norms of a pair: blockIdx.y picks the norm
__global__ __launch_bounds__(256) void k_fold_bwd_pair(const float *__restrict__ scratch_a, const float *__restrict__ scratch_b, int nblocks,
                                                       int c, float *__restrict__ dgamma_a, float *__restrict__ dbeta_a,
                                                       float *__restrict__ sums_a, float *__restrict__ dgamma_b,
                                                       float *__restrict__ dbeta_b, float *__restrict__ sums_b) {
  if (blockIdx.y) fold_bwd_body<false>(scratch_b, blockIdx.x, nblocks, c, dgamma_b, dbeta_b, sums_b);
  else fold_bwd_body<false>(scratch_a, blockIdx.x, nblocks, c, dgamma_a, dbeta_a, sums_a);
}

// SyncBN: combine the per-rank [mean | M2 | count] records (Chan's parallel formula, double) into the global
// mean / invstd, update the running statistics and num_batches_tracked, and leave 1/N for the backward pass
__global__ void k_sync_combine(const float *__restrict__ all_stats, int world, int c, float eps, float momentum,
                               float *__restrict__ running_mean, float *__restrict__ running_var, long long *__restrict__ nbt,
                               float *__restrict__ stats, float *__restrict__ inv_n_out) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  const int rec = 2 * c + 1;
  double n = 0.0;
  for (int r = 0; r < world; ++r) n += (double)all_stats[(int64_t)r * rec + 2 * c];
  if (ch == 0) {
    if (inv_n_out) *inv_n_out = n > 0.0 ? (float)(1.0 / n) : 0.f;
    if (nbt) *nbt += 1;
  }
  if (ch >= c) return;
  double mean = 0.0;
  for (int r = 0; r < world; ++r) mean = __builtin_fma((double)all_stats[(int64_t)r * rec + 2 * c], (double)all_stats[(int64_t)r * rec + ch], mean);
  mean = n > 0.0 ? mean / n : 0.0;
  double m2 = 0.0;
  for (int r = 0; r < world; ++r) {
    const double d = (double)all_stats[(int64_t)r * rec + ch] - mean;
    m2 += __builtin_fma(d, (double)all_stats[(int64_t)r * rec + 2 * c] * d, (double)all_stats[(int64_t)r * rec + c + ch]);
  }
  const double var = n > 0.0 ? m2 / n : 0.0;
  stats[ch] = (float)mean;
  stats[c + ch] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) bn_update_running(running_mean[ch], running_var[ch], momentum, mean, n > 1.0 ? m2 / (n - 1.0) : var);
}

// y = relu?( (x - mean) * invstd * gamma + beta (+ residual) )
// A thread owns ONE channel group (its per-channel constants live in registers) and walks rows: with
// G = C / W groups, thread t handles group t % G of rows t / G, t / G + R, ...  (R = rows per sweep of the grid).
// Two independent 16-byte loads are in flight per operand per thread.  NT: the output is not read again soon.
// y_ld = row stride of the output (elements): > c when y is a column slice of a wider buffer (zero-copy ME.cat)
// (this loop, bwd_apply_rows and the two constant loaders below are __forceinline__: inlined by the ordinary inliner the bf16
// kernels took up to 24 VGPRs more and lost a wave or two per SIMD -- profiles/norm_arith.txt, section 3)
template <typename T, bool NT>
__device__ __forceinline__ void apply_rows(const T *__restrict__ x, const T *__restrict__ res, int64_t n, int c, const BnFwdConsts<Width<T>::V> &k,
                                  int relu, T *__restrict__ y, int64_t y_ld, int cg, int rl, int RL) {
  constexpr int W = Width<T>::V;
  auto finish = [&](float (&xv)[W], const float (&rv)[W]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
      float o = k.out(i, xv[i]);
      if (res) o += rv[i];
      xv[i] = (relu && o < 0.f) ? 0.f : o;
    }
  };
  const int64_t stride = (int64_t)gridDim.x * RL;
  for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < n; r += 2 * stride) {
    const int64_t r2 = r + stride;
    const bool two = r2 < n;
    float xa[W], xb[W], ra[W], rb[W];
    ldv<W>(x + r * c + cg * W, xa);
    if (two) ldv<W>(x + r2 * c + cg * W, xb);
    if (res) { ldv<W>(res + r * c + cg * W, ra); if (two) ldv<W>(res + r2 * c + cg * W, rb); }
    finish(xa, ra);
    store_row<NT, W>(y + r * y_ld + cg * W, xa);
    if (two) {
      finish(xb, rb);
      store_row<NT, W>(y + r2 * y_ld + cg * W, xb);
    }
  }
}
template <typename T>
__global__ __launch_bounds__(kNT) void k_bn_apply(const T *__restrict__ x, const T *__restrict__ res, int64_t n, int c,
                                                  const float *__restrict__ gamma, const float *__restrict__ beta,
                                                  const float *__restrict__ stats, int relu, T *__restrict__ y, int64_t y_ld) {
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  if (rl >= RL) return;
  BnFwdConsts<W> k;
  k.template load<Mem<false>>(stats, gamma, beta, c, cg * W);
  apply_rows<T, true>(x, res, n, c, k, relu, y, y_ld, cg, rl, RL);
}

// dx = gamma*invstd * (dy' - mean(dy') - xhat * mean(dy' xhat));  dres = dy'
template <typename T, bool NT, bool FMA>
__device__ __forceinline__ void bwd_apply_rows(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ dy, int64_t n, int c,
                                      const BnBwdConsts<Width<T>::V> &k, int relu, T *__restrict__ dx, T *__restrict__ dres,
                                      int64_t dy_ld, int64_t y_ld, int cg, int rl, int RL) {
  constexpr int W = Width<T>::V;
  const int64_t stride = (int64_t)gridDim.x * RL;
  for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < n; r += stride) {
    const int64_t o = r * c + cg * W;
    float xv[W], gv[W];
    ldv<W>(x + o, xv);
    ldv<W>(dy + r * dy_ld + cg * W, gv);
    if (relu == 1) {
      float yv[W];
      ldv<W>(y + r * y_ld + cg * W, yv);
#pragma unroll
      for (int i = 0; i < W; ++i) gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
    } else if (relu == 2) {
#pragma unroll
      for (int i = 0; i < W; ++i) gv[i] = k.out(i, xv[i]) > 0.f ? gv[i] : 0.f;
    }
    if (dres) store_row<NT, W>(dres + o, gv);
#pragma unroll
    for (int i = 0; i < W; ++i) xv[i] = k.template dx<FMA>(i, xv[i], gv[i]);
    store_row<NT, W>(dx + o, xv);
  }
}
template <typename T>
__global__ __launch_bounds__(kNT) void k_bn_bwd_apply(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ dy,
                                                      int64_t n, int c, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta,
                                                      const float *__restrict__ stats, const float *__restrict__ sums,
                                                      float inv_n, int relu, T *__restrict__ dx, T *__restrict__ dres,
                                                      int64_t dy_ld, const float *__restrict__ inv_n_dev, int64_t y_ld) {
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  if (rl >= RL) return;
  if (inv_n_dev) inv_n = *inv_n_dev;   // SyncBN: 1 / global row count lives on the device (no host sync)
  BnBwdConsts<W> k;
  float s[W], ss[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { s[i] = sums[cg * W + i]; ss[i] = sums[c + cg * W + i]; }
  k.load(stats, gamma, beta, c, cg * W, relu, inv_n, s, ss);
  bwd_apply_rows<T, true, kDxFma<T, kBwdThree>>(x, y, dy, n, c, k, relu, dx, dres, dy_ld, y_ld, cg, rl, RL);
}

// k_colreduce as the first of three launches: >= 128 rows per block, <= 512 blocks: coarse levels (a few thousand rows) still get
// tens of blocks -- with 1024 rows per block their reductions were 5-block, 13 us latency chains
constexpr int kReduceMaxBlocks = 512;

// ------------------------------------------------------------------------------------------------ one launch per direction
// A BatchNorm direction is three dependent steps (column sums over all rows -> fold + finish the statistics -> elementwise
// apply): three launches per direction made 372 of the compute stream's 596 launches per training step, most of them on
// coarse levels where a launch is a few microseconds of work.  The fused kernels run the three steps in ONE launch of <= 256
// co-resident workgroups separated by two grid-wide barriers (arrive = agent-scope add on a counter, wait = spin on
// it); a workgroup applies to the SAME slab of rows it reduced, walking it backwards, so the rows it read last in step 1 are
// the first it needs in step 3 (L2 / Infinity Cache hits instead of a second HBM pass on the large levels).
// Co-residency: 256 workgroups x 256 threads at <= 128 VGPRs is a quarter of what the chip holds (256 CUs x 4), so such kernels
// from different streams / processes can spin at the same time without starving each other's unscheduled workgroups.  The cap
// is 256 and not 512 because the weight-gradient kernel on the side stream owns whole CUs (all registers, all LDS) for up to a
// millisecond: every workgroup of a barrier kernel has to find a free CU before ANY of them gets past the first barrier
// (measured in the 8-scene step, layers <= 24 MB fused: 30.9 ms with 512 workgroups, 29.8 ms with 256, 30.0 ms unfused).
constexpr int kFusedMaxBlocks = 256;

__device__ inline void grid_arrive_wait(unsigned *ctr, unsigned target) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's coherent stores are acknowledged
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) __builtin_amdgcn_s_sleep(1);
  }
  __syncthreads();
}
// the last workgroup to leave puts the counter back to zero for the slot's next user
__device__ inline void grid_leave(unsigned *ctr, unsigned total) {
  if (threadIdx.x == 0) {
    const unsigned old = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == total - 1) __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// column sums of one slab of rows [r0, r1) -> dst[2][C]; the body of k_colreduce (same summation order)
template <typename T, int MODE>
__device__ inline void colreduce_slab(const T *x, const T *y, const T *dy, const float *stats, const float *gamma, const float *beta,
                                      int64_t n, int c, int relu, int64_t r0, int64_t r1, float *dst, int64_t dy_ld, int64_t y_ld) {
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  const bool active = rl < RL;
  float s0[W], s1[W];
#pragma unroll
  for (int i = 0; i < W; ++i) s0[i] = s1[i] = 0.f;
  float pivot[W];
  BnBwdConsts<W> k;
  if (MODE == 1) k.load_norm(stats, gamma, beta, c, cg * W, relu);
  else if (n > 0) ldv<W>(x + cg * W, pivot);   // row 0, as in k_colreduce<T, 0>
  if (active) {
    int64_t r = r0 + rl;
    constexpr int U = MODE == 0 ? 4 : 2;
    auto accumulate = [&](const float (&xv)[W], float (&gv)[W], const float (&yv)[W]) __attribute__((always_inline)) {
      if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < W; ++i) bn_acc_fwd(xv[i], pivot[i], s0[i], s1[i]);
      } else {
        if (relu == 1) {
#pragma unroll
          for (int i = 0; i < W; ++i) gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
        } else if (relu == 2) {
#pragma unroll
          for (int i = 0; i < W; ++i) gv[i] = k.out(i, xv[i]) > 0.f ? gv[i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < W; ++i) bn_acc_bwd(gv[i], xv[i], k.mean[i], k.istd[i], s0[i], s1[i]);
      }
    };
    for (; r + (U - 1) * RL < r1; r += U * RL) {
      float xv[U][W], gv[U][W], yv[U][W];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ldv<W>(x + (r + u * RL) * c + cg * W, xv[u]);
        if (MODE == 1) {
          ldv<W>(dy + (r + u * RL) * dy_ld + cg * W, gv[u]);
          if (relu == 1) ldv<W>(y + (r + u * RL) * y_ld + cg * W, yv[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) accumulate(xv[u], gv[u], yv[u]);
    }
    for (; r < r1; r += RL) {
      float xv[W], gv[W], yv[W];
      ldv<W>(x + r * c + cg * W, xv);
      if (MODE == 1) {
        ldv<W>(dy + r * dy_ld + cg * W, gv);
        if (relu == 1) ldv<W>(y + r * y_ld + cg * W, yv);
      }
      accumulate(xv, gv, yv);
    }
  }
  __shared__ float red[2][kNT][8];
#pragma unroll
  for (int i = 0; i < W; ++i) { red[0][threadIdx.x][i] = s0[i]; red[1][threadIdx.x][i] = s1[i]; }
  __syncthreads();
  if (rl == 0) {
    for (int j = 1; j < RL; ++j) {
#pragma unroll
      for (int i = 0; i < W; ++i) { s0[i] += red[0][j * G + cg][i]; s1[i] += red[1][j * G + cg][i]; }
    }
#pragma unroll
    for (int i = 0; i < W; ++i) { st_coh(dst + cg * W + i, s0[i]); st_coh(dst + c + cg * W + i, s1[i]); }
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(4))) void k_bn_fwd_fused(const T *x, const T *res, int64_t n, int c, const float *gamma, const float *beta,
                                                      float eps, float momentum, float *running_mean, float *running_var,
                                                      long long *nbt, float *stats, int relu, T *y, int64_t y_ld, float *scratch,
                                                      const float *partials, int partial_rows, int partial_rpb, int nfoldrows,
                                                      const float *pivot_ptr, int64_t rows_per_block, unsigned *ctr) {
  constexpr int W = Width<T>::V;
  const unsigned nwg = gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(r0 + rows_per_block, n);
  // ---- step 1: per-workgroup column sums (or: fold the conv epilogue's partial rows into <= 128 rows)
  if (partials) {
    for (int pb = blockIdx.x; pb < nfoldrows; pb += nwg)
      partial_reduce_rows<true>(partials, pb * partial_rpb, min(pb * partial_rpb + partial_rpb, partial_rows), 2 * c, scratch + (int64_t)pb * 2 * c);
  } else {
    colreduce_slab<T, 0>(x, nullptr, nullptr, nullptr, nullptr, nullptr, n, c, 0, r0, r1, scratch + (int64_t)blockIdx.x * 2 * c, c, c);
  }
  grid_arrive_wait(ctr, nwg);
  // ---- step 2: fold + finish the statistics, 16 channels per workgroup
  for (int fb = blockIdx.x; fb < (c + kFoldCh - 1) / kFoldCh; fb += nwg) {
    fold_fwd_body<T, true>(scratch, x, fb, nfoldrows, c, n, eps, momentum, running_mean, running_var, stats, partials != nullptr, pivot_ptr);
    __syncthreads();
  }
  count_batch(nbt);
  grid_arrive_wait(ctr, 2 * nwg);
  grid_leave(ctr, 3 * nwg);
  // ---- step 3: y = relu?((x - mean) * invstd * gamma + beta (+ residual)) over this workgroup's slab, last rows first
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  if (rl >= RL) return;
  BnFwdConsts<W> k;
  k.template load<Mem<true>>(stats, gamma, beta, c, cg * W);
  constexpr int U = W == 8 ? 2 : 4;   // rows in flight per thread (registers: <= 128 VGPRs, see above)
  for (int64_t r = r1 - 1 - rl; r >= r0; r -= (int64_t)U * RL) {
    float xv[U][W], rv[U][W];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ru = r - (int64_t)u * RL;
      if (ru >= r0) {
        ldv<W>(x + ru * c + cg * W, xv[u]);
        if (res) ldv<W>(res + ru * c + cg * W, rv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ru = r - (int64_t)u * RL;
      if (ru >= r0) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
          float o = k.out(i, xv[u][i]);
          if (res) o += rv[u][i];
          xv[u][i] = (relu && o < 0.f) ? 0.f : o;
        }
        stv<W>(y + ru * y_ld + cg * W, xv[u]);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) __attribute__((amdgpu_waves_per_eu(4))) void k_bn_bwd_fused(const T *x, const T *y, const T *dy, int64_t n, int c, const float *gamma,
                                                      const float *beta, const float *stats, int relu, T *dx, T *dres, float *dgamma,
                                                      float *dbeta, float *scratch, float *sums, int64_t dy_ld, int64_t y_ld,
                                                      int64_t rows_per_block, float inv_n, unsigned *ctr) {
  constexpr int W = Width<T>::V;
  const unsigned nwg = gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = min(r0 + rows_per_block, n);
  colreduce_slab<T, 1>(x, y, dy, stats, gamma, beta, n, c, relu, r0, r1, scratch + (int64_t)blockIdx.x * 2 * c, dy_ld, y_ld);
  grid_arrive_wait(ctr, nwg);
  for (int fb = blockIdx.x; fb < (c + kFoldCh - 1) / kFoldCh; fb += nwg) {
    fold_bwd_body<true>(scratch, fb, (int)nwg, c, dgamma, dbeta, sums);
    __syncthreads();
  }
  grid_arrive_wait(ctr, 2 * nwg);
  grid_leave(ctr, 3 * nwg);
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  if (rl >= RL) return;
  BnBwdConsts<W> k;
  float s[W], ss[W];
#pragma unroll
  for (int i = 0; i < W; ++i) { s[i] = ld_coh(sums + cg * W + i); ss[i] = ld_coh(sums + c + cg * W + i); }
  k.load(stats, gamma, beta, c, cg * W, relu, inv_n, s, ss);
  constexpr int U = W == 8 ? 1 : 2;
  for (int64_t r = r1 - 1 - rl; r >= r0; r -= (int64_t)U * RL) {
    float xv[U][W], gv[U][W], yv[U][W];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ru = r - (int64_t)u * RL;
      if (ru >= r0) {
        ldv<W>(x + ru * c + cg * W, xv[u]);
        ldv<W>(dy + ru * dy_ld + cg * W, gv[u]);
        if (relu == 1) ldv<W>(y + ru * y_ld + cg * W, yv[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ru = r - (int64_t)u * RL;
      if (ru >= r0) {
        if (relu == 1) {
#pragma unroll
          for (int i = 0; i < W; ++i) gv[u][i] = yv[u][i] > 0.f ? gv[u][i] : 0.f;
        } else if (relu == 2) {
#pragma unroll
          for (int i = 0; i < W; ++i) gv[u][i] = k.out(i, xv[u][i]) > 0.f ? gv[u][i] : 0.f;
        }
        if (dres) stv<W>(dres + ru * c + cg * W, gv[u]);
#pragma unroll
        for (int i = 0; i < W; ++i) xv[u][i] = k.template dx<kDxFma<T, kBwdFused>>(i, xv[u][i], gv[u][i]);
        stv<W>(dx + ru * c + cg * W, xv[u]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ two launches, no barrier
// Small layers (the coarse levels: a few thousand to ~100 k rows) are latency chains, not bandwidth: three dependent launches
// per direction, or ONE launch with two hand-rolled grid barriers whose workgroups must all be resident before the first may
// pass (round 4: 53 us per backward launch in the step, 8 % of the HBM peak; the weight-gradient kernel on the side stream owns
// CUs for a millisecond at a time).  Here a direction is TWO ordinary launches: the column reduction into <= kFoldParts partial
// rows, and an apply kernel whose every workgroup first folds those partial rows itself -- the threads of a workgroup that share
// a channel group split the rows between them (fixed assignment, double accumulation, combined through LDS in lane order: every
// workgroup computes bit-identical statistics) -- and then streams its rows.  No inter-workgroup synchronisation, no fold
// launch; the redundant fold reads (workgroups x parts x 2C floats) stay in L2.  Workgroup 0 also writes what the fold kernels
// write: saved statistics, running statistics, num_batches_tracked / d gamma, d beta.
constexpr int kFoldParts = 64;      // partial rows (upper bound; knob BN_FOLD_PARTS)

// -> this thread's channel-group totals of the two column sums, as doubles
template <int W>
__device__ inline void fold_in_block(const float *__restrict__ scratch, int nparts, int c, int G, int RL, int cg, int rl,
                                     double (&t0)[W], double (&t1)[W]) {
  __shared__ double fred[2][kNT][W];
  double a0[W], a1[W];
#pragma unroll
  for (int i = 0; i < W; ++i) a0[i] = a1[i] = 0.0;
  if (rl < RL) {
    for (int b = rl; b < nparts; b += RL) {
      const float *row = scratch + (int64_t)b * 2 * c + cg * W;
#pragma unroll
      for (int i = 0; i < W; ++i) { a0[i] += (double)row[i]; a1[i] += (double)row[c + i]; }
    }
  }
#pragma unroll
  for (int i = 0; i < W; ++i) { fred[0][threadIdx.x][i] = a0[i]; fred[1][threadIdx.x][i] = a1[i]; }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < W; ++i) { t0[i] = 0.0; t1[i] = 0.0; }
  if (rl < RL) {
    const int lim = RL < nparts ? RL : nparts;
    for (int j = 0; j < lim; ++j) {
#pragma unroll
      for (int i = 0; i < W; ++i) { t0[i] += fred[0][j * G + cg][i]; t1[i] += fred[1][j * G + cg][i]; }
    }
  }
}

// One norm's forward constants for this thread.  FOLD: from the workgroup's own fold of p.scratch (workgroup 0 also writes what
// k_fold_fwd writes); otherwise from the saved statistics.  Every thread of the workgroup calls it (fold_in_block synchronises).
template <typename T, bool FOLD>
__device__ __forceinline__ void fwd_consts(const PairFwdNorm<T> &p, int64_t n, int c, int nparts, int G, int RL, int cg, int rl, BnFwdConsts<Width<T>::V> &k) {
  constexpr int W = Width<T>::V;
  if constexpr (FOLD) {
    double t0[W], t1[W];
    fold_in_block<W>(p.scratch, nparts, c, G, RL, cg, rl, t0, t1);
    if (rl < RL) {
      float piv[W];
      if (n > 0) ldv<W>(p.x + cg * W, piv);          // the pivot of k_colreduce<T, 0>: row 0
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const int ch = cg * W + i;
        const BnMoments m = bn_finish(t0[i], t1[i], n, n > 0 ? (double)piv[i] : 0.0, p.eps);
        k.set(i, (float)m.mean, m.istd, p.gamma[ch], p.beta[ch]);
        if (blockIdx.x == 0 && rl == 0) {
          p.stats[ch] = (float)m.mean; p.stats[c + ch] = m.istd;
          if (p.running_mean) bn_update_running(p.running_mean[ch], p.running_var[ch], p.momentum, m, n);
        }
      }
    }
    count_batch(p.nbt);
  } else {
    if (rl < RL) k.template load<Mem<false>>(p.stats, p.gamma, p.beta, c, cg * W);
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) void k_bn_apply_fold(const T *__restrict__ x, const T *__restrict__ res, int64_t n, int c,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                       float momentum, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                       long long *__restrict__ nbt, float *__restrict__ stats,
                                                       const float *__restrict__ scratch, int nparts, int relu, T *__restrict__ y,
                                                       int64_t y_ld) {
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  BnFwdConsts<W> k;
  fwd_consts<T, true>({x, gamma, beta, running_mean, running_var, nbt, stats, scratch, eps, momentum}, n, c, nparts, G, RL, cg, rl, k);
  if (rl >= RL) return;
  apply_rows<T, false>(x, res, n, c, k, relu, y, y_ld, cg, rl, RL);
}

// one norm of a backward pair as the kernels see it
template <typename T> struct PairBwdNorm {
  const T *x;
  const float *gamma, *beta, *stats;
  const float *scratch;     // partial rows (FOLD)
  const float *sums;        // folded sums (three launches)
  float *dgamma, *dbeta;    // FOLD: workgroup 0 writes them
  T *dx;
};
// One norm's backward constants for this thread.  FOLD: the sums from the workgroup's own fold of p.scratch, rounded as k_fold_bwd
// stores them (workgroup 0 also writes dgamma / dbeta); otherwise from p.sums.  Every thread of the workgroup calls it.
template <typename T, bool FOLD>
__device__ __forceinline__ void bwd_consts(const PairBwdNorm<T> &p, int c, int nparts, float inv_n, int relu, int G, int RL, int cg, int rl,
                                  BnBwdConsts<Width<T>::V> &k) {
  constexpr int W = Width<T>::V;
  double t0[W], t1[W];
  if constexpr (FOLD) fold_in_block<W>(p.scratch, nparts, c, G, RL, cg, rl, t0, t1);
  if (rl >= RL) return;
  float s[W], ss[W];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const int ch = cg * W + i;
    if constexpr (FOLD) {
      s[i] = (float)t0[i]; ss[i] = (float)t1[i];
      if (blockIdx.x == 0 && rl == 0) { p.dbeta[ch] = s[i]; p.dgamma[ch] = ss[i]; }
    } else {
      s[i] = p.sums[ch]; ss[i] = p.sums[c + ch];
    }
  }
  k.load(p.stats, p.gamma, p.beta, c, cg * W, relu, inv_n, s, ss);
}

template <typename T>
__global__ __launch_bounds__(kNT) void k_bn_bwd_apply_fold(const T *__restrict__ x, const T *__restrict__ y, const T *__restrict__ dy,
                                                           int64_t n, int c, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ stats,
                                                           const float *__restrict__ scratch, int nparts, float inv_n, int relu,
                                                           T *__restrict__ dx, T *__restrict__ dres, float *__restrict__ dgamma,
                                                           float *__restrict__ dbeta, int64_t dy_ld, int64_t y_ld) {
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  BnBwdConsts<W> k;
  bwd_consts<T, true>({x, gamma, beta, stats, scratch, nullptr, dgamma, dbeta, dx}, c, nparts, inv_n, relu, G, RL, cg, rl, k);
  if (rl >= RL) return;
  bwd_apply_rows<T, false, kDxFma<T, kBwdFold>>(x, y, dy, n, c, k, relu, dx, dres, dy_ld, y_ld, cg, rl, RL);
}

// ------------------------------------------------------------------------------------------------ two norms, shared passes
// A residual block with a downsample branch runs two norms on the same rows: forward y = relu?(bn_a(xa) + bn_b(xb)), backward
// both receive the same masked gradient.  As single calls the branch output is written and read back only to be added (7 tensor
// passes forward), and the masked gradient is written and read back twice (13 backward).  The pair kernels read every operand
// once per step -- statistics of both norms in one launch, one fold launch (blockIdx.y = the norm), one apply -- 5 passes forward
// and 10 backward.  Every per-element expression and every summation order is the single kernels': results are bit-identical.
// FOLD: the `fold` path -- every workgroup folds both norms' partial rows itself, as k_bn_apply_fold / k_bn_bwd_apply_fold do.

// y = relu?(bn_a(xa) + stored(bn_b(xb))); res (may be NULL) = bn_b(xb), the branch output the single calls materialise
template <typename T, bool FOLD>
__global__ __launch_bounds__(kNT) void k_bn_apply_pair(PairFwdNorm<T> a, PairFwdNorm<T> b, int64_t n, int c, int nparts, int relu,
                                                       T *__restrict__ y, int64_t y_ld, T *__restrict__ res) {
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  BnFwdConsts<W> ka, kb;
  fwd_consts<T, FOLD>(a, n, c, nparts, G, RL, cg, rl, ka);
  if constexpr (FOLD) __syncthreads();             // fold_in_block's LDS is read by the first fold until here
  fwd_consts<T, FOLD>(b, n, c, nparts, G, RL, cg, rl, kb);
  if (rl >= RL) return;
  auto finish = [&](float (&xa)[W], float (&xb)[W]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
      xb[i] = kb.out(i, xb[i]);
      const float o = ka.out(i, xa[i]) + stored_value<T>(xb[i]);      // the branch rounded as its store would
      xa[i] = (relu && o < 0.f) ? 0.f : o;
    }
  };
  const int64_t stride = (int64_t)gridDim.x * RL;
  for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < n; r += 2 * stride) {
    const int64_t r2 = r + stride;
    const bool two = r2 < n;
    float xa[W], xa2[W], xb[W], xb2[W];
    ldv<W>(a.x + r * c + cg * W, xa);
    ldv<W>(b.x + r * c + cg * W, xb);
    if (two) { ldv<W>(a.x + r2 * c + cg * W, xa2); ldv<W>(b.x + r2 * c + cg * W, xb2); }
    finish(xa, xb);
    if (res) stv_nt<W>(res + r * c + cg * W, xb);
    stv_nt<W>(y + r * y_ld + cg * W, xa);
    if (two) {
      finish(xa2, xb2);
      if (res) stv_nt<W>(res + r2 * c + cg * W, xb2);
      stv_nt<W>(y + r2 * y_ld + cg * W, xa2);
    }
  }
}

// dxa, dxb from one read of xa, ya, dy, xb: both norms receive dy' = dy masked by norm a's ReLU (relu: 0 or 1 -- a mask recomputed
// from xa alone would ignore the branch that was added); dres (may be NULL) = dy'
template <typename T, bool FOLD>
__global__ __launch_bounds__(kNT) void k_bn_bwd_apply_pair(PairBwdNorm<T> a, PairBwdNorm<T> b, const T *__restrict__ y,
                                                           const T *__restrict__ dy, int64_t n, int c, int nparts, float inv_n, int relu,
                                                           T *__restrict__ dres, int64_t dy_ld, int64_t y_ld) {
  constexpr BwdKernel kAs = FOLD ? kBwdFold : kBwdThree;      // the single kernel this instance stands for
  constexpr int W = Width<T>::V;
  const int G = c / W, RL = kNT / G;
  const int cg = threadIdx.x % G, rl = threadIdx.x / G;
  BnBwdConsts<W> ka, kb;
  bwd_consts<T, FOLD>(a, c, nparts, inv_n, relu, G, RL, cg, rl, ka);
  if constexpr (FOLD) __syncthreads();             // fold_in_block's LDS is read by the first fold until here
  bwd_consts<T, FOLD>(b, c, nparts, inv_n, 0, G, RL, cg, rl, kb);
  if (rl >= RL) return;
  const int64_t stride = (int64_t)gridDim.x * RL;
  for (int64_t r = (int64_t)blockIdx.x * RL + rl; r < n; r += stride) {
    const int64_t o = r * c + cg * W;
    float xv[W], gv[W], xbv[W];
    ldv<W>(a.x + o, xv);
    ldv<W>(b.x + o, xbv);
    ldv<W>(dy + r * dy_ld + cg * W, gv);
    if (relu == 1) {
      float yv[W];
      ldv<W>(y + r * y_ld + cg * W, yv);
#pragma unroll
      for (int i = 0; i < W; ++i) gv[i] = yv[i] > 0.f ? gv[i] : 0.f;
    }
    if (dres) stv_nt<W>(dres + o, gv);
#pragma unroll
    for (int i = 0; i < W; ++i) {
      xv[i] = ka.template dx<kDxFma<T, kAs>>(i, xv[i], gv[i]);
      xbv[i] = kb.template dx<kDxFma<T, kAs>>(i, xbv[i], gv[i]);
    }
    stv_nt<W>(a.dx + o, xv);
    stv_nt<W>(b.dx + o, xbv);
  }
}

// ------------------------------------------------------------------------------------------------ host: one plan per call
// Everything a BatchNorm call decides on the host is computed ONCE by norm_plan() from (direction, n, c, element size, conv
// partial rows, resident-workgroup cap, tuning table): the path, every grid and rows-per-block, and where each workspace region
// lies.  The entry points are plan + one switch; lgs_bn_workspace_bytes is the bound over every plan.  Paths are tried in this
// order -- the order IS the policy:
//   fold  (directions that apply, statistics from x, n > 0, BN_FOLD != 0, tensor <= BN_FOLD_MAX_MB): k_colreduce into
//         <= min(BN_FOLD_PARTS, kFoldParts) partial rows, then k_bn_apply_fold / k_bn_bwd_apply_fold on <= BN_FOLD_GRID workgroups;
//   fused (directions that apply, BN_FUSED != 0, tensor <= BN_FUSED_MAX_MB -- forward: the smaller of it and BN_FUSED_FWD_MAX_MB --
//         and the device holds >= 16 workgroups of the kernel at once): ONE launch of <= min(cap, kFusedMaxBlocks, BN_FUSED_BLOCKS);
//   three: k_colreduce into <= kReduceMaxBlocks rows (or k_partial_reduce: the conv epilogue's rows into <= kPartialFoldRows),
//         k_fold_*, then the apply on <= kApplyMaxBlocks workgroups (skipped for an empty tensor).
// lgs_bn_stats and lgs_bn_backward_reduce are the first two launches of `three`.
using NormPlan = lgs_norm_plan_info;
enum NormDir { kNormFwd = 0, kNormBwd = 1, kNormStats = 2, kNormBwdReduce = 3 };
enum NormPath { kNormFold = 1, kNormFused = 2, kNormThree = 3 };
constexpr int kApplyMaxBlocks = 4096;   // k_bn_apply / k_bn_bwd_apply: grid-stride over the rows
constexpr int kCoopMinBlocks = 16;      // fewer co-resident workgroups than this: the grid-barrier kernels are not worth it

// n rows over at most `cap` workgroups of at least 128 rows each -> workgroups used (>= 1, also for n == 0)
inline int row_blocks(int64_t n, int64_t cap, int64_t *rows_per_block) {
  int64_t nb = (n + 127) / 128;
  if (nb > cap) nb = cap;
  if (nb < 1) nb = 1;
  int64_t rpb = (n + nb - 1) / nb;
  if (rpb < 1) rpb = 1;
  *rows_per_block = rpb;
  nb = (n + rpb - 1) / rpb;
  return (int)(nb > 0 ? nb : 1);
}
// workgroups of an elementwise launch that gives each thread `per_thread` vectors before it strides; 0 = nothing to launch
inline int apply_blocks(int64_t n, int c, int W, int per_thread, int64_t cap) {
  const int64_t total = n * (int64_t)(c / W), g = (total + per_thread * kNT - 1) / (per_thread * kNT);
  return (int)(g < cap ? g : cap);
}
// The scratch of a call is [partial rows][2c] floats, then ONE more row: `sums` (backward) or the dgamma / dbeta spill
// (lgs_bn_backward_reduce) -- never both in one call.  The size is the bound over every path and knob setting (callers cache it
// per (n, c) and change knobs afterwards), so it depends on neither: the most rows any splitter makes, that row, and what the
// size has always carried on top (a second row and 256 bytes) so that it does not move under its callers.
inline int64_t norm_workspace_bytes(int64_t n, int c) {
  int64_t rpb, rows = kPartialFoldRows;
  for (int cap : {kReduceMaxBlocks, kFusedMaxBlocks, kFoldParts}) rows = std::max<int64_t>(rows, row_blocks(n, cap, &rpb));
  return (int64_t)sizeof(float) * 2 * c * (rows + 2) + 256;
}

// resident_cap(): workgroups of the direction's grid-barrier kernel the device holds at once (fused_resident); asked only
// where the knobs and the size allow that path.  partial_rows: the conv epilogue's rows, 0 = statistics from x.  No HIP call.
template <typename Cap>
NormPlan norm_plan(int dir, int64_t n, int c, int dtype, int partial_rows, Cap &&resident_cap) {
  NormPlan p = {};
  const int W = epl(dtype);
  const int64_t tensor_bytes = n * (int64_t)c * (int64_t)esize(dtype);
  const bool applies = dir == kNormFwd || dir == kNormBwd;
  p.from_partials = (dir == kNormFwd || dir == kNormStats) && partial_rows > 0;
  if (p.from_partials) {     // wherever it happens (k_partial_reduce, step 1 of k_bn_fwd_fused): into <= kPartialFoldRows rows
    const int nb = partial_rows < kPartialFoldRows ? partial_rows : kPartialFoldRows;
    p.partial_rpb = (partial_rows + nb - 1) / nb;
    p.fold_rows = (partial_rows + p.partial_rpb - 1) / p.partial_rpb;
  }
  int64_t cap = 0;
  if (applies && !p.from_partials && n > 0 && tune(T_BN_FOLD) != 0 && tensor_bytes <= (tune(T_BN_FOLD_MAX_MB) << 20)) {
    p.path = kNormFold;
    cap = tune(T_BN_FOLD_PARTS);
    if (cap < 1 || cap > kFoldParts) cap = kFoldParts;
    const int64_t grid_cap = tune(T_BN_FOLD_GRID) < 1 ? 256 : tune(T_BN_FOLD_GRID);
    p.apply_grid = apply_blocks(n, c, W, 2, grid_cap);       // two rows per thread and sweep in the forward kernel
    if (p.apply_grid < 1) p.apply_grid = 1;
  } else {
    // above ~24 MB a direction is bandwidth-bound and the three-launch path's 4096-workgroup apply streams faster than 512
    // resident workgroups can (1.2 M rows x 96 ch bf16 forward: 0.135 ms vs 0.181 ms fused); below, launches dominate
    int64_t max_mb = tune(T_BN_FUSED_MAX_MB);
    if (dir == kNormFwd && tune(T_BN_FUSED_FWD_MAX_MB) < max_mb) max_mb = tune(T_BN_FUSED_FWD_MAX_MB);
    if (applies && tune(T_BN_FUSED) != 0 && tensor_bytes <= (max_mb << 20)) {
      cap = resident_cap();
      if (cap > kFusedMaxBlocks) cap = kFusedMaxBlocks;
      if (cap < kCoopMinBlocks) cap = 0;
      if (tune(T_BN_FUSED_BLOCKS) > 0 && tune(T_BN_FUSED_BLOCKS) < cap) cap = tune(T_BN_FUSED_BLOCKS);
    }
    if (cap > 0) {
      p.path = kNormFused;
    } else {
      p.path = kNormThree;
      cap = kReduceMaxBlocks;
      p.fold_grid = (c + kFoldCh - 1) / kFoldCh;
      if (applies) p.apply_grid = apply_blocks(n, c, W, 1, kApplyMaxBlocks);
    }
  }
  if (!(p.path == kNormThree && p.from_partials)) p.reduce_grid = row_blocks(n, cap, &p.rows_per_block);
  if (!p.from_partials) p.fold_rows = p.reduce_grid;
  const int64_t row_bytes = (int64_t)sizeof(float) * 2 * c;
  p.partials = {0, row_bytes * p.fold_rows};
  if (dir == kNormBwd && p.path != kNormFold) p.sums = {p.partials.bytes, row_bytes};
  if (dir == kNormBwdReduce) p.spill = {p.partials.bytes, row_bytes};
  p.bytes_total = p.partials.bytes + p.sums.bytes + p.spill.bytes;
  p.workspace_bytes = norm_workspace_bytes(n, c);
  return p;
}
inline float *region(void *workspace, const lgs_conv_plan_region &r) { return reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + r.offset); }

// barrier counters of the fused kernels: a ring of slots per device, zeroed once; a kernel leaves its slot at zero
constexpr int kCtrSlots = 256;
// `s`: the stream of the launch that asks.  The ring is zeroed ONCE, asynchronously on the first asker's stream; until that memset
// is known to have completed every asker's stream is ordered behind it through an event -- no host synchronisation anywhere
// (round 4 blocked the host in hipDeviceSynchronize at the first BatchNorm of a process).
inline unsigned *fused_counter(hipStream_t s) {
  static unsigned *ring[64] = {nullptr};
  static hipEvent_t zeroed[64] = {nullptr};
  static std::atomic<bool> settled[64];
  static std::atomic<unsigned> next[64];
  static std::mutex mu;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!settled[dev].load(std::memory_order_acquire)) {
    std::lock_guard<std::mutex> lock(mu);
    if (!ring[dev]) {
      unsigned *p = nullptr;
      if (hipMalloc(&p, kCtrSlots * sizeof(unsigned)) != hipSuccess) return nullptr;
      if (hipEventCreateWithFlags(&zeroed[dev], hipEventDisableTiming) != hipSuccess ||
          hipMemsetAsync(p, 0, kCtrSlots * sizeof(unsigned), s) != hipSuccess || hipEventRecord(zeroed[dev], s) != hipSuccess)
        return nullptr;
      ring[dev] = p;
    } else if (hipEventQuery(zeroed[dev]) == hipSuccess) {
      settled[dev].store(true, std::memory_order_release);
    } else {
      (void)hipGetLastError();                                   // hipErrorNotReady is not an error
      if (hipStreamWaitEvent(s, zeroed[dev], 0) != hipSuccess) return nullptr;
    }
  }
  return ring[dev] + (next[dev].fetch_add(1) % kCtrSlots);
}
// Workgroups a grid-barrier kernel may be launched with: every one of them must be RESIDENT at the same time, or the resident
// ones spin on the barrier for workgroups the dispatcher can never place (a hard GPU hang).  The bound is the kernel's own
// occupancy on THIS device x its CU count (a CPX partition of the chip has 32-38 CUs, not 256), halved for headroom against
// another stream's kernels holding CUs, cached per (device, kernel); norm_plan caps it at kFusedMaxBlocks and takes the
// three-launch path below kCoopMinBlocks.  What this cannot see: HSA_CU_MASK-style external masks and other PROCESSES on the
// same GPU -- those setups must run with the tuning knob BN_FUSED=0 (bench.py --same-device does).
inline int fused_resident(const void *kernel) {
  static std::mutex mu;
  static std::vector<std::pair<std::pair<int, const void *>, int>> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::lock_guard<std::mutex> lock(mu);
  for (auto &e : cache)
    if (e.first.first == dev && e.first.second == kernel) return e.second;
  int per_cu = 0, cus = 0, cap = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kNT, 0) == hipSuccess &&
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
    cap = per_cu * cus / 2;
  else
    (void)hipGetLastError();
  cache.push_back({{dev, kernel}, cap});
  return cap;
}

template <typename T> constexpr int dtype_of() { return sizeof(T) == 2 ? LGS_BF16 : LGS_F32; }
// dtype -> f(RowType<T, true>()): the family takes 16-byte accesses only, so its channel-count check sits on the shared lift
template <typename F>
int with_elem(int dtype, int c, const char *who, F &&f) {
  return with_row_type(dtype, true, who, [&](auto e) {
    LGS_REQUIRE(c % epl(dtype) == 0 && c / epl(dtype) <= kNT && c <= 2048, std::string(who) + ": channel count unsupported");
    return f(e);
  });
}
// row stride of a [n, c] operand that may be a column slice of a wider row-major buffer: 0 = c; rows must start 16-byte aligned
#define LGS_BN_STRIDE(who, p, row_stride, ld)                \
  const int64_t ld = (row_stride) > 0 ? (row_stride) : c;    \
  LGS_REQUIRE(!(p) || stride_ok(p, ld, c, dtype), who ": " #p " rows must start 16-byte aligned (row stride a multiple of 16 bytes)")

// the partial rows of a three-launch statistics pass: the column reduction over x, or the conv epilogue's rows folded
template <typename T>
void stats_rows(const NormPlan &p, const T *x, int64_t n, int c, const float *partials, int partial_rows, float *rows, hipStream_t s) {
  const T *no = nullptr;
  const float *nof = nullptr;
  if (p.from_partials) LGS_KLAUNCH(k_partial_reduce, p.fold_rows, 256, 0, s, partials, partial_rows, 2 * c, p.partial_rpb, rows);
  else LGS_KLAUNCH((k_colreduce<T, 0>), p.reduce_grid, kNT, 0, s, x, no, no, nof, nof, nof, n, c, 0, p.rows_per_block, rows, (int64_t)c, (int64_t)c, (T *)nullptr);
}

template <typename T>
int bn_forward_t(const T *x, int64_t n, int c, const float *gamma, const float *beta, float eps, float momentum, float *rm, float *rv,
                 long long *nbt, const T *res, int relu, T *y, float *stats, void *workspace, hipStream_t s, const float *partials,
                 int partial_rows, const float *pivot, int64_t y_ld) {
  if (!partials) partial_rows = 0;
  const NormPlan p = norm_plan(kNormFwd, n, c, dtype_of<T>(), partial_rows, [] { return fused_resident(reinterpret_cast<const void *>(&k_bn_fwd_fused<T>)); });
  float *rows = region(workspace, p.partials);  // caller-owned: no allocator call (and no implicit sync) here
  const T *no = nullptr;
  const float *nof = nullptr;
  switch (p.path) {
    case kNormFold:
      LGS_KLAUNCH((k_colreduce<T, 0>), p.reduce_grid, kNT, 0, s, x, no, no, nof, nof, nof, n, c, 0, p.rows_per_block, rows, (int64_t)c, (int64_t)c, (T *)nullptr);
      LGS_KLAUNCH((k_bn_apply_fold<T>), p.apply_grid, kNT, 0, s, x, res, n, c, gamma, beta, eps, momentum, rm, rv, nbt, stats, rows, p.fold_rows, relu, y, y_ld);
      break;
    case kNormFused: {
      unsigned *ctr = fused_counter(s);
      LGS_REQUIRE(ctr != nullptr, "lgs_bn_forward: could not allocate the grid-barrier counters");
      LGS_KLAUNCH((k_bn_fwd_fused<T>), p.reduce_grid, kNT, 0, s, x, res, n, c, gamma, beta, eps, momentum, rm, rv, nbt, stats, relu, y, y_ld, rows,
                  p.from_partials ? partials : nof, partial_rows, p.partial_rpb, p.fold_rows, pivot, p.rows_per_block, ctr);
      break;
    }
    default:
      stats_rows<T>(p, x, n, c, partials, partial_rows, rows, s);
      LGS_KLAUNCH((k_fold_fwd<T>), p.fold_grid, 256, 0, s, rows, x, p.fold_rows, c, n, eps, momentum, rm, rv, nbt, stats, p.from_partials, pivot);
      if (p.apply_grid) LGS_KLAUNCH((k_bn_apply<T>), p.apply_grid, kNT, 0, s, x, res, n, c, gamma, beta, stats, relu, y, y_ld);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

// relu mode 1 with a dresidual output, paths `three` and `fold`: the reduce launch writes the masked gradient to dres while it sums,
// and the apply launch reads it back as an unmasked dy -- y is read once and dy masked once (7 tensor passes instead of 8; the
// value is dy or 0, exact in T, so dx and dres are what the two-mask launches give).  Knob BN_PAIR = 0: mask in both launches.
template <typename T> struct MaskOnce {
  T *gout;                  // where the reduce launch writes dy' (NULL: nowhere)
  const T *y, *dy;          // what the apply launch reads, masks by (relu) ...
  T *dres;                  // ... and writes dy' to
  int relu;
  int64_t dy_ld;
};
template <typename T> MaskOnce<T> mask_once(bool once, const T *y, const T *dy, T *dres, int relu, int64_t dy_ld, int c) {
  if (once) return {dres, nullptr, dres, nullptr, 0, c};
  return {nullptr, y, dy, dres, relu, dy_ld};
}
template <typename T>
int bn_backward_t(const T *x, const T *y, const T *dy, int64_t n, int c, const float *gamma, const float *beta, const float *stats, int relu,
                  T *dx, T *dres, float *dgamma, float *dbeta, void *workspace, hipStream_t s, int64_t dy_ld, int64_t y_ld) {
  const NormPlan p = norm_plan(kNormBwd, n, c, dtype_of<T>(), 0, [] { return fused_resident(reinterpret_cast<const void *>(&k_bn_bwd_fused<T>)); });
  float *rows = region(workspace, p.partials), *sums = region(workspace, p.sums);
  const float inv_n = n > 0 ? 1.f / (float)n : 0.f;
  const MaskOnce<T> m = mask_once(relu == 1 && dres && n > 0 && p.path != kNormFused && tune(T_BN_PAIR) != 0, y, dy, dres, relu, dy_ld, c);
  switch (p.path) {
    case kNormFold:
      LGS_KLAUNCH((k_colreduce<T, 1>), p.reduce_grid, kNT, 0, s, x, y, dy, stats, gamma, beta, n, c, relu, p.rows_per_block, rows, dy_ld, y_ld, m.gout);
      LGS_KLAUNCH((k_bn_bwd_apply_fold<T>), p.apply_grid, kNT, 0, s, x, m.y, m.dy, n, c, gamma, beta, stats, rows, p.fold_rows, inv_n, m.relu, dx, m.dres, dgamma,
                  dbeta, m.dy_ld, y_ld);
      break;
    case kNormFused: {
      unsigned *ctr = fused_counter(s);
      LGS_REQUIRE(ctr != nullptr, "lgs_bn_backward: could not allocate the grid-barrier counters");
      LGS_KLAUNCH((k_bn_bwd_fused<T>), p.reduce_grid, kNT, 0, s, x, y, dy, n, c, gamma, beta, stats, relu, dx, dres, dgamma, dbeta, rows, sums, dy_ld, y_ld,
                  p.rows_per_block, inv_n, ctr);
      break;
    }
    default:
      LGS_KLAUNCH((k_colreduce<T, 1>), p.reduce_grid, kNT, 0, s, x, y, dy, stats, gamma, beta, n, c, relu, p.rows_per_block, rows, dy_ld, y_ld, m.gout);
      LGS_KLAUNCH(k_fold_bwd, p.fold_grid, 256, 0, s, rows, p.fold_rows, c, dgamma, dbeta, sums);
      if (p.apply_grid) LGS_KLAUNCH((k_bn_bwd_apply<T>), p.apply_grid, kNT, 0, s, x, m.y, m.dy, n, c, gamma, beta, stats, sums, inv_n, m.relu, dx, m.dres, m.dy_ld,
                                    (const float *)nullptr, y_ld);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int bn_stats_t(const T *x, int64_t n, int c, float *mean_m2, void *workspace, hipStream_t s, const float *partials, int partial_rows, const float *pivot) {
  if (!partials) partial_rows = 0;
  const NormPlan p = norm_plan(kNormStats, n, c, dtype_of<T>(), partial_rows, [] { return 0; });
  float *rows = region(workspace, p.partials);
  stats_rows<T>(p, x, n, c, partials, partial_rows, rows, s);
  LGS_KLAUNCH((k_fold_stats<T>), p.fold_grid, 256, 0, s, rows, x, p.fold_rows, c, n, mean_m2, p.from_partials, pivot);
  LGS_HIP(hipGetLastError());
  return 0;
}
template <typename T>
int bn_apply_t(const T *x, int64_t n, int c, const float *gamma, const float *beta, const float *stats, const T *res, int relu, T *y, hipStream_t s,
               int64_t y_ld) {
  const int grid = apply_blocks(n, c, Width<T>::V, 1, kApplyMaxBlocks);
  if (grid) LGS_KLAUNCH((k_bn_apply<T>), grid, kNT, 0, s, x, res, n, c, gamma, beta, stats, relu, y, y_ld);
  LGS_HIP(hipGetLastError());
  return 0;
}
template <typename T>
int bn_bwd_reduce_t(const T *x, const T *y, const T *dy, int64_t n, int c, const float *gamma, const float *beta, const float *stats, int relu,
                    float *sums, float *dgamma, float *dbeta, void *workspace, hipStream_t s, int64_t dy_ld, int64_t y_ld) {
  const NormPlan p = norm_plan(kNormBwdReduce, n, c, dtype_of<T>(), 0, [] { return 0; });
  float *rows = region(workspace, p.partials), *spill = region(workspace, p.spill);  // dgamma / dbeta land there when the caller does not want them
  LGS_KLAUNCH((k_colreduce<T, 1>), p.reduce_grid, kNT, 0, s, x, y, dy, stats, gamma, beta, n, c, relu, p.rows_per_block, rows, dy_ld, y_ld, (T *)nullptr);
  LGS_KLAUNCH(k_fold_bwd, p.fold_grid, 256, 0, s, rows, p.fold_rows, c, dgamma ? dgamma : spill + c, dbeta ? dbeta : spill, sums);
  LGS_HIP(hipGetLastError());
  return 0;
}
template <typename T>
int bn_bwd_apply_t(const T *x, const T *y, const T *dy, int64_t n, int c, const float *gamma, const float *beta, const float *stats, const float *sums,
                   float inv_n_total, const float *inv_n_dev, int relu, T *dx, T *dres, hipStream_t s, int64_t dy_ld, int64_t y_ld) {
  const int grid = apply_blocks(n, c, Width<T>::V, 1, kApplyMaxBlocks);
  if (grid) LGS_KLAUNCH((k_bn_bwd_apply<T>), grid, kNT, 0, s, x, y, dy, n, c, gamma, beta, stats, sums, inv_n_total, relu, dx, dres, dy_ld, inv_n_dev, y_ld);
  LGS_HIP(hipGetLastError());
  return 0;
}

// ---- a pair of norms on the same rows (lgs_bn_forward_pair / lgs_bn_backward_pair)
// The pair asks norm_plan() for the SINGLE-norm plan of (direction, n, c, dtype) and derives everything from it: the same
// grids and rows per workgroup (so every sum is taken in the single call's order), and two sets of partial rows / `sums` rows
// behind one another.  Where that plan says `fused`, the knob BN_PAIR is 0, or the tensor is empty, the pair entry points issue
// today's two single calls (path 0).
using NormPairPlan = lgs_norm_pair_plan_info;
inline int64_t norm_pair_workspace_bytes(int64_t n, int c) { return 2 * ((norm_workspace_bytes(n, c) + 255) / 256 * 256); }
inline int single_launches(const NormPlan &p) { return p.path == kNormFold ? 2 : p.path == kNormFused ? 1 : (p.apply_grid ? 3 : 2); }
template <typename Cap>
NormPairPlan norm_pair_plan(int dir, int64_t n, int c, int dtype, Cap &&resident_cap) {
  NormPairPlan q = {};
  const NormPlan p = norm_plan(dir, n, c, dtype, 0, resident_cap);
  q.single_path = p.path;
  q.workspace_bytes = norm_pair_workspace_bytes(n, c);
  if (p.path == kNormFused || tune(T_BN_PAIR) == 0 || n <= 0) {
    q.path = 0;
    q.launches = 2 * single_launches(p);
    return q;
  }
  q.path = p.path;
  q.launches = p.path == kNormFold ? 2 : 3;
  q.reduce_grid = p.reduce_grid; q.rows_per_block = p.rows_per_block; q.fold_rows = p.fold_rows;
  q.fold_grid = p.fold_grid; q.apply_grid = p.apply_grid;
  q.partials_a = p.partials;
  q.partials_b = {q.partials_a.offset + q.partials_a.bytes, p.partials.bytes};
  q.bytes_total = q.partials_b.offset + q.partials_b.bytes;
  if (p.sums.bytes) {
    q.sums_a = {q.bytes_total, p.sums.bytes};
    q.sums_b = {q.sums_a.offset + q.sums_a.bytes, p.sums.bytes};
    q.bytes_total = q.sums_b.offset + q.sums_b.bytes;
  }
  return q;
}

template <typename T>
int bn_forward_pair_t(const PairFwdNorm<T> &a0, const PairFwdNorm<T> &b0, int64_t n, int c, int relu, T *y, int64_t y_ld, T *res,
                      const NormPairPlan &q, void *workspace, hipStream_t s) {
  PairFwdNorm<T> a = a0, b = b0;
  a.scratch = region(workspace, q.partials_a);
  b.scratch = region(workspace, q.partials_b);
  const T *no = nullptr;
  const float *nof = nullptr;
  LGS_KLAUNCH((k_colreduce_pair<T, 0>), dim3(q.reduce_grid, 2), kNT, 0, s, a.x, no, no, nof, nof, nof, n, c, 0, q.rows_per_block,
              const_cast<float *>(a.scratch), (int64_t)c, (int64_t)c, (T *)nullptr, b.x, nof, const_cast<float *>(b.scratch));
  if (q.path == kNormFold) {
    LGS_KLAUNCH((k_bn_apply_pair<T, true>), q.apply_grid, kNT, 0, s, a, b, n, c, q.fold_rows, relu, y, y_ld, res);
  } else {
    LGS_KLAUNCH((k_fold_fwd_pair<T>), dim3(q.fold_grid, 2), 256, 0, s, a, b, q.fold_rows, c, n);
    LGS_KLAUNCH((k_bn_apply_pair<T, false>), q.apply_grid, kNT, 0, s, a, b, n, c, q.fold_rows, relu, y, y_ld, res);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T>
int bn_backward_pair_t(const PairBwdNorm<T> &a0, const PairBwdNorm<T> &b0, const T *y, const T *dy, int64_t n, int c, int relu, T *dres,
                       int64_t dy_ld, int64_t y_ld, const NormPairPlan &q, void *workspace, hipStream_t s) {
  PairBwdNorm<T> a = a0, b = b0;
  float *rows_a = region(workspace, q.partials_a), *rows_b = region(workspace, q.partials_b);
  a.scratch = rows_a; b.scratch = rows_b;
  const float inv_n = 1.f / (float)n;
  // the masked gradient, where the caller wants it, is written by the reduce launch and read back by the apply (see bn_backward_t)
  const MaskOnce<T> m = mask_once(relu == 1 && dres, y, dy, dres, relu, dy_ld, c);
  LGS_KLAUNCH((k_colreduce_pair<T, 1>), q.reduce_grid, kNT, 0, s, a.x, y, dy, a.stats, a.gamma, a.beta, n, c, relu, q.rows_per_block, rows_a, dy_ld,
              y_ld, m.gout, b.x, b.stats, rows_b);
  if (q.path == kNormFold) {
    LGS_KLAUNCH((k_bn_bwd_apply_pair<T, true>), q.apply_grid, kNT, 0, s, a, b, m.y, m.dy, n, c, q.fold_rows, inv_n, m.relu, m.dres, m.dy_ld, y_ld);
  } else {
    float *sums_a = region(workspace, q.sums_a), *sums_b = region(workspace, q.sums_b);
    a.sums = sums_a; b.sums = sums_b;
    LGS_KLAUNCH(k_fold_bwd_pair, dim3(q.fold_grid, 2), 256, 0, s, rows_a, rows_b, q.fold_rows, c, a.dgamma, a.dbeta, sums_a, b.dgamma, b.dbeta, sums_b);
    LGS_KLAUNCH((k_bn_bwd_apply_pair<T, false>), q.apply_grid, kNT, 0, s, a, b, m.y, m.dy, n, c, q.fold_rows, inv_n, m.relu, m.dres, m.dy_ld, y_ld);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // namespace lgs

using namespace lgs;

extern "C" {

int lgs_bn_stats(const void *x, int64_t n, int c, float *mean_m2, int dtype, void *workspace, const float *conv_partials,
                 int conv_partial_rows, const float *pivot, void *stream) {
  LGS_REQUIRE(x && mean_m2 && workspace, "lgs_bn_stats: null argument");
  return with_elem(dtype, c, "lgs_bn_stats", [&](auto e) {
    return bn_stats_t(e.in(x), n, c, mean_m2, workspace, (hipStream_t)stream, conv_partials, conv_partial_rows, pivot);
  });
}
int lgs_bn_apply(const void *x, int64_t n, int c, const float *gamma, const float *beta, const float *stats,
                 const void *residual, int relu, void *y, int dtype, int64_t y_row_stride, void *stream) {
  LGS_REQUIRE(x && y && gamma && beta && stats, "lgs_bn_apply: null argument");
  LGS_BN_STRIDE("lgs_bn_apply", y, y_row_stride, y_ld);
  return with_elem(dtype, c, "lgs_bn_apply", [&](auto e) {
    return bn_apply_t(e.in(x), n, c, gamma, beta, stats, e.in(residual), relu, e.out(y), (hipStream_t)stream, y_ld);
  });
}
int lgs_bn_sync_combine(const float *all_stats, int world, int c, float eps, float momentum, float *running_mean,
                        float *running_var, int64_t *num_batches_tracked, float *stats, float *inv_n_total, void *stream) {
  LGS_REQUIRE(all_stats && stats && world > 0 && c > 0, "lgs_bn_sync_combine: bad argument");
  LGS_KLAUNCH(k_sync_combine, (unsigned)((c + 127) / 128), 128, 0, (hipStream_t)stream, all_stats, world, c, eps, momentum,
                     running_mean, running_var, reinterpret_cast<long long *>(num_batches_tracked), stats, inv_n_total);
  LGS_HIP(hipGetLastError());
  return 0;
}
int lgs_bn_backward_reduce(const void *x, const void *y, const void *dy, int64_t n, int c, const float *gamma,
                           const float *beta, const float *stats, int relu, float *sums, float *dgamma, float *dbeta, int dtype,
                           void *workspace, int64_t dy_row_stride, int64_t y_row_stride, void *stream) {
  LGS_REQUIRE(x && dy && stats && sums && workspace, "lgs_bn_backward_reduce: null argument");
  LGS_BN_STRIDE("lgs_bn_backward_reduce", dy, dy_row_stride, dy_ld);
  LGS_BN_STRIDE("lgs_bn_backward_reduce", y, y_row_stride, y_ld);
  LGS_REQUIRE(relu != 1 || y, "lgs_bn_backward_reduce: relu mode 1 needs the forward output");
  LGS_REQUIRE(relu != 2 || (gamma && beta), "lgs_bn_backward_reduce: relu mode 2 needs gamma and beta");
  return with_elem(dtype, c, "lgs_bn_backward_reduce", [&](auto e) {
    return bn_bwd_reduce_t(e.in(x), e.in(y), e.in(dy), n, c, gamma, beta, stats, relu, sums, dgamma, dbeta, workspace, (hipStream_t)stream, dy_ld, y_ld);
  });
}
int lgs_bn_backward_apply(const void *x, const void *y, const void *dy, int64_t n, int c, const float *gamma,
                          const float *beta, const float *stats, const float *sums, float inv_n_total,
                          const float *inv_n_device, int relu, void *dx, void *dresidual, int dtype, int64_t dy_row_stride,
                          int64_t y_row_stride, void *stream) {
  LGS_REQUIRE(x && dy && dx && gamma && stats && sums, "lgs_bn_backward_apply: null argument");
  LGS_BN_STRIDE("lgs_bn_backward_apply", dy, dy_row_stride, dy_ld);
  LGS_BN_STRIDE("lgs_bn_backward_apply", y, y_row_stride, y_ld);
  LGS_REQUIRE(relu != 1 || y, "lgs_bn_backward_apply: relu mode 1 needs the forward output");
  LGS_REQUIRE(relu != 2 || beta, "lgs_bn_backward_apply: relu mode 2 needs beta");
  return with_elem(dtype, c, "lgs_bn_backward_apply", [&](auto e) {
    return bn_bwd_apply_t(e.in(x), e.in(y), e.in(dy), n, c, gamma, beta, stats, sums, inv_n_total, inv_n_device, relu, e.out(dx), e.out(dresidual),
                          (hipStream_t)stream, dy_ld, y_ld);
  });
}

int64_t lgs_bn_workspace_bytes(int64_t n, int c) { return norm_workspace_bytes(n, c); }

int lgs_bn_forward(const void *x, int64_t n, int c, const float *gamma, const float *beta, float eps, float momentum,
                   float *running_mean, float *running_var, int64_t *num_batches_tracked, const void *residual, int relu,
                   void *y, float *stats, int dtype, void *workspace, const float *conv_partials, int conv_partial_rows,
                   const float *pivot, int64_t y_row_stride, void *stream) {
  LGS_REQUIRE(x && y && gamma && beta && stats && workspace, "lgs_bn_forward: null argument");
  LGS_BN_STRIDE("lgs_bn_forward", y, y_row_stride, y_ld);
  return with_elem(dtype, c, "lgs_bn_forward", [&](auto e) {
    return bn_forward_t(e.in(x), n, c, gamma, beta, eps, momentum, running_mean, running_var, reinterpret_cast<long long *>(num_batches_tracked),
                        e.in(residual), relu, e.out(y), stats, workspace, (hipStream_t)stream, conv_partials, conv_partial_rows, pivot, y_ld);
  });
}

int lgs_bn_backward(const void *x, const void *y, const void *dy, int64_t dy_row_stride, int64_t n, int c, const float *gamma,
                    const float *beta, const float *stats, int relu, void *dx, void *dresidual, float *dgamma, float *dbeta,
                    int dtype, void *workspace, int64_t y_row_stride, void *stream) {
  LGS_REQUIRE(x && dy && dx && gamma && stats && dgamma && dbeta && workspace, "lgs_bn_backward: null argument");
  LGS_BN_STRIDE("lgs_bn_backward", dy, dy_row_stride, dy_ld);
  LGS_BN_STRIDE("lgs_bn_backward", y, y_row_stride, y_ld);
  LGS_REQUIRE(relu != 1 || y, "lgs_bn_backward: relu mode 1 needs the forward output");
  LGS_REQUIRE(relu != 2 || beta, "lgs_bn_backward: relu mode 2 needs beta");
  return with_elem(dtype, c, "lgs_bn_backward", [&](auto e) {
    return bn_backward_t(e.in(x), e.in(y), e.in(dy), n, c, gamma, beta, stats, relu, e.out(dx), e.out(dresidual), dgamma, dbeta, workspace,
                         (hipStream_t)stream, dy_ld, y_ld);
  });
}

int64_t lgs_bn_pair_workspace_bytes(int64_t n, int c) { return norm_pair_workspace_bytes(n, c); }

// the pair's plan for a call on the current device (asks it for the resident-workgroup bound where the single plan would)
int lgs_bn_pair_plan(int direction, int64_t n, int c, int dtype, lgs_norm_pair_plan_info *out) {
  LGS_REQUIRE(out && (direction == kNormFwd || direction == kNormBwd) && n >= 0, "lgs_bn_pair_plan: bad argument");
  return with_elem(dtype, c, "lgs_bn_pair_plan", [&](auto e) {
    using T = typename decltype(e)::T;
    *out = norm_pair_plan(direction, n, c, dtype, [&] {
      return fused_resident(direction == kNormFwd ? reinterpret_cast<const void *>(&k_bn_fwd_fused<T>) : reinterpret_cast<const void *>(&k_bn_bwd_fused<T>));
    });
    return 0;
  });
}
int lgs_debug_norm_pair_plan(const lgs_norm_plan_query *q, lgs_norm_pair_plan_info *out) {
  LGS_REQUIRE(q && out && (q->direction == kNormFwd || q->direction == kNormBwd) && q->n >= 0, "lgs_debug_norm_pair_plan: bad argument");
  return with_elem(q->dtype, q->c, "lgs_debug_norm_pair_plan", [&](auto) {
    *out = norm_pair_plan(q->direction, q->n, q->c, q->dtype, [&] { return q->resident_cap; });
    return 0;
  });
}

int lgs_bn_forward_pair(const void *xa, const lgs_bn_params *na, float *stats_a, const void *xb, const lgs_bn_params *nb, float *stats_b,
                        int64_t n, int c, int relu, void *y, int64_t y_row_stride, void *res, int dtype, void *workspace, void *stream) {
  LGS_REQUIRE(xa && xb && na && nb && na->gamma && na->beta && nb->gamma && nb->beta && stats_a && stats_b && y && workspace && n >= 0,
              "lgs_bn_forward_pair: null argument");
  LGS_BN_STRIDE("lgs_bn_forward_pair", y, y_row_stride, y_ld);
  lgs_norm_pair_plan_info q;
  int rc;
  if ((rc = lgs_bn_pair_plan(kNormFwd, n, c, dtype, &q))) return rc;
  if (q.path == 0) {      // today's two calls; the branch output is their intermediate
    LGS_REQUIRE(res, "lgs_bn_forward_pair: this call runs as two single norms (lgs_bn_pair_plan: path 0) and needs the res buffer");
    if ((rc = lgs_bn_forward(xb, n, c, nb->gamma, nb->beta, nb->eps, nb->momentum, nb->running_mean, nb->running_var, nb->num_batches_tracked,
                             nullptr, 0, res, stats_b, dtype, workspace, nullptr, 0, nullptr, 0, stream))) return rc;
    return lgs_bn_forward(xa, n, c, na->gamma, na->beta, na->eps, na->momentum, na->running_mean, na->running_var, na->num_batches_tracked,
                          res, relu, y, stats_a, dtype, workspace, nullptr, 0, nullptr, y_row_stride, stream);
  }
  return with_elem(dtype, c, "lgs_bn_forward_pair", [&](auto e) {
    using T = typename decltype(e)::T;
    const PairFwdNorm<T> a = {e.in(xa), na->gamma, na->beta, na->running_mean, na->running_var, reinterpret_cast<long long *>(na->num_batches_tracked),
                              stats_a, nullptr, na->eps, na->momentum};
    const PairFwdNorm<T> b = {e.in(xb), nb->gamma, nb->beta, nb->running_mean, nb->running_var, reinterpret_cast<long long *>(nb->num_batches_tracked),
                              stats_b, nullptr, nb->eps, nb->momentum};
    return bn_forward_pair_t<T>(a, b, n, c, relu, e.out(y), y_ld, e.out(res), q, workspace, (hipStream_t)stream);
  });
}

int lgs_bn_backward_pair(const void *xa, const void *ya, const float *gamma_a, const float *beta_a, const float *stats_a, int relu,
                         const void *xb, const float *gamma_b, const float *stats_b, const void *dy, int64_t dy_row_stride, int64_t n, int c,
                         void *dxa, void *dxb, float *dgamma_a, float *dbeta_a, float *dgamma_b, float *dbeta_b, void *dresidual, int dtype,
                         void *workspace, int64_t ya_row_stride, void *stream) {
  LGS_REQUIRE(xa && xb && dy && dxa && dxb && gamma_a && gamma_b && stats_a && stats_b && dgamma_a && dbeta_a && dgamma_b && dbeta_b && workspace &&
                  n >= 0, "lgs_bn_backward_pair: null argument");
  LGS_BN_STRIDE("lgs_bn_backward_pair", dy, dy_row_stride, dy_ld);
  LGS_BN_STRIDE("lgs_bn_backward_pair", ya, ya_row_stride, y_ld);
  LGS_REQUIRE(relu == 0 || relu == 1, "lgs_bn_backward_pair: relu is 0 or 1 (a mask recomputed from xa alone would ignore the added branch)");
  LGS_REQUIRE(relu != 1 || ya, "lgs_bn_backward_pair: relu mode 1 needs the forward output");
  lgs_norm_pair_plan_info q;
  int rc;
  if ((rc = lgs_bn_pair_plan(kNormBwd, n, c, dtype, &q))) return rc;
  if (q.path == 0) {      // today's two calls; the masked gradient is their intermediate
    LGS_REQUIRE(dresidual, "lgs_bn_backward_pair: this call runs as two single norms (lgs_bn_pair_plan: path 0) and needs the dresidual buffer");
    if ((rc = lgs_bn_backward(xa, ya, dy, dy_row_stride, n, c, gamma_a, beta_a, stats_a, relu, dxa, dresidual, dgamma_a, dbeta_a, dtype, workspace,
                              ya_row_stride, stream))) return rc;
    return lgs_bn_backward(xb, nullptr, dresidual, 0, n, c, gamma_b, nullptr, stats_b, 0, dxb, nullptr, dgamma_b, dbeta_b, dtype, workspace, 0, stream);
  }
  return with_elem(dtype, c, "lgs_bn_backward_pair", [&](auto e) {
    using T = typename decltype(e)::T;
    const PairBwdNorm<T> a = {e.in(xa), gamma_a, beta_a, stats_a, nullptr, nullptr, dgamma_a, dbeta_a, e.out(dxa)};
    const PairBwdNorm<T> b = {e.in(xb), gamma_b, nullptr, stats_b, nullptr, nullptr, dgamma_b, dbeta_b, e.out(dxb)};
    return bn_backward_pair_t<T>(a, b, e.in(ya), e.in(dy), n, c, relu, e.out(dresidual), dy_ld, y_ld, q, workspace, (hipStream_t)stream);
  });
}

// the plan of a call given by plain integers, resident-workgroup cap included: no HIP call (tests/test_norm_plan_cpu.py)
int lgs_debug_norm_plan(const lgs_norm_plan_query *q, lgs_norm_plan_info *out) {
  LGS_REQUIRE(q && out && q->direction >= kNormFwd && q->direction <= kNormBwdReduce && q->n >= 0 && q->conv_partial_rows >= 0,
              "lgs_debug_norm_plan: bad argument");
  return with_elem(q->dtype, q->c, "lgs_debug_norm_plan", [&](auto) {
    *out = norm_plan(q->direction, q->n, q->c, q->dtype, q->conv_partial_rows, [&] { return q->resident_cap; });
    return 0;
  });
}

}  // extern "C"
