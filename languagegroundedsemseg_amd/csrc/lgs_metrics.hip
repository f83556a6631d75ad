// lgs_metrics.hip -- segmentation metrics of a step in one pass over the [N, C] scores, gfx950.
//
// Replaces what the reference's eval_step runs after the loss on every training and validation step
//   lib/train_test/pl_BaselineTrainer.py:357-378 (pred = soutput.F.max(1)[1], prob = softmax(soutput.F, 1), the confusion matrix)
// HBM-bound like k_ce_fwd_bwd (lgs_loss.hip), with the same access shape (lgs_classrows.h): half a wavefront per row, 16-byte loads, Q x R = 4
// chunks in flight per lane.  The scores are read once; the pass writes pred[n] (8 bytes per row), prob[n, c] if asked, and adds the
// rows' (label, pred) cells to an int64 [c, c] matrix that lives on the device across steps.
//
// The matrix is the one part with no counterpart in the loss kernel.  Real batches put a third of their rows on two cells, so one
// global atomic per row is a million adds on a handful of addresses.  Three levels of combining before an add leaves the CU:
//   1. a half-wave merges equal keys among its R consecutive rows (Morton order: neighbours share labels) in registers;
//   2. a workgroup keeps an open-addressed table of kSlots (key, count) pairs in LDS for ALL the tiles it walks; a key that finds no
//      slot within kProbe steps goes to global memory directly;
//   3. the launch has at most METRICS_BLOCKS (8192) workgroups, each walking tiles blockIdx.x, + gridDim.x, ...: a cell costs one global
//      add per workgroup that saw it, however many rows hit it.  (One tile per workgroup: 497 us at 1.2 M x 200 bf16 with 90 % of the
//      rows on one cell, 220 us with the cap; a cap of 2048 leaves two uneven rounds of resident workgroups: 273 - 373 us.)
// All sums are integers: any order gives the same matrix, bit for bit.
#include <limits.h>

#include <algorithm>

#include "lgs_classrows.h"

namespace lgs {

namespace {

constexpr int kSlots = 256;        // LDS table entries per workgroup (one per thread for the flush)
constexpr int kProbe = 8;          // linear probes before a key goes to global memory
constexpr float kNegInf = -__builtin_huge_valf();

// count `add` rows of cell `key`: the workgroup's table first, global memory when the probe sequence is taken by other keys
__device__ inline void cell_add(int32_t *l_key, uint32_t *l_cnt, int32_t key, uint32_t add, unsigned long long *confmat) {
  uint32_t slot = ((uint32_t)key * 2654435761u) >> 24;     // kSlots == 256
#pragma unroll 1
  for (int p = 0; p < kProbe; ++p) {
    const int32_t prev = atomicCAS(&l_key[slot], -1, key);
    if (prev == -1 || prev == key) {
      atomicAdd(&l_cnt[slot], add);
      return;
    }
    slot = (slot + 1) & (kSlots - 1);
  }
  atomicAdd(confmat + key, (unsigned long long)add);
}

// A tile is 8 half-waves x R rows.  pred follows torch.max(x, 1)[1]: the lowest index among the maxima, the first NaN if there is one
// (a NaN beats every number), 0 for a row of -inf only.  PROB: softmax in fp32 from the values as stored, exact expf and a division.
template <typename T, int Q, int R, bool PROB>
__global__ __launch_bounds__(256) void k_seg_metrics(const T *__restrict__ scores, int64_t n, int c, const int64_t *__restrict__ labels,
                                                     int64_t ignore_index, int64_t *__restrict__ pred, float *__restrict__ prob,
                                                     unsigned long long *__restrict__ confmat) {
  constexpr int W = Width<T>::V;
  __shared__ int32_t l_key[kSlots];
  __shared__ uint32_t l_cnt[kSlots];
  l_key[threadIdx.x] = -1;
  l_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 31;
  const int hw = threadIdx.x >> 5;
  // rows that are no multiple of 16 bytes (13 classes; 20 in bf16) and unaligned views take element-wise accesses: kernel-uniform
  const bool vec = (c % W) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0 && (reinterpret_cast<uintptr_t>(prob) & 15) == 0;
  const int nchunk = (c + W - 1) / W;
  const int64_t ntiles = (n + 8 * R - 1) / (8 * R);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (tile * 8 + hw) * R;
    if (row0 >= n) continue;          // (uniform per half-wave: the shuffles below stay inside it)
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
            ldv<W>(scores + row * c + ch * W, v[r][q]);
          } else {
#pragma unroll
            for (int i = 0; i < W; ++i) v[r][q][i] = ch * W + i < c ? ld_elem(scores + row * c + ch * W + i) : kNegInf;
          }
        }
      }
    }
    int32_t keys[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + r;
      keys[r] = -1;
      if (row >= n) continue;
      // this lane's candidate: its elements come in rising index order, so "strictly better" keeps the first of equals and the first NaN
      float bv = kNegInf;
      int bi = INT_MAX;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int ch = q * 32 + lane;
        if (ch < nchunk) {
#pragma unroll
          for (int i = 0; i < W; ++i) {
            const float x = v[r][q][i];
            const bool take = (x > bv) || (x != x && bv == bv);
            if (take && (vec || ch * W + i < c)) { bv = x; bi = ch * W + i; }
          }
        }
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 32);
        const int oi = __shfl_xor(bi, o, 32);
        const bool on = ov != ov, mn = bv != bv;
        const bool take = on ? (!mn || oi < bi) : (!mn && (ov > bv || (ov == bv && oi < bi)));
        if (take) { bv = ov; bi = oi; }
      }
      const int p = bi == INT_MAX ? 0 : bi;      // nothing above -inf
      const int64_t lab = labs[r];
      if (lab != ignore_index && lab >= 0 && lab < c) keys[r] = (int32_t)lab * c + p;
      if (lane == 0) pred[row] = p;
      if (PROB) {
        const float mx = bi == INT_MAX ? kNegInf : bv;
        float se = 0.f;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int ch = q * 32 + lane;
          if (ch < nchunk) {
#pragma unroll
            for (int i = 0; i < W; ++i) {
              const float e = expf(v[r][q][i] - mx);      // padding lanes hold -inf: exp = 0 (never stored)
              se += e;
              v[r][q][i] = e;
            }
          }
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) se += __shfl_xor(se, o, 32);
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int ch = q * 32 + lane;
          if (ch < nchunk) {
            float *dst = prob + row * c + ch * W;
            if (vec) {
#pragma unroll
              for (int i = 0; i < W; i += 4)
                *reinterpret_cast<float4 *>(dst + i) = make_float4(v[r][q][i] / se, v[r][q][i + 1] / se, v[r][q][i + 2] / se, v[r][q][i + 3] / se);
            } else {
#pragma unroll
              for (int i = 0; i < W; ++i)
                if (ch * W + i < c) dst[i] = v[r][q][i] / se;
            }
          }
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (keys[r] < 0) continue;
        uint32_t add = 1;
#pragma unroll
        for (int s = r + 1; s < R; ++s)
          if (keys[s] == keys[r]) { ++add; keys[s] = -1; }
        cell_add(l_key, l_cnt, keys[r], add, confmat);
      }
    }
  }
  __syncthreads();
  if (l_key[threadIdx.x] >= 0) atomicAdd(confmat + l_key[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" int lgs_seg_metrics(const void *scores, int64_t n, int c, const int64_t *labels, int64_t ignore_index, int64_t *pred,
                               float *prob, int64_t *confmat, int dtype, void *stream) {
  LGS_REQUIRE(confmat && n >= 0 && ((scores && labels && pred) || n == 0), "lgs_seg_metrics: null argument");
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_seg_metrics: unknown dtype");
  int q;
  if (int rc = class_shape(c, dtype, "lgs_seg_metrics", &q)) return rc;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const int64_t max_blocks = std::min<int64_t>(std::max<int64_t>(tune(T_METRICS_BLOCKS), 1), 65536);
  unsigned long long *cm = reinterpret_cast<unsigned long long *>(confmat);
  // a tile is 32 / 16 / 8 rows
  const int rc = with_class_rows<2>(dtype, q, prob ? 1 : 0, "lgs_seg_metrics", [&](auto e, auto want_prob) {
    using E = decltype(e);
    LGS_KLAUNCH((k_seg_metrics<typename E::T, E::Q, E::R, decltype(want_prob)::value != 0>), (unsigned)std::min<int64_t>(e.tiles(n), max_blocks),
                256, 0, s, e.in(scores), n, c, labels, ignore_index, pred, prob, cm);
    return 0;
  });
  if (rc) return rc;
  LGS_HIP(hipGetLastError());
  return 0;
}
