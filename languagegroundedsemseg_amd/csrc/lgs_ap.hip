// lgs_ap.hip -- per-class average precision of a step's [N, C] scores: sorted positives, one counting pass; gfx950.
//
// Replaces what the reference's validation step runs on `prob` after the loss
//   lib/train_test/pl_BaselineTrainer.py:380, downstream/insseg/lib/pl_Trainer.py:316 (AveragePrecision(num_classes, average=None)),
//   downstream/insseg/lib/test.py:58-62, :215 (sklearn's average_precision_score per class)
// which is an order statistic per class: C sorts of N scores.  With P_c positives in class c, sklearn's step-wise sum over distinct
// thresholds equals
//   AP_c = (1 / P_c) sum over the positives i of c of  TP_c(s_i) / Rank_c(s_i),    s_i = prob[i, c]
//   TP_c(s) = #{ j : label_j = c, prob[j, c] >= s },   Rank_c(s) = #{ j : prob[j, c] >= s }  (all N rows: ignored rows are negatives)
// so only the positives are sorted (at most N keys over all classes together) and every other element of the matrix is COUNTED
// against the sorted positives of its column.  Stages, all on the caller's stream, no host synchronisation:
//   1. keys      one 64-bit key per row: (label << 32) | ord(prob[i, label]) for a counted row, all ones otherwise.  Probabilities
//                as input: a gather, one thread per row (k_ap_keys).  Logits: a class-row pass (lgs_classrows.h) that computes the
//                row's softmax as k_seg_metrics<PROB> does and leaves (max, sum) per row for pass 2 (k_ap_softmax_keys).
//   2. sort      rocprim::radix_sort_keys over bits [0, 32 + bits(c)); the segment starts and minima are c + 1 binary searches
//                (k_ap_offsets: the keys carry the class, so no histogram and no scan of counts is needed).
//   3. rank      the hot path, one more read of [N, C]: an element below its column's lowest positive ends at one compare; the others
//                search the column's sorted positives for the highest one that is <= the element and add 1 to that positive's
//                counter.  A lane runs the searches of the W elements of a 16-byte chunk together (W independent load chains).
//                Small inputs (n c < 2^19): the class-row shape, plain global uint32 atomics (k_ap_rank).  Big ones: scattered
//                global adds are what bounds that form (one 64-byte request each, 13 G per second measured), so a workgroup owns
//                the W columns of one chunk over a slab of rows and keeps their counters in LDS (k_ap_rank_cols).
//   4. finish    an inclusive scan of the counters (rocprim; the sums wrap mod 2^32 and every DIFFERENCE that is used is a Rank <= N),
//                one term TP / Rank per positive in fp64 (k_ap_terms: all positives of equal key share the TP and Rank of the tie
//                group's first slot), and one workgroup per class that adds the terms in a fixed order (k_ap_finish).
// Every count is an integer and the fp64 sums have one order: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cstring>
#include <rocprim/rocprim.hpp>

#include <algorithm>

#include "lgs_classrows.h"

namespace lgs {

namespace {

constexpr float kNegInf = -__builtin_huge_valf();
constexpr uint64_t kNoKey = ~0ull;
constexpr int kMaxClasses = 32 * kClassChunks * 8;     // class_shape's widest head (bf16)
constexpr int64_t kRankBlocks = 4096;                  // workgroups of the two class-row passes: each walks tiles b, b + grid, ...
constexpr int kColThreads = 1024;                      // k_ap_rank_cols: one workgroup of 16 waves per CU,
constexpr int kColSlots = 65536;                       //   128 KiB of packed 16-bit counters,
constexpr int kColSplit = 4096;                        //   16 KiB of splitters: every 16th key of the run (evenly spaced ones of a longer run),
constexpr int64_t kColRows = 60 * kColThreads;         //   at most 61 440 (< 2^16) rows per slab
constexpr int64_t kColMinElems = 1 << 19;              // n c from which the rank pass keeps its counters in LDS

// ord_key with -0 counted as +0: sklearn compares scores as numbers, and the plain map would rank a -0.0 below a +0.0
// (the zero is chosen on the bit pattern, as it always was: that keeps the instruction streams of the class-row kernels)
__device__ inline uint32_t ord_of(float f) { return ord_key_of_bits(f == 0.f ? 0u : __float_as_uint(f)); }
__device__ inline bool counted(int64_t lab, int64_t ignore_index, int c) { return lab != ignore_index && lab >= 0 && lab < c; }
__device__ inline uint32_t key_lo(const uint64_t *__restrict__ k, int64_t i) { return (uint32_t)k[i]; }

// stage 1, probabilities: the row's own-class score
template <typename T>
__global__ __launch_bounds__(256) void k_ap_keys(const T *__restrict__ scores, int64_t n, int c, const int64_t *__restrict__ labels,
                                                 int64_t ignore_index, uint64_t *__restrict__ keys) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const int64_t lab = labels[row];
  keys[row] = counted(lab, ignore_index, c) ? ((uint64_t)lab << 32) | ord_of(ld_elem(scores + row * c + lab)) : kNoKey;
}

// stage 1, logits: the softmax of k_seg_metrics<PROB> (the maximum, expf(x - max) in place, per-lane sums in q-then-i order, the xor
// butterfly 16 .. 1, e / se) for the row's own class; rowstat[row] = (max, se)
template <typename T, int Q, int R>
__global__ __launch_bounds__(256) void k_ap_softmax_keys(const T *__restrict__ scores, int64_t n, int c, const int64_t *__restrict__ labels,
                                                         int64_t ignore_index, uint64_t *__restrict__ keys, float2 *__restrict__ rowstat) {
  constexpr int W = Width<T>::V;
  const int lane = threadIdx.x & 31;
  const int hw = threadIdx.x >> 5;
  const bool vec = (c % W) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0;
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
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + r;
      if (row >= n) continue;
      float mx = kNegInf;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int ch = q * 32 + lane;
        if (ch < nchunk) {
#pragma unroll
          for (int i = 0; i < W; ++i)
            if (v[r][q][i] > mx) mx = v[r][q][i];
        }
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 32);
        if (ov > mx) mx = ov;
      }
      float se = 0.f;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int ch = q * 32 + lane;
        if (ch < nchunk) {
#pragma unroll
          for (int i = 0; i < W; ++i) {
            const float e = expf(v[r][q][i] - mx);      // padding elements hold -inf: exp = 0
            se += e;
            v[r][q][i] = e;
          }
        }
      }
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) se += __shfl_xor(se, o, 32);
      const int64_t lab = labs[r];
      const bool cnt = counted(lab, ignore_index, c);
      if (lane == 0) {
        rowstat[row] = make_float2(mx, se);
        if (!cnt) keys[row] = kNoKey;
      }
      if (cnt) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const int ch = q * 32 + lane;
#pragma unroll
          for (int i = 0; i < W; ++i)
            if (ch * W + i == (int)lab) keys[row] = ((uint64_t)lab << 32) | ord_of(v[r][q][i] / se);      // one lane, one element
        }
      }
    }
  }
}

// stage 2b: off[t] = first sorted key of class >= t, t in [0, c] (off[c] = the number of positives); mn[t] = the lowest positive of t
__global__ void k_ap_offsets(const uint64_t *__restrict__ skeys, int64_t n, int c, uint32_t *__restrict__ off, uint32_t *__restrict__ mn) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > c) return;
  const uint64_t k = (uint64_t)t << 32;
  int64_t lo = 0, hi = n;      // lower_bound, spelled out here and in k_ap_terms: a case measured outside the parent's spread with the helper
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (skeys[mid] < k) lo = mid + 1; else hi = mid;
  }
  off[t] = (uint32_t)lo;
  if (t < c) mn[t] = lo < n ? key_lo(skeys, lo) : 0xffffffffu;      // (read only where the segment is not empty)
}

// stage 3.  LOGITS: the element is expf(x - max) / se with the row's pair from stage 1 -- the expressions of k_seg_metrics<PROB>.
template <typename T, int Q, int R, bool LOGITS>
__global__ __launch_bounds__(256) void k_ap_rank(const T *__restrict__ scores, int64_t n, int c, const float2 *__restrict__ rowstat,
                                                 const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ off,
                                                 const uint32_t *__restrict__ mn, uint32_t *__restrict__ cnt) {
  constexpr int W = Width<T>::V;
  __shared__ uint32_t l_off[kMaxClasses + 1];
  __shared__ uint32_t l_min[kMaxClasses];
  for (int t = threadIdx.x; t <= c; t += 256) {
    l_off[t] = off[t];
    if (t < c) l_min[t] = mn[t];
  }
  __syncthreads();
  const int lane = threadIdx.x & 31;
  const int hw = threadIdx.x >> 5;
  const bool vec = (c % W) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0;
  const int nchunk = (c + W - 1) / W;
  const int64_t ntiles = (n + 8 * R - 1) / (8 * R);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (tile * 8 + hw) * R;
    if (row0 >= n) continue;
    float v[R][Q][W];
    float2 st[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int64_t row = row0 + r;
      if (LOGITS) st[r] = row < n ? rowstat[row] : make_float2(0.f, 1.f);
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
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int ch = q * 32 + lane;
        if (ch >= nchunk || row0 + r >= n) continue;
        // the W searches of this chunk side by side: [base, base + len) always holds the answer and key[base] <= the element
        uint32_t o[W], base[W], len[W];
        uint32_t longest = 0;
#pragma unroll
        for (int i = 0; i < W; ++i) {
          const int cls = ch * W + i;
          const bool in = cls < c;
          const int k = in ? cls : 0;
          float p = v[r][q][i];
          if (LOGITS) p = expf(p - st[r].x) / st[r].y;
          o[i] = ord_of(p);
          const uint32_t lo = l_off[k], hi = l_off[k + 1];
          const bool live = in && hi > lo && o[i] >= l_min[k];
          base[i] = lo;
          len[i] = live ? hi - lo : 0;
          longest = len[i] > longest ? len[i] : longest;
        }
        if (longest == 0) continue;
        while (longest > 1) {
#pragma unroll
          for (int i = 0; i < W; ++i) {
            const uint32_t half = len[i] >> 1;
            if (half > 0) {
              const bool up = key_lo(skeys, (int64_t)base[i] + half) <= o[i];
              base[i] += up ? half : 0;
              len[i] = up ? len[i] - half : half;
            }
          }
          longest -= longest >> 1;
        }
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (len[i] > 0) atomicAdd(cnt + base[i], 1u);
      }
    }
  }
}

// stage 3 for big inputs: the counters in LDS.  Workgroup (x, y) owns the W columns of 16-byte chunk x -- whose sorted positives are ONE
// run of L slots, the classes being adjacent -- and the rows of slab y, one row per thread and step.  A slot receives at most one add
// per row, so with at most kColRows rows per slab a 16-bit counter cannot overflow: two per LDS word, flushed with one global add per
// slot that was hit.  A run longer than kColSlots (a hot class) combines its adds in a table of (slot, count) pairs instead.  Either
// way kColSplit splitters of the run in LDS take the upper levels of every search.
template <typename T, bool LOGITS>
__global__ __launch_bounds__(kColThreads) void k_ap_rank_cols(const T *__restrict__ scores, int64_t n, int c, int64_t slab_rows,
                                                              const float2 *__restrict__ rowstat, const uint64_t *__restrict__ skeys,
                                                              const uint32_t *__restrict__ off, const uint32_t *__restrict__ mn,
                                                              uint32_t *__restrict__ cnt) {
  constexpr int W = Width<T>::V;
  __shared__ uint32_t l_cnt[kColSlots / 2];
  __shared__ uint32_t l_spl[kColSplit];                 // every step-th key of the run: the upper levels of every search
  const int c0 = blockIdx.x * W;
  const uint32_t s0 = off[c0], L = off[c0 + W < c ? c0 + W : c] - s0;
  if (L == 0) return;               // (the whole workgroup: none of its columns has a positive)
  const bool lds = L <= (uint32_t)kColSlots;
  const uint32_t step = lds ? 16u : (L + kColSplit - 1) / kColSplit;      // (16 keys of 8 bytes are one 128-byte line)
  // a longer run: the same LDS as an open-addressed table of kColSlots / 4 (slot, count) pairs -- the rows that score a hot class
  // lowest all land on its first few slots, and a million global adds on a handful of addresses take milliseconds
  uint32_t *const t_key = l_cnt, *const t_cnt = l_cnt + kColSlots / 4;
  if (lds) {
    for (uint32_t j = threadIdx.x; j < (L + 1) / 2; j += kColThreads) l_cnt[j] = 0;
  } else {
    for (uint32_t j = threadIdx.x; j < (uint32_t)kColSlots / 4; j += kColThreads) { t_key[j] = 0xffffffffu; t_cnt[j] = 0; }
  }
  for (uint32_t j = threadIdx.x; j < (L + step - 1) / step; j += kColThreads) l_spl[j] = key_lo(skeys, (int64_t)s0 + (int64_t)j * step);
  __syncthreads();
  uint32_t lo[W], seg[W], low[W];   // per column: first slot, positives, lowest positive (uniform)
  uint32_t sp0[W], spn[W];          // and the run's splitters that lie inside the column: the first, how many
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const int k = c0 + i < c ? c0 + i : c - 1;
    lo[i] = off[k];
    seg[i] = c0 + i < c ? off[k + 1] - lo[i] : 0;
    low[i] = mn[k];
    sp0[i] = (lo[i] - s0 + step - 1) / step;
    const uint32_t last = seg[i] > 0 ? (lo[i] + seg[i] - 1 - s0) / step : 0;
    spn[i] = seg[i] > 0 && last >= sp0[i] ? last - sp0[i] + 1 : 0;
  }
  const bool vec = (c % W) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0;
  const int64_t r0 = (int64_t)blockIdx.y * slab_rows, r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
  for (int64_t row = r0 + threadIdx.x; row < r1; row += kColThreads) {
    float v[W];
    if (vec) {
      ldv<W>(scores + row * c + c0, v);
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) v[i] = c0 + i < c ? ld_elem(scores + row * c + c0 + i) : kNegInf;
    }
    float2 st = make_float2(0.f, 1.f);
    if (LOGITS) st = rowstat[row];
    uint32_t o[W], base[W], len[W];
    uint32_t longest = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      float p = v[i];
      if (LOGITS) p = expf(p - st.x) / st.y;
      o[i] = ord_of(p);
      base[i] = lo[i];
      len[i] = seg[i] > 0 && o[i] >= low[i] ? seg[i] : 0;
    }
    // the splitters in LDS first: the highest one of the column that is <= the element leaves at most `step` keys to global memory
    // (one 128-byte line of them while the counters are in LDS); an element below the column's first splitter searches the slots in
    // front of it
    uint32_t sb[W], sl[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
      sb[i] = sp0[i];
      sl[i] = 0;
      if (len[i] > 0 && spn[i] > 0) {
        if (l_spl[sp0[i]] <= o[i]) sl[i] = spn[i];
        else len[i] = s0 + sp0[i] * step - lo[i];
      }
      longest = sl[i] > longest ? sl[i] : longest;
    }
    while (longest > 1) {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t half = sl[i] >> 1;
        if (half > 0) {
          const bool up = l_spl[sb[i] + half] <= o[i];
          sb[i] += up ? half : 0;
          sl[i] = up ? sl[i] - half : half;
        }
      }
      longest -= longest >> 1;
    }
    longest = 0;
#pragma unroll
    for (int i = 0; i < W; ++i) {
      if (sl[i] > 0) {
        base[i] = s0 + sb[i] * step;
        const uint32_t rest = lo[i] + seg[i] - base[i];
        len[i] = rest < step ? rest : step;
      }
      longest = len[i] > longest ? len[i] : longest;
    }
    while (longest > 1) {
#pragma unroll
      for (int i = 0; i < W; ++i) {
        const uint32_t half = len[i] >> 1;
        if (half > 0) {
          const bool up = key_lo(skeys, (int64_t)base[i] + half) <= o[i];
          base[i] += up ? half : 0;
          len[i] = up ? len[i] - half : half;
        }
      }
      longest -= longest >> 1;
    }
#pragma unroll
    for (int i = 0; i < W; ++i) {
      if (len[i] == 0) continue;
      if (lds) {
        const uint32_t j = base[i] - s0;
        atomicAdd(&l_cnt[j >> 1], 1u << ((j & 1u) * 16));
      } else {
        uint32_t h = (base[i] * 2654435761u) >> 18;      // kColSlots / 4 == 2^14 entries
        bool placed = false;
#pragma unroll 1
        for (int p = 0; p < 4 && !placed; ++p) {
          const uint32_t prev = atomicCAS(&t_key[h], 0xffffffffu, base[i]);
          if (prev == 0xffffffffu || prev == base[i]) {
            atomicAdd(&t_cnt[h], 1u);
            placed = true;
          }
          h = (h + 1) & (kColSlots / 4 - 1);
        }
        if (!placed) atomicAdd(cnt + base[i], 1u);
      }
    }
  }
  __syncthreads();
  if (lds) {
    for (uint32_t j = threadIdx.x; j < L; j += kColThreads) {
      const uint32_t add = (l_cnt[j >> 1] >> ((j & 1u) * 16)) & 0xffffu;
      if (add) atomicAdd(cnt + s0 + j, add);
    }
  } else {
    for (uint32_t j = threadIdx.x; j < (uint32_t)kColSlots / 4; j += kColThreads)
      if (t_key[j] != 0xffffffffu) atomicAdd(cnt + t_key[j], t_cnt[j]);
  }
}

// stage 4b: pfx = inclusive scan of the counters over all slots (mod 2^32).  Positive k of class cls, a = the first slot of its tie
// group: TP = end(cls) - a, Rank = pfx[end - 1] - pfx[a - 1]
__global__ __launch_bounds__(256) void k_ap_terms(const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ off, int c,
                                                  const uint32_t *__restrict__ pfx, double *__restrict__ terms) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (int64_t)off[c]) return;
  const uint64_t key = skeys[k];
  const int cls = (int)(key >> 32);
  int64_t lo = off[cls], hi = k;              // the first slot in [off[cls], k] that holds `key`
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (skeys[mid] < key) lo = mid + 1; else hi = mid;
  }
  const uint32_t end = off[cls + 1];
  const uint32_t rank = pfx[end - 1] - (lo > 0 ? pfx[lo - 1] : 0u);
  terms[k] = (double)(end - (uint32_t)lo) / (double)rank;
}

// stage 4c: one workgroup per class: thread t adds the terms t, t + 256, ... of the segment, then a tree over the 256 partial sums
__global__ __launch_bounds__(256) void k_ap_finish(const double *__restrict__ terms, const uint32_t *__restrict__ off, double *__restrict__ ap) {
  __shared__ double l_sum[256];
  const int cls = blockIdx.x;
  const int64_t lo = off[cls], hi = off[cls + 1];
  double acc = 0.0;
  int64_t k = lo + threadIdx.x;
  for (; k + 768 < hi; k += 1024) {
    const double t0 = terms[k], t1 = terms[k + 256], t2 = terms[k + 512], t3 = terms[k + 768];
    acc += t0; acc += t1; acc += t2; acc += t3;
  }
  for (; k < hi; k += 256) acc += terms[k];
  l_sum[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) l_sum[threadIdx.x] += l_sum[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) ap[cls] = hi > lo ? l_sum[0] / (double)(hi - lo) : __longlong_as_double(0x7ff8000000000000ll);
}

__global__ void k_ap_nan(double *__restrict__ ap, int c) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < c) ap[t] = __longlong_as_double(0x7ff8000000000000ll);
}

int class_bits(int c) {      // the all-ones key must sort behind class c - 1: 2^bits - 1 >= c
  int b = 1;
  while ((1 << b) - 1 < c) ++b;
  return b;
}

// temporary bytes of the two rocprim calls (size queries: no launch)
int rocprim_bytes(int64_t n, int c, hipStream_t s, size_t *sort_b, size_t *scan_b) {
  const size_t m = (size_t)(n > 0 ? n : 1);
  LGS_HIP(rocprim::radix_sort_keys(nullptr, *sort_b, (uint64_t *)nullptr, (uint64_t *)nullptr, m, 0u, (unsigned)(32 + class_bits(c)), s));
  LGS_HIP(rocprim::inclusive_scan(nullptr, *scan_b, (uint32_t *)nullptr, (uint32_t *)nullptr, m, rocprim::plus<uint32_t>(), s));
  return 0;
}

}  // namespace

}  // namespace lgs

using namespace lgs;

extern "C" int64_t lgs_ap_workspace_bytes(int64_t n, int c) {
  if (n < 0 || c < 1 || c > kMaxClasses) return -1;
  size_t sort_b = 0, scan_b = 0;
  if (rocprim_bytes(n, c, (hipStream_t)0, &sort_b, &scan_b)) return -1;
  return ap_layout(n, c, (int64_t)std::max(sort_b, scan_b)).total;
}

extern "C" int lgs_average_precision(const void *scores, int64_t n, int c, const int64_t *labels, int64_t ignore_index, int from_logits,
                                     double *ap_out, int dtype, void *workspace, void *stream) {
  LGS_REQUIRE(ap_out && n >= 0 && ((scores && labels && workspace) || n == 0), "lgs_average_precision: null argument");
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, "lgs_average_precision: unknown dtype");
  LGS_REQUIRE(n < (1ll << 31) - 1, "lgs_average_precision: more rows than a 32-bit slot index holds");
  int q;
  if (int rc = class_shape(c, dtype, "lgs_average_precision", &q)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    LGS_KLAUNCH(k_ap_nan, (unsigned)((c + 255) / 256), 256, 0, s, ap_out, c);
    LGS_HIP(hipGetLastError());
    return 0;
  }
  size_t sort_b = 0, scan_b = 0;
  if (int rc = rocprim_bytes(n, c, s, &sort_b, &scan_b)) return rc;
  const ApWs w = ap_layout(n, c, (int64_t)std::max(sort_b, scan_b));
  void *tmp = Layout::at<char>(workspace, w.tmp);
  uint64_t *keys = Layout::at<uint64_t>(workspace, w.keys), *skeys = Layout::at<uint64_t>(workspace, w.skeys);
  double *terms = Layout::at<double>(workspace, w.terms);
  float2 *rowstat = Layout::at<float2>(workspace, w.rowstat);
  uint32_t *cnt = Layout::at<uint32_t>(workspace, w.cnt), *pfx = Layout::at<uint32_t>(workspace, w.pfx);
  uint32_t *off = Layout::at<uint32_t>(workspace, w.off), *mn = Layout::at<uint32_t>(workspace, w.mn);
  const unsigned row_blocks = (unsigned)((n + 255) / 256);
  LGS_HIP(hipMemsetAsync(cnt, 0, sizeof(uint32_t) * n, s));
  // 1. keys
  if (from_logits) {
    const int rc = with_class_rows<1>(dtype, q, 0, "lgs_average_precision", [&](auto e, auto) {
      using E = decltype(e);
      LGS_KLAUNCH((k_ap_softmax_keys<typename E::T, E::Q, E::R>), (unsigned)std::min<int64_t>(e.tiles(n), kRankBlocks), 256, 0, s,
                  e.in(scores), n, c, labels, ignore_index, keys, rowstat);
      return 0;
    });
    if (rc) return rc;
  } else if (dtype == LGS_BF16) {
    LGS_KLAUNCH(k_ap_keys<bf16_t>, row_blocks, 256, 0, s, reinterpret_cast<const bf16_t *>(scores), n, c, labels, ignore_index, keys);
  } else {
    LGS_KLAUNCH(k_ap_keys<float>, row_blocks, 256, 0, s, reinterpret_cast<const float *>(scores), n, c, labels, ignore_index, keys);
  }
  // 2. sort, segment starts
  LGS_HIP(rocprim::radix_sort_keys(tmp, sort_b, keys, skeys, (size_t)n, 0u, (unsigned)(32 + class_bits(c)), s));
  LGS_KLAUNCH(k_ap_offsets, (unsigned)((c + 1 + 255) / 256), 256, 0, s, skeys, n, c, off, mn);
  // 3. rank pass: small inputs row by row, big ones column chunk by column chunk in slabs of rows that give ~1024 workgroups
  const int rc = with_class_rows<2>(dtype, q, from_logits ? 1 : 0, "lgs_average_precision", [&](auto e, auto logits) {
    using E = decltype(e);
    constexpr bool kLogits = decltype(logits)::value != 0;
    if (n * c < kColMinElems) {
      LGS_KLAUNCH((k_ap_rank<typename E::T, E::Q, E::R, kLogits>), (unsigned)std::min<int64_t>(e.tiles(n), kRankBlocks), 256, 0, s,
                  e.in(scores), n, c, rowstat, skeys, off, mn, cnt);
    } else {
      const int64_t chunks = (c + epl(dtype) - 1) / epl(dtype), want = std::max<int64_t>(1024 / chunks, 1);
      const int64_t slab = std::min<int64_t>(kColRows, ((n + want - 1) / want + kColThreads - 1) / kColThreads * kColThreads);
      LGS_KLAUNCH((k_ap_rank_cols<typename E::T, kLogits>), dim3((unsigned)chunks, (unsigned)((n + slab - 1) / slab)), kColThreads, 0, s,
                  e.in(scores), n, c, slab, rowstat, skeys, off, mn, cnt);
    }
    return 0;
  });
  if (rc) return rc;
  // 4. finish
  LGS_HIP(rocprim::inclusive_scan(tmp, scan_b, cnt, pfx, (size_t)n, rocprim::plus<uint32_t>(), s));
  LGS_KLAUNCH(k_ap_terms, row_blocks, 256, 0, s, skeys, off, c, pfx, terms);
  LGS_KLAUNCH(k_ap_finish, (unsigned)c, 256, 0, s, terms, off, ap_out);
  LGS_HIP(hipGetLastError());
  return 0;
}
