// lgs_mapsort.h -- window mask sort and row permutation of a 27-slot table: kernels and their constants.  Included by lgs_manager.hip only.
#pragma once
#include "lgs_common.h"

namespace lgs {

// Rows whose neighbourhoods have the same shape are clustered: inside windows of kMaskWindow Morton-consecutive
// positions (spatially compact -> the gathered rows stay L2-resident) the positions are re-ordered by their
// 27-bit presence mask, so a 32-row MFMA block meets far fewer distinct (block, offset) combinations
// (measured on the synthetic rooms: zero-padded MFMA work 1.83x -> 1.31x of the real pairs).
constexpr int kMaskWindow = 16384;
// Sort key of a neighbourhood mask inside its window (tuning knob MASK_ORDER; the row order is free, only speed depends on it):
//   0  the mask itself (offset 26 most significant);
//   1  offsets by CLASS, corners most significant, then edges, faces, centre -- the rare offsets split the window first, so a
//      tile's rows agree on them and fewer (32-row block, offset) pairs are gathered for nothing;
//   2  the reverse (faces most significant);  3  popcount-major, then the mask.
__device__ inline uint32_t mask_sort_code(uint32_t m, int order) {
  if (order == 0) return m;
  if (order == 3) return ((uint32_t)__popc(m) << 27) | m;
  // offset k = (dx+1) + 3 (dy+1) + 9 (dz+1): class = number of non-zero components
  uint32_t corner = 0, edge = 0, face = 0, centre = (m >> 13) & 1u;
  int nc = 0, ne = 0, nf = 0;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
    const int cls = (dx != 0) + (dy != 0) + (dz != 0);
    const uint32_t b = (m >> k) & 1u;
    if (cls == 3) corner |= b << nc++;
    else if (cls == 2) edge |= b << ne++;
    else if (cls == 1) face |= b << nf++;
  }
  if (order == 1) return (corner << 19) | (edge << 7) | (face << 1) | centre;
  return (face << 21) | (edge << 9) | (corner << 1) | centre;
}
__global__ void k_mask_sort_keys(const uint32_t *pmask, int64_t n, int64_t n_pad, int window, int order, uint64_t *keys, int32_t *vals) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pad) return;
  keys[p] = p < n ? (((uint64_t)(p / window)) << 32) | mask_sort_code(pmask[p], order) : ~0ull;
  vals[p] = (int32_t)p;
}
// key bits the window sort has to look at: 32 bits of mask code + the window index.  A padding key is all ones; its low
// bits beat every real key as long as the largest real window index is not all ones too -- one more bit than it needs.
inline unsigned mask_sort_bits(int64_t n_pad, int window) {
  const uint64_t nw = (uint64_t)((n_pad + window - 1) / window);
  unsigned wb = 1;
  while ((1ull << wb) - 1 < nw) ++wb;
  return 32u + wb > 64u ? 64u : 32u + wb;
}
// MAP_WINDOW_SORT: the same permutation without the global sort.  The window index is the high part of the radix key and p is
// already ascending, so the result is an independent stable sort of every window by its 32-bit code -- and sorting the composite
// (code, index in window), padding rows under the code 0xffffffff that no real code reaches (order 3 tops out at 0xdfffffff), by
// ANY correct sort gives that stable order, because composites are unique.  One workgroup per window: 16 composites per thread,
// a bitonic network whose stages are taken four at a time in registers (the 16 elements of a thread differ in four index bits
// [B, B + 4), so the compare-exchanges at distances 2^(B+3) .. 2^B need no other thread); between such passes the window goes
// through LDS once, and every thread writes back exactly the slots it read, so one workgroup barrier per pass suffices.  The
// first four merge sizes and the last pass have B = 0: the codes come from global memory and the permutation goes to it straight
// from registers.  29 passes for 16 384 positions.  Only workgroup barriers, no hand-off between workgroups.
// One CU's vector ALU is the bound (a window is one workgroup), so the network is kept cheap per comparator: the 46-bit composite
// sits in the mantissa of a double in [1, 2), where the order of the numbers is the order of the bit patterns, and a
// compare-exchange is v_min_f64 + v_max_f64 (both return an operand unchanged); the direction of a merge is the same for all 16
// elements of a thread once the merge is wider than a thread's span, so a descending thread complements the mantissas on the way
// in and out instead of steering every comparator; B is a template parameter, so the LDS offsets are immediates.
constexpr int kWsMinLog2 = 10, kWsMaxLog2 = 14;
inline int window_sort_log2(int64_t window) {   // -> log2(window) where k_window_sort serves it, else -1 (the radix sort does)
  for (int l = kWsMinLog2; l <= kWsMaxLog2; ++l)
    if (window == (1ll << l)) return l;
  return -1;
}
inline size_t window_sort_lds(int log2w) { return (((size_t)1 << log2w) + ((size_t)1 << (log2w - 4))) * sizeof(double); }
static_assert((((size_t)1 << kWsMaxLog2) + ((size_t)1 << (kWsMaxLog2 - 4))) * 8 <= 160 * 1024, "k_window_sort: LDS budget of one CU");
constexpr unsigned long long kWsOne = 0x3ff0000000000000ull, kWsMant = 0x000fffffffffffffull;
// (the instructions by name: fmin / fmax would first quiet a possible signalling NaN of each operand, two more v_max_f64 per comparator)
__device__ inline double ws_min(double x, double y) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; }
__device__ inline double ws_max(double x, double y) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y)); return r; }
__device__ inline void ws_cmpx(double &lo, double &hi) {
  double a;
  asm("v_min_f64 %0, %1, %2\n\tv_max_f64 %1, %1, %2" : "=&v"(a), "+v"(hi) : "v"(lo));
  lo = a;
}
// LDS slot of index i: i + i / 16 (one pad slot per 16: the B = 0 passes walk 16-element rows).  For a thread's elements
// base | r << B the two terms split without a carry, so the slot is slot(base) + a compile-time offset
template <int B>
__device__ inline int ws_base(int t) { return ((t >> B) << (B + 4)) | (t & ((1 << B) - 1)); }
template <int B>
__device__ inline void ws_store(double *lds, const double (&e)[16], int t) {
  const int base = ws_base<B>(t);
  double *q = lds + base + (base >> 4);
#pragma unroll
  for (int r = 0; r < 16; ++r) q[(r << B) + ((r << B) >> 4)] = e[r];
}
// one pass: load the 16 elements at index bits [B, B + 4), the stages at distances 2^hi .. 2^B of the merge to runs of 2^m (m >= B + 4:
// ascending where the thread's base has bit m clear), store unless it is the last pass of the sort
template <int B>
__device__ inline void ws_pass(double *lds, double (&e)[16], int t, int hi, int m, bool store) {
  const int base = ws_base<B>(t);
  const double *q = lds + base + (base >> 4);
  const unsigned long long flip = ((base >> m) & 1) ? kWsMant : 0ull;
#pragma unroll
  for (int r = 0; r < 16; ++r) e[r] = __longlong_as_double((long long)((unsigned long long)__double_as_longlong(q[(r << B) + ((r << B) >> 4)]) ^ flip));
#pragma unroll
  for (int s = 3; s >= 0; --s) {
    if (B + s > hi) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (!(r & (1 << s))) ws_cmpx(e[r], e[r | (1 << s)]);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) e[r] = __longlong_as_double((long long)((unsigned long long)__double_as_longlong(e[r]) ^ flip));
  if (store) ws_store<B>(lds, e, t);
}
__global__ __launch_bounds__(1024) void k_window_sort(const uint32_t *__restrict__ pmask, int64_t n, int64_t n_pad, int log2w, int order,
                                                      int32_t *__restrict__ perm) {
  extern __shared__ double ws_lds[];     // [window + window / 16]
  const int t = threadIdx.x;             // blockDim = window / 16
  const int64_t w0 = (int64_t)blockIdx.x << log2w;
  double e[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t p = w0 + 16 * t + r;
    const uint32_t code = p < n ? mask_sort_code(pmask[p], order) : 0xffffffffu;
    e[r] = __longlong_as_double((long long)(kWsOne | ((unsigned long long)code << 14) | (unsigned)(16 * t + r)));
  }
  // merges to runs of 2, 4, 8, 16 inside the thread: the direction bit m is a bit of r (or, for m = 4, of t)
#pragma unroll
  for (int m = 1; m <= 4; ++m) {
#pragma unroll
    for (int s = m - 1; s >= 0; --s) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (r & (1 << s)) continue;
        const bool up = (((16 * t) | r) & (1 << m)) == 0;
        const double a = ws_min(e[r], e[r | (1 << s)]), b = ws_max(e[r], e[r | (1 << s)]);
        e[r] = up ? a : b; e[r | (1 << s)] = up ? b : a;
      }
    }
  }
  ws_store<0>(ws_lds, e, t);
  __syncthreads();
  for (int m = 5; m <= log2w; ++m) {
    for (int hi = m - 1; hi >= 0;) {
      const int b = hi >= 3 ? hi - 3 : 0;
      const bool store = !(m == log2w && b == 0);
      switch (b) {
        case 0: ws_pass<0>(ws_lds, e, t, hi, m, store); break;
        case 1: ws_pass<1>(ws_lds, e, t, hi, m, store); break;
        case 2: ws_pass<2>(ws_lds, e, t, hi, m, store); break;
        case 3: ws_pass<3>(ws_lds, e, t, hi, m, store); break;
        case 4: ws_pass<4>(ws_lds, e, t, hi, m, store); break;
        case 5: ws_pass<5>(ws_lds, e, t, hi, m, store); break;
        case 6: ws_pass<6>(ws_lds, e, t, hi, m, store); break;
        case 7: ws_pass<7>(ws_lds, e, t, hi, m, store); break;
        case 8: ws_pass<8>(ws_lds, e, t, hi, m, store); break;
        case 9: ws_pass<9>(ws_lds, e, t, hi, m, store); break;
        default: ws_pass<10>(ws_lds, e, t, hi, m, store); break;
      }
      __syncthreads();
      hi = b - 1;
    }
  }
  // the last pass had B = 0: the thread holds sorted slots 16 t .. 16 t + 15 of its window (n_pad is a multiple of 256: all of them or none)
  if (w0 + 16 * t >= n_pad) return;
  int4 *dst = reinterpret_cast<int4 *>(perm + w0 + 16 * t);
  int32_t v[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = (int32_t)(w0 + (int64_t)(__double_as_longlong(e[r]) & 0x3fff));
#pragma unroll
  for (int r = 0; r < 16; r += 4) dst[r >> 2] = make_int4(v[r], v[r + 1], v[r + 2], v[r + 3]);
}
__global__ void k_permute_map3(const int32_t *nbr_tmp, const uint32_t *pmask, const int32_t *perm, const int32_t *order,
                               int64_t n, int64_t n_pad, int32_t *nbr, int32_t *out_row, uint32_t *mask64) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // grid covers n_pad exactly
  int32_t src = q < n ? perm[q] : -1;
  uint32_t pm = src >= 0 ? pmask[src] : 0u;
  out_row[q] = src >= 0 ? (order ? order[src] : src) : -1;
  uint32_t m = 0;
  for (int k = 0; k < 27; ++k) {
    nbr[(int64_t)k * n_pad + q] = src >= 0 ? nbr_tmp[(int64_t)k * n_pad + src] : -1;
    if (__ballot((pm >> k) & 1u)) m |= 1u << k;
  }
  if ((threadIdx.x & 63) == 0) mask64[q >> 6] = m;
}
// MAP_PERMUTE_LDS: the same tables with the gathers taken from LDS.  perm[q] stays inside q's window (the sort is per window), so the
// rows a window gathers from nbr_tmp[k] are ONE contiguous segment of at most 4 x window bytes: workgroup (w, g) keeps the window's
// slice of perm in registers (as indices into the segment), and for each of its offsets k in [g kg, g kg + kg) stages the segment
// with 16-byte loads -- the next offset's loads are issued into registers before the current one is gathered -- reads LDS at the
// permuted index and writes nbr[k] coalesced.  Group 0 also stages pmask and `order` the same way for mask64 and out_row.
// A thread owns quads of four consecutive positions, so perm, the staged rows and the tables all move as 16-byte accesses and only
// the LDS reads are single words.  window is a multiple of 256 (so is n_pad): a group of 64 positions lies in one window.
constexpr int kPlThreads = 1024, kPlMaxWindow = 32768;
__device__ __forceinline__ int pl_clamp(int l, int len) { return l < 0 ? 0 : (l >= len ? len - 1 : l); }
typedef int pl_v4 __attribute__((ext_vector_type(4)));   // a plain 16-byte vector: arrays of it stay in registers
template <int Q>   // the nq 16-byte pieces of a window's segment of one row: global memory -> registers -> LDS
__device__ __forceinline__ void pl_load(pl_v4 (&pre)[Q], const int32_t *seg, int nq, int t) {
  const pl_v4 *src = reinterpret_cast<const pl_v4 *>(seg);
#pragma unroll
  for (int j = 0; j < Q; ++j) pre[j] = src[j * kPlThreads + t < nq ? j * kPlThreads + t : t & 63];   // unconditional: nq >= 64
}
template <int Q>
__device__ __forceinline__ void pl_store(const pl_v4 (&pre)[Q], int32_t *lds, int nq, int t) {
  pl_v4 *lds4 = reinterpret_cast<pl_v4 *>(lds);
#pragma unroll
  for (int j = 0; j < Q; ++j)
    if (j * kPlThreads + t < nq) lds4[j * kPlThreads + t] = pre[j];
}
__device__ __forceinline__ int4 pl_gather(const int32_t *lds, int4 l, int none) {
  return make_int4(l.x >= 0 ? lds[l.x] : none, l.y >= 0 ? lds[l.y] : none, l.z >= 0 ? lds[l.z] : none, l.w >= 0 ? lds[l.w] : none);
}
template <int IPT>   // positions per thread: window <= IPT * kPlThreads
__global__ __launch_bounds__(kPlThreads) void k_permute_map3_lds(const int32_t *__restrict__ nbr_tmp, const uint32_t *__restrict__ pmask,
                                                                 const int32_t *__restrict__ perm, const int32_t *__restrict__ order, int64_t n,
                                                                 int64_t n_pad, int window, int kg, int32_t *__restrict__ nbr,
                                                                 int32_t *__restrict__ out_row, uint32_t *__restrict__ mask64) {
  extern __shared__ int32_t pl_lds[];    // [min(window, n_pad)]
  constexpr int Q = IPT / 4;             // a thread owns Q quads of four consecutive positions: quad j * kPlThreads + t of the window
  const int t = threadIdx.x;
  const int64_t w0 = (int64_t)blockIdx.x * window;
  const int len = (int)(n_pad - w0 < (int64_t)window ? n_pad - w0 : (int64_t)window);   // positions of this window: a multiple of 256
  const int nq = len >> 2;
  const int live = (int)(n - w0 < (int64_t)len ? n - w0 : (int64_t)len);                // ... of which the first `live` are rows
  int4 loc[Q];                           // perm[q] - w0, or -1 for a padding position
  {
    const int4 *src = reinterpret_cast<const int4 *>(perm + w0);   // perm has n_pad entries
    const int w0i = (int)w0;
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int qd = j * kPlThreads + t;
      int4 l = make_int4(-1, -1, -1, -1);
      if (qd < nq) {
        const int4 p = src[qd];
        // a correct permutation is inside the window; nothing else may index the LDS
        l.x = 4 * qd + 0 < live ? pl_clamp(p.x - w0i, len) : -1;
        l.y = 4 * qd + 1 < live ? pl_clamp(p.y - w0i, len) : -1;
        l.z = 4 * qd + 2 < live ? pl_clamp(p.z - w0i, len) : -1;
        l.w = 4 * qd + 3 < live ? pl_clamp(p.w - w0i, len) : -1;
      }
      loc[j] = l;
    }
  }
  pl_v4 pre[Q];
  const int k0 = blockIdx.y * kg, k1 = k0 + kg < 27 ? k0 + kg : 27;
  if (blockIdx.y == 0) {
    pl_load<Q>(pre, reinterpret_cast<const int32_t *>(pmask) + w0, nq, t);   // pmask has n_pad entries
    pl_store<Q>(pre, pl_lds, nq, t);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int qd = j * kPlThreads + t;   // 64 consecutive quads per wave, nq a multiple of 64: a wave is inside or outside as a whole
      const int4 pm = pl_gather(pl_lds, loc[j], 0);
      uint32_t m = (uint32_t)(pm.x | pm.y | pm.z | pm.w);   // an offset is in the group's mask if any of its 64 positions has it: 16 lanes
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) m |= (uint32_t)__shfl_xor((int)m, o, 64);
      if (qd < nq && (t & 15) == 0) mask64[(w0 + 4 * qd) >> 6] = m;
    }
    __syncthreads();
    if (order) {                           // `order` has n entries, not n_pad
#pragma unroll
      for (int j = 0; j < Q; ++j) {
        const int qd = j * kPlThreads + t;
        if (qd >= nq) continue;
        int4 v = make_int4(-1, -1, -1, -1);
        if (4 * qd + 3 < live) v = reinterpret_cast<const int4 *>(order + w0)[qd];
        else if (4 * qd < live) {
          v.x = order[w0 + 4 * qd];
          if (4 * qd + 1 < live) v.y = order[w0 + 4 * qd + 1];
          if (4 * qd + 2 < live) v.z = order[w0 + 4 * qd + 2];
        }
        reinterpret_cast<int4 *>(pl_lds)[qd] = v;
      }
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int qd = j * kPlThreads + t;
      if (qd >= nq) continue;
      const int4 l = loc[j];
      const int w0i = (int)w0;
      const int4 v = order ? pl_gather(pl_lds, l, -1)
                           : make_int4(l.x >= 0 ? w0i + l.x : -1, l.y >= 0 ? w0i + l.y : -1, l.z >= 0 ? w0i + l.z : -1, l.w >= 0 ? w0i + l.w : -1);
      reinterpret_cast<int4 *>(out_row + w0)[qd] = v;
    }
    __syncthreads();
  }
  pl_load<Q>(pre, nbr_tmp + (int64_t)k0 * n_pad + w0, nq, t);
  for (int k = k0; k < k1; ++k) {
    pl_store<Q>(pre, pl_lds, nq, t);
    __syncthreads();
    if (k + 1 < k1) pl_load<Q>(pre, nbr_tmp + (int64_t)(k + 1) * n_pad + w0, nq, t);
    int4 *dst = reinterpret_cast<int4 *>(nbr + (int64_t)k * n_pad + w0);
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const int qd = j * kPlThreads + t;
      if (qd < nq) dst[qd] = pl_gather(pl_lds, loc[j], -1);
    }
    __syncthreads();
  }
}

}  // namespace lgs
