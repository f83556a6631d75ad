// lgs_manager.hip -- coordinate manager + kernel-map construction for gfx950.
//
// Replaces (functionally) MinkowskiEngine's CoordinateManager as used by the reference:
//   SparseTensor(feats, coords)            /root/reference/lib/train_test/pl_BaselineTrainer.py:300
//   stride-2 output maps                    /root/reference/models/res16unet.py:49-107
//   kernel maps for k in {1,2,3}            /root/reference/models/modules/common.py:179-236
//
// Design: every coordinate is packed into ONE 64-bit Morton key
//   key = batch << 54 | interleave3(x + 2^17, y + 2^17, z + 2^17)
// Level-0 rows keep the caller's order (logits stay row-aligned with the input), but every map also
// carries its rows in Morton order (`order`: sorted position -> row).  Consequences:
//   * coarsening by 2 is a bit-mask on the key and preserves the sort, so a strided map and its
//     2x2x2 kernel map come from one flag+scan over the sorted keys -- no hashing;
//   * 3x3x3 maps come from 27 probes per voxel into a directory of the occupied 4x4x4 blocks of the sorted keys (DirRef; the
//     per-voxel open-addressing hash, HashRef, stays behind the knob MAP_BLOCK_DIR = 0);
//   * conv tiles are runs of 64 Morton-consecutive voxels, so a wavefront ballot gives the per-tile
//     bitmask of kernel offsets that have any neighbour at all (planar surfaces miss most
//     out-of-plane offsets), which the conv kernels use to skip work.
#include "lgs_common.h"

#include <cstring>
#include <initializer_list>
#include <memory>
#include <tuple>
#include <rocprim/rocprim.hpp>

namespace lgs {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

constexpr int kBias = 1 << (kCoordBits - 1);  // 131072
constexpr uint64_t kEmpty = ~0ull;

__host__ __device__ inline uint64_t spread3(uint64_t x) {
  x &= 0x1fffff;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
__host__ __device__ inline uint32_t compact3(uint64_t x) {
  x &= 0x1249249249249249ull;
  x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ull;
  x = (x ^ (x >> 4)) & 0x100f00f00f00f00full;
  x = (x ^ (x >> 8)) & 0x1f0000ff0000ffull;
  x = (x ^ (x >> 16)) & 0x1f00000000ffffull;
  x = (x ^ (x >> 32)) & 0x1fffff;
  return (uint32_t)x;
}
__device__ inline uint64_t pack_key(int b, int xb, int yb, int zb) {  // biased coords
  return ((uint64_t)b << 54) | spread3((uint64_t)xb) | (spread3((uint64_t)yb) << 1) | (spread3((uint64_t)zb) << 2);
}
__device__ inline void unpack_key(uint64_t key, int &b, int &xb, int &yb, int &zb) {
  b = (int)(key >> 54);
  uint64_t m = key & ((1ull << 54) - 1);
  xb = (int)compact3(m);
  yb = (int)compact3(m >> 1);
  zb = (int)compact3(m >> 2);
}
__device__ inline uint64_t hash64(uint64_t k) {
  k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
  return k;
}

// ------------------------------------------------------------------------------------------- kernels
__global__ void k_pack_keys(const int32_t *coords, int64_t n, uint64_t *keys, int32_t *vals, int *err) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int4 c = reinterpret_cast<const int4 *>(coords)[i];
  bool ok = c.x >= 0 && c.x < 1024 && c.y > -kBias && c.y < kBias - 64 && c.z > -kBias && c.z < kBias - 64 &&
            c.w > -kBias && c.w < kBias - 64;
  if (!ok) { atomicOr(err, 1); c = make_int4(0, 0, 0, 0); }
  keys[i] = pack_key(c.x, c.y + kBias, c.z + kBias, c.w + kBias);
  vals[i] = (int32_t)i;
}

// head[p] = 1 if sorted key p starts a new run of (key & keep_mask)
__global__ void k_heads(const uint64_t *skeys, int64_t n, uint64_t keep_mask, int32_t *head) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint64_t k = skeys[p] & keep_mask;
  head[p] = (p == 0 || (skeys[p - 1] & keep_mask) != k) ? 1 : 0;
}

// insert step: flag (by input index) the first occurrence of every distinct coordinate
__global__ void k_mark_first(const int32_t *svals, const int32_t *head, int64_t n, int32_t *is_first) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  is_first[svals[p]] = head[p];
}
// urow = exclusive scan of is_first over input order; write coords/unique_index of surviving rows,
// and the sorted-order arrays of the deduplicated map
__global__ void k_emit_unique(const int32_t *coords, const int32_t *is_first, const int32_t *urow, int64_t n,
                              int32_t *ucoords, int64_t *unique_index) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !is_first[i]) return;
  int32_t u = urow[i];
  reinterpret_cast<int4 *>(ucoords)[u] = reinterpret_cast<const int4 *>(coords)[i];
  if (unique_index) unique_index[u] = i;
}
__global__ void k_emit_sorted(const uint64_t *skeys, const int32_t *svals, const int32_t *head,
                              const int32_t *runid_incl, const int32_t *urow, int64_t n, uint64_t *ukeys,
                              int32_t *order) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n || !head[p]) return;
  int32_t q = runid_incl[p] - 1;
  ukeys[q] = skeys[p];
  order[q] = urow[svals[p]];
}
__global__ void k_emit_inverse(const int32_t *svals, const int32_t *runid_incl, const int32_t *order, int64_t n,
                               int64_t *inverse) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  inverse[svals[p]] = order[runid_incl[p] - 1];
}

// stride-2: coarse rows are created in Morton order (row == sorted position)
// nc = the row count the coarse arrays were SIZED for (counted at insert time, no synchronisation): a run index beyond it is
// never written, and the last thread compares the two counts (d_err bit 1, lgs_manager_check)
__global__ void k_emit_coarse(const uint64_t *fkeys, const int32_t *head, const int32_t *cidx_incl, int64_t n,
                              uint64_t keep_mask, uint64_t *ckeys, int32_t *ccoords, int32_t *cstart,
                              int32_t *fine_cidx, int64_t nc, int *d_err) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  int32_t q = cidx_incl[p] - 1;
  fine_cidx[p] = q;
  if (p == n - 1 && (int64_t)q + 1 != nc && d_err) atomicOr(d_err, 2);
  if (q >= nc) return;
  if (head[p]) {
    uint64_t k = fkeys[p] & keep_mask;
    ckeys[q] = k;
    cstart[q] = (int32_t)p;
    int b, x, y, z;
    unpack_key(k, b, x, y, z);
    reinterpret_cast<int4 *>(ccoords)[q] = make_int4(b, x - kBias, y - kBias, z - kBias);
  }
  if (p == n - 1) cstart[q + 1] = (int32_t)n;
}

__global__ void k_hash_fill(uint64_t *hkeys, int64_t cap) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) hkeys[i] = kEmpty;
}
__global__ void k_hash_insert(const uint64_t *skeys, const int32_t *order, int64_t n, uint64_t *hkeys,
                              int32_t *hvals, uint64_t capm1) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint64_t key = skeys[p];
  uint64_t s = hash64(key) & capm1;
  for (;;) {
    unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(hkeys + s), (unsigned long long)kEmpty,
                                        (unsigned long long)key);
    if (prev == kEmpty) { hvals[s] = order ? order[p] : (int32_t)p; return; }
    s = (s + 1) & capm1;  // keys are unique here, no equality case
  }
}

// Row counts of ALL coarser levels from the sorted stride-1 keys: coarsening by 2^L drops the 3 L low Morton bits and keeps the
// order, so the level-L map has one row per run of equal masked keys.  Counting the run heads of every level in the pass that
// already exists for the insert lets lgs_manager_insert return them with ITS host synchronisation: the four
// lgs_manager_stride2 calls of the U-Net then need none (5 host syncs per training step -> 1; duplicates of the input do not
// matter: equal keys stay equal under any mask).
constexpr int kPreLevels = 8;
constexpr int kCountPerThread = 16;
constexpr int kBatchShift = 54;   // key bits above it: the batch index
// counts[kPreLevels] (one slot more): the distinct batch indices, i.e. the rows of the origin map (lgs_manager_origin) --
// the same at every level of one insert
__global__ __launch_bounds__(256) void k_count_levels(const uint64_t *__restrict__ skeys, int64_t n, int32_t *__restrict__ counts) {
  // a workgroup walks 256 x kCountPerThread consecutive keys and adds ONE number per level to the global counters (one
  // atomic per wave and level on eight shared addresses cost 0.67 ms at 1.2 M keys: the atomics serialise at the L2)
  __shared__ int32_t l_cnt[kPreLevels + 1];
  if (threadIdx.x <= kPreLevels) l_cnt[threadIdx.x] = 0;
  __syncthreads();
  int32_t c[kPreLevels + 1];
#pragma unroll
  for (int L = 0; L <= kPreLevels; ++L) c[L] = 0;
  const int64_t base = (int64_t)blockIdx.x * 256 * kCountPerThread;
#pragma unroll 4
  for (int i = 0; i < kCountPerThread; ++i) {
    const int64_t p = base + (int64_t)i * 256 + threadIdx.x;
    if (p >= n) break;
    const uint64_t k = skeys[p], q = p > 0 ? skeys[p - 1] : ~0ull, d = k ^ q;
#pragma unroll
    for (int L = 1; L <= kPreLevels; ++L) c[L - 1] += (p == 0 || (d >> (3 * L)) != 0) ? 1 : 0;
    c[kPreLevels] += (p == 0 || (d >> kBatchShift) != 0) ? 1 : 0;
  }
#pragma unroll
  for (int L = 0; L <= kPreLevels; ++L) {
    int32_t v = c[L];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&l_cnt[L], v);
  }
  __syncthreads();
  if (threadIdx.x <= kPreLevels && l_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], l_cnt[threadIdx.x]);
}

// ---- neighbour lookup: "which row of the probed map has this key?" for NP keys at once, all NP loads of a step in flight together
// (the probe kernels are bound by the latency of their random accesses, not by their number: profiles/r06_experiments.txt).
// HashRef (MAP_BLOCK_DIR = 0): the open-addressing table with one slot per voxel.
struct HashRef {
  const uint64_t *hkeys;
  const int32_t *hvals;
  uint64_t capm1;
  template <int NP>
  __device__ inline void find(const uint64_t (&key)[NP], bool (&ok)[NP], int32_t (&r)[NP]) const {
    uint64_t slot[NP], hk[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) slot[j] = hash64(key[j]) & capm1;
#pragma unroll
    for (int j = 0; j < NP; ++j) hk[j] = ok[j] ? hkeys[slot[j]] : kEmpty;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (ok[j]) {
        uint64_t cur = hk[j], sl = slot[j];
        while (cur != key[j] && cur != kEmpty) {
          sl = (sl + 1) & capm1;
          cur = hkeys[sl];
        }
        slot[j] = sl;
        ok[j] = cur == key[j];
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) r[j] = ok[j] ? hvals[slot[j]] : -1;
  }
};
// DirRef (MAP_BLOCK_DIR = 1): the block directory.  The rows are Morton-sorted, so the keys of one 4 x 4 x 4 block of cells (cells
// of the map's own grid: the key above bit 3 log2ts + 6) are ONE run of the sorted order, and inside the run the order is the order
// of the 6-bit cell index.  One entry per occupied block therefore answers the lookup exactly: present = the cell's occupancy bit,
// sorted position = first + popcount(occupancy below that bit), row = order[position].  The table has one entry per ~16 rows
// instead of two slots per row (level 0 of the 8-scene batch: 8 MB instead of 48 MB), and the 64 Morton-consecutive rows of a
// wave ask for a few dozen entries between them instead of 1 728 unrelated slots.
struct DirEnt { uint64_t id, occ; int32_t first, pad[3]; };   // 32 bytes: a probe reads one aligned half cache line
static_assert(sizeof(DirEnt) == 32, "DirEnt is read as two 16-byte halves");
struct DirRef {
  const DirEnt *ent;
  uint64_t capm1;
  int sh;                 // 3 log2ts of the probed map: the cell index is key bits [sh, sh + 6), the block id the bits above
  const int32_t *order;   // the probed map's sorted position -> row (nullptr: identity)
  template <int NP>
  __device__ inline void find(const uint64_t (&key)[NP], bool (&ok)[NP], int32_t (&r)[NP]) const {
    uint32_t slot[NP];     // the table has at most 2^31 entries (n < 2^31)
    ulonglong2 e[NP];      // (id, occ)
    int32_t first[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) slot[j] = (uint32_t)(hash64(key[j] >> (sh + 6)) & capm1);
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      e[j] = ok[j] ? *reinterpret_cast<const ulonglong2 *>(ent + slot[j]) : make_ulonglong2(kEmpty, 0ull);
      first[j] = ok[j] ? ent[slot[j]].first : 0;
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      if (ok[j]) {
        const uint64_t id = key[j] >> (sh + 6);
        uint32_t sl = slot[j];
        while (e[j].x != id && e[j].x != kEmpty) {
          sl = (sl + 1) & (uint32_t)capm1;
          e[j] = *reinterpret_cast<const ulonglong2 *>(ent + sl);
          first[j] = ent[sl].first;
        }
        const int cell = (int)((key[j] >> sh) & 63);
        ok[j] = e[j].x == id && ((e[j].y >> cell) & 1ull);
        first[j] += __popcll(e[j].y & ((1ull << cell) - 1ull));
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) r[j] = ok[j] ? (order ? order[first[j]] : first[j]) : -1;
  }
};
__global__ void k_dir_fill(DirEnt *dir, int64_t cap) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  ulonglong2 *q = reinterpret_cast<ulonglong2 *>(dir + i);
  q[0] = make_ulonglong2(kEmpty, 0ull);
  q[1] = make_ulonglong2(0ull, 0ull);
}
// one pass: the thread at a block head (the pattern of k_heads) walks its run of at most 64 keys, ORs the occupancy and inserts
// the entry with k_hash_insert's atomicCAS idiom (block ids are unique among the heads).  The table holds at least twice the
// block count, so the probe sequence ends; a full table (impossible by that sizing) sets d_err bit 3 instead of spinning.
__global__ void k_dir_build(const uint64_t *skeys, int64_t n, int sh, DirEnt *dir, uint64_t capm1, int *d_err) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint64_t id = skeys[p] >> (sh + 6);
  if (p > 0 && (skeys[p - 1] >> (sh + 6)) == id) return;
  uint64_t occ = 0;
  for (int64_t q = p; q < n && q < p + 64; ++q) {
    const uint64_t k = skeys[q];
    if ((k >> (sh + 6)) != id) break;
    occ |= 1ull << ((k >> sh) & 63);
  }
  uint64_t s = hash64(id) & capm1;
  for (uint64_t tries = 0; tries <= capm1; ++tries) {
    unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&dir[s].id), (unsigned long long)kEmpty, (unsigned long long)id);
    if (prev == kEmpty) { dir[s].occ = occ; dir[s].first = (int32_t)p; return; }
    s = (s + 1) & capm1;
  }
  if (d_err) atomicOr(d_err, 8);
}

// 3x3x3 stride-1 map: one thread per sorted position, 27 probes; nbr is offset-major [27][n_pad].
// Round 6: the probes of one z-plane (nine offsets) are issued TOGETHER -- nine slots computed, nine table loads in flight, then
// the (rare) continued probes, then nine value loads in flight -- instead of 27 dependent load chains one after the other (level 0
// of the 8-scene batch: 0.87 -> see profiles/r06_experiments.txt).  Same probe sequence per offset in either table: the map is
// bit-identical.
template <typename L>
__global__ __launch_bounds__(256) void k_build_map3(const uint64_t *skeys, int64_t n, int64_t n_pad, int ts, L look, int32_t *nbr, uint32_t *pmask) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // blockDim multiple of 64; p < n_pad by grid
  bool live = p < n;
  int b = 0, x = 0, y = 0, z = 0;
  if (live) unpack_key(skeys[p], b, x, y, z);
  uint32_t m = 0;
#pragma unroll 1
  for (int g = 0; g < 3; ++g) {
    uint64_t key[9];
    bool ok[9];
    const int zz = z + (g - 1) * ts;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int xx = x + (j % 3 - 1) * ts, yy = y + (j / 3 - 1) * ts;
      ok[j] = live && (((unsigned)xx | (unsigned)yy | (unsigned)zz) < (1u << kCoordBits));
      key[j] = ok[j] ? pack_key(b, xx, yy, zz) : 0ull;
    }
    int32_t r[9];
    look.template find<9>(key, ok, r);
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int k = 9 * g + j;
      nbr[(int64_t)k * n_pad + p] = r[j];
      if (r[j] >= 0) m |= 1u << k;
    }
  }
  pmask[p] = m;
}

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

// 3x3x3 stride-2, fine-stationary view (dgrad of the strided conv, forward of its transposed conv): slot k of fine position p holds
// the coarse row at c_fine - off_k * ts.  That coordinate lies on the coarse grid only where, on every axis, off_k is 0 for an even
// fine coordinate (in units of ts) and +-1 for an odd one: at most 2^3 of the 27 offsets, fixed by the row's parity class.  Only
// those are probed, all (<= 8) in flight together as in k_build_map3; the other slots are -1.  Rows of one parity class share the
// candidate set, so the window mask sort that follows groups them and a 64-row group's mask64 carries at most 8 bits.
template <typename L>
__global__ __launch_bounds__(256) void k_build_map3_fine(const uint64_t *fkeys, int64_t n, int64_t n_pad, int log2ts, L look, int32_t *nbr, uint32_t *pmask) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // blockDim multiple of 64; p < n_pad by grid
  const bool live = p < n;
  int b = 0, x = 0, y = 0, z = 0;
  if (live) unpack_key(fkeys[p], b, x, y, z);
  const int ts = 1 << log2ts;
  // the bias 2^17 is a multiple of 2 ts, so the parity of the biased coordinate is the parity of the coordinate
  const int ox = (x >> log2ts) & 1, oy = (y >> log2ts) & 1, oz = (z >> log2ts) & 1;
  uint64_t key[8];
  int kk[8];
  bool ok[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int jx = j & 1, jy = (j >> 1) & 1, jz = j >> 2;
    // an even axis has the single candidate 0 (taken at j-bit 0), an odd one -1 and +1
    const int dx = ox ? 2 * jx - 1 : 0, dy = oy ? 2 * jy - 1 : 0, dz = oz ? 2 * jz - 1 : 0;
    const int xx = x - dx * ts, yy = y - dy * ts, zz = z - dz * ts;
    ok[j] = live && (ox || !jx) && (oy || !jy) && (oz || !jz) && (((unsigned)xx | (unsigned)yy | (unsigned)zz) < (1u << kCoordBits));
    kk[j] = (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1);
    key[j] = ok[j] ? pack_key(b, xx, yy, zz) : 0ull;
  }
  int32_t r[8];
  look.template find<8>(key, ok, r);
  uint32_t m = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (ok[j]) m |= 1u << kk[j];
  for (int k = 0; k < 27; ++k) {
    int32_t v = -1;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (ok[j] && kk[j] == k) v = r[j];
    nbr[(int64_t)k * n_pad + p] = v;
  }
  pmask[p] = m;
}

// 1x1 stride-2: the fine row at the coarse row's own coordinate, if there is one.  No hashing: the fine positions of a coarse cell are
// one run of the Morton order and the cell's own coordinate has the smallest key of the run, so it can only be the run's first position.
// coarse-stationary view: nbr[q] = that fine row or -1 (padding: -1)
__global__ void k_build_map1_coarse(const uint64_t *fkeys, const int32_t *forder, const uint64_t *ckeys, const int32_t *cstart,
                                    int64_t n_c, int64_t nc_pad, int32_t *nbr) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc_pad) return;
  int32_t r = -1;
  if (q < n_c) {
    const int32_t p = cstart[q];
    if (fkeys[p] == ckeys[q]) r = forder ? forder[p] : p;
  }
  nbr[q] = r;
}
// fine-stationary view: position p writes fine row out_row[p]; nbr[p] = its coarse row where the fine coordinate lies on the coarse grid
__global__ void k_build_map1_fine(const uint64_t *fkeys, const int32_t *forder, const int32_t *fine_cidx, int64_t n, int64_t n_pad,
                                  uint64_t child_bits, int32_t *nbr, int32_t *out_row) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pad) return;
  const bool live = p < n;
  nbr[p] = (live && (fkeys[p] & child_bits) == 0) ? fine_cidx[p] : -1;
  out_row[p] = live ? (forder ? forder[p] : (int32_t)p) : -1;
}

// 2x2x2 stride-2, coarse-stationary view: nbr8[k][q] = fine row of child k of coarse row q
__global__ void k_build_map2_coarse(const uint64_t *fkeys, const int32_t *forder, const int32_t *cstart,
                                    int64_t n_c, int64_t nc_pad, int shift, int32_t *nbr8, uint32_t *mask64) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t child[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) child[k] = -1;
  if (q < n_c) {
    int32_t s = cstart[q], e = cstart[q + 1];
    for (int32_t p = s; p < e; ++p) {
      int k = (int)((fkeys[p] >> shift) & 7);
      int32_t row = forder ? forder[p] : p;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j == k) child[j] = row;
    }
  }
  uint32_t m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    nbr8[(int64_t)k * nc_pad + q] = child[k];
    if (__ballot(child[k] >= 0)) m |= 1u << k;
  }
  if ((threadIdx.x & 63) == 0) mask64[q >> 6] = m;
}

// fine-grouped (degree-1) view: fine positions sorted by child index k, each group padded to 256
__global__ void k_child_keys(const uint64_t *fkeys, int64_t n, int shift, uint32_t *kk, int32_t *pp, int32_t *cnt) {
  __shared__ int32_t h[8];
  if (threadIdx.x < 8) h[threadIdx.x] = 0;
  __syncthreads();
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n) {
    uint32_t k = (uint32_t)((fkeys[p] >> shift) & 7);
    kk[p] = k;
    pp[p] = (int32_t)p;
    atomicAdd(&h[k], 1);
  }
  __syncthreads();
  if (threadIdx.x < 8 && h[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], h[threadIdx.x]);
}
__global__ void k_group_offsets(const int32_t *cnt, int32_t *goff /*[9] padded starts*/, int32_t *gsrc /*[9] plain starts*/) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int32_t a = 0, b = 0;
    for (int k = 0; k < 8; ++k) {
      goff[k] = a; gsrc[k] = b;
      a += (cnt[k] + kPadRows - 1) / kPadRows * kPadRows;
      b += cnt[k];
    }
    goff[8] = a; gsrc[8] = b;
  }
}
__global__ void k_fill_i32(int32_t *p, int64_t n, int32_t v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
// several small fills as ONE launch: segment j gets n[j] copies of v[j]
constexpr int kFillSegs = 4;
struct FillSegs { int32_t *p[kFillSegs]; int64_t n[kFillSegs]; int32_t v[kFillSegs]; };
__global__ void k_fill_segs(FillSegs f) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kFillSegs; ++j) {
    if (i < f.n[j]) { f.p[j][i] = f.v[j]; return; }
    i -= f.n[j];
  }
}
__global__ void k_build_map2_fine(const uint32_t *kk_sorted, const int32_t *pp_sorted, int64_t n, const int32_t *goff,
                                  const int32_t *gsrc, const int32_t *fine_cidx, const int32_t *forder,
                                  int32_t *g_nbr, int32_t *g_out, int32_t *tile_k) {
  int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  int k = (int)kk_sorted[s];
  int32_t p = pp_sorted[s];
  int32_t slot = goff[k] + ((int32_t)s - gsrc[k]);
  g_nbr[slot] = fine_cidx[p];
  g_out[slot] = forder ? forder[p] : p;
  if (((s - gsrc[k]) & (kGroup - 1)) == 0) tile_k[slot >> 6] = k;
}
// MAP_OWN_SORTS: the same grouped view without the radix sort.  Sorting the positions by their 3-bit child index, stably, is an
// 8-way partition: position p of child k lands at goff[k] + (the number of earlier positions with child k).  Three plain launches:
// per-workgroup counts of the eight children over chunks of 256 x rounds positions; ONE workgroup that turns the counts of each child
// into exclusive prefixes over the chunks (a wave per child) and writes the group starts k_group_offsets made; and a pass that
// ranks the positions of its chunk (ballots inside a wave, counts of the waves before it through LDS) and writes g_nbr, g_out and
// tile_k directly -- neither the (child, position) pairs nor their sorted copies exist.
constexpr int kCpMaxRounds = 16;  // a workgroup walks its chunk in rounds of 256 positions (child_rounds)
__global__ __launch_bounds__(256) void k_child_hist(const uint64_t *__restrict__ fkeys, int64_t n, int shift, int rounds, int32_t nwg,
                                                    int32_t *__restrict__ wg_cnt /*[8][nwg]*/) {
  __shared__ int32_t h[8];
  if (threadIdx.x < 8) h[threadIdx.x] = 0;
  __syncthreads();
  int32_t c[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) c[b] = 0;
  const int64_t base = (int64_t)blockIdx.x * 256 * rounds;
  for (int i = 0; i < rounds; ++i) {
    const int64_t p = base + i * 256 + threadIdx.x;
    if (p >= n) break;
    const int k = (int)((fkeys[p] >> shift) & 7);
#pragma unroll
    for (int b = 0; b < 8; ++b) c[b] += k == b ? 1 : 0;
  }
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    int32_t v = c[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&h[b], v);
  }
  __syncthreads();
  if (threadIdx.x < 8) wg_cnt[(int64_t)threadIdx.x * nwg + blockIdx.x] = h[threadIdx.x];
}
__global__ __launch_bounds__(512) void k_child_prefix(int32_t *wg_cnt /*[8][nwg]: counts in, exclusive prefixes out*/, int32_t nwg,
                                                      int32_t *goff /*[9] padded starts*/, int32_t *gsrc /*[9] plain starts*/) {
  __shared__ int32_t tot[8];
  const int b = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t *row = wg_cnt + (int64_t)b * nwg;
  int32_t carry = 0;
  for (int32_t w0 = 0; w0 < nwg; w0 += 64) {
    const int32_t w = w0 + lane;
    const int32_t v = w < nwg ? row[w] : 0;
    int32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t u = __shfl_up(inc, o, 64);
      if (lane >= o) inc += u;
    }
    if (w < nwg) row[w] = carry + inc - v;
    carry += __shfl(inc, 63, 64);
  }
  if (lane == 0) tot[b] = carry;
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t a = 0, s = 0;
    for (int k = 0; k < 8; ++k) {
      goff[k] = a; gsrc[k] = s;
      a += (tot[k] + kPadRows - 1) / kPadRows * kPadRows;
      s += tot[k];
    }
    goff[8] = a; gsrc[8] = s;
  }
}
__global__ __launch_bounds__(256) void k_child_scatter(const uint64_t *__restrict__ fkeys, int64_t n, int shift, int rounds, int32_t nwg,
                                                       const int32_t *__restrict__ wg_off, const int32_t *__restrict__ goff,
                                                       const int32_t *__restrict__ fine_cidx, const int32_t *__restrict__ forder,
                                                       int32_t *__restrict__ g_nbr, int32_t *__restrict__ g_out, int32_t *__restrict__ tile_k) {
  __shared__ int32_t run[8], start[8];   // positions of each child before the current round (in this child's group); the group's first slot
  __shared__ int32_t wcnt[2][4][8];      // [round & 1][wave][child]: the round after next reuses a buffer, two barriers later
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  if (t < 8) { run[t] = wg_off[(int64_t)t * nwg + blockIdx.x]; start[t] = goff[t]; }
  const int64_t base = (int64_t)blockIdx.x * 256 * rounds;
  for (int i = 0; i < rounds && base + i * 256 < n; ++i) {   // the bound is the same for the whole workgroup
    const int64_t p = base + i * 256 + t;
    const int k = p < n ? (int)((fkeys[p] >> shift) & 7) : 8;
    int32_t before = 0, mine = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bal = __ballot(k == b);
      if (k == b) before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == b) mine = __popcll(bal);
    }
    if (lane < 8) wcnt[i & 1][wave][lane] = mine;
    __syncthreads();
    if (k < 8) {
      int32_t r = run[k] + before;
      for (int w = 0; w < wave; ++w) r += wcnt[i & 1][w][k];
      const int32_t slot = start[k] + r;
      g_nbr[slot] = fine_cidx[p];
      g_out[slot] = forder ? forder[p] : (int32_t)p;
      if ((r & (kGroup - 1)) == 0) tile_k[slot >> 6] = k;
    }
    __syncthreads();
    if (t < 8) run[t] += wcnt[i & 1][0][t] + wcnt[i & 1][1][t] + wcnt[i & 1][2][t] + wcnt[i & 1][3][t];
  }
}

// export helpers (parity tests): count pairs of a view then write (k, in, out) triples
__global__ void k_view_count(View v, int32_t *count) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.n_pad) return;
  int32_t orow = v.out_row ? v.out_row[p] : (p < v.n_out ? (int32_t)p : -1);
  int c = 0;
  if (orow >= 0) {
    if (!v.nbr) c = 1;
    else
      for (int s = 0; s < v.KS; ++s) c += v.nbr[(int64_t)s * v.n_pad + p] >= 0;
  }
  if (c) atomicAdd(count, c);
}
__global__ void k_view_export(View v, int32_t *cursor, int32_t *ek, int32_t *ein, int32_t *eout) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.n_pad) return;
  int32_t orow = v.out_row ? v.out_row[p] : (p < v.n_out ? (int32_t)p : -1);
  if (orow < 0) return;
  for (int s = 0; s < v.KS; ++s) {
    int32_t i = v.nbr ? v.nbr[(int64_t)s * v.n_pad + p] : (int32_t)p;
    if (i < 0) continue;
    int k = v.tile_k ? v.tile_k[p >> 6] : (v.mirror ? v.K - 1 - s : s);
    int32_t at = atomicAdd(cursor, 1);
    ek[at] = k; ein[at] = i; eout[at] = orow;
  }
}

// ---- origin map + segment maps (pooling / broadcast)
// origin map: one row (b, 0, 0, 0) per batch index, ascending; nb = the count taken at insert time (d_err bit 2 if it differs)
__global__ void k_origin_coords(const uint64_t *skeys, const int32_t *head, const int32_t *cincl, int64_t n, int64_t nb,
                                int32_t *coords, int *d_err) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int32_t q = cincl[p] - 1;
  if (p == n - 1 && (int64_t)q + 1 != nb && d_err) atomicOr(d_err, 4);
  if (q >= nb || !head[p]) return;
  reinterpret_cast<int4 *>(coords)[q] = make_int4((int)(skeys[p] >> kBatchShift), 0, 0, 0);
}
// segments of the origin map over a fine map: one run of sorted positions per batch index
__global__ void k_origin_segments(const int32_t *head, const int32_t *cincl, int64_t n, int64_t nb, int32_t *seg_start,
                                  int32_t *coarse_of) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int32_t q = cincl[p] - 1;
  coarse_of[p] = q < nb ? q : (int32_t)(nb - 1);
  if (q >= nb) return;
  if (head[p]) seg_start[q] = (int32_t)p;
  if (p == n - 1) seg_start[q + 1] = (int32_t)n;
}
// the origin segment map per fine ROW (the inverse of `order` composed with coarse_of): what a row-stationary pass needs
__global__ void k_row_seg(const int32_t *fine_row, const int32_t *coarse_of, int64_t n, int32_t *row_seg) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int32_t r = fine_row[p];
  if (r >= 0 && r < n) row_seg[r] = coarse_of[p];
}
// a stride-2^k segment map composes the k stride-2 steps in between (each keeps the sort, so runs stay runs)
constexpr int kMaxChain = 12;
struct Chain {
  const int32_t *fine_cidx[kMaxChain];  // level j's fine_cidx (indexed by level j-1 sorted positions), j = 1..k
  const int32_t *cstart[kMaxChain];     // level j's cstart [n_j + 1]
  int k;
};
__global__ void k_compose_coarse_of(Chain ch, int64_t n, int32_t *coarse_of) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  int32_t v = (int32_t)p;
  for (int j = 0; j < ch.k; ++j) v = ch.fine_cidx[j][v];
  coarse_of[p] = v;
}
__global__ void k_compose_seg_start(Chain ch, int64_t nc, int32_t *seg_start) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q > nc) return;
  int32_t v = (int32_t)q;
  for (int j = ch.k - 1; j >= 0; --j) v = ch.cstart[j][v];
  seg_start[q] = v;
}
// chunk items of a two-pass map: segment q owns items [item_start[q], item_start[q+1]), ceil(len / kSegChunk) of them
__global__ void k_item_counts(const int32_t *seg_start, int64_t nc, int32_t *cnt) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc) return;
  cnt[q] = (seg_start[q + 1] - seg_start[q] + kSegChunk - 1) / kSegChunk;
}
__global__ void k_item_fill(const int32_t *item_start, int64_t nc, int64_t n_items, int32_t *item_seg) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nc) return;
  for (int32_t j = item_start[q]; j < item_start[q + 1] && j < n_items; ++j) item_seg[j] = (int32_t)q;
}

struct CoordMap {
  int ts = 1, log2ts = 0;
  int64_t n = 0, n_pad = 0;
  int32_t *coords = nullptr;  // [n,4]
  int32_t *order = nullptr;   // sorted position -> row; nullptr = identity
  uint64_t *skeys = nullptr;  // sorted Morton keys [n]
  uint64_t *hkeys = nullptr;  // hash (lazy)
  int32_t *hvals = nullptr;
  int64_t hcap = 0;
  DirEnt *dir = nullptr;      // block directory (lazy)
  int64_t dcap = 0;
  int fine_key = -1, coarse_key = -1;
  bool origin = false;           // one row (b, 0, 0, 0) per batch index (lgs_manager_origin); tensor stride 0
  int32_t *cstart = nullptr;     // [n+1] first fine sorted position of each row (maps made by stride2)
  int32_t *fine_cidx = nullptr;  // [n_fine] coarse row of each fine sorted position
};

}  // namespace lgs

using namespace lgs;

struct lgs_manager {
  int device = 0;
  hipMemPool_t pool = nullptr;
  // All map construction runs on the manager's OWN stream: the host-side row-count syncs then wait for map work
  // only (never for the compute backlog of the caller's stream), and the maps of step t+1 are built while step t's
  // backward is still running.  Consumers order themselves after `ev_ready` (lgs::kmap_wait).
  hipStream_t ms = nullptr;
  hipEvent_t ev_ready = nullptr, ev_in = nullptr;
  std::vector<hipStream_t> users;  // caller streams that consumed this manager's arrays (joined before freeing)
  hipStream_t last_stream = nullptr;
  std::vector<CoordMap> maps;
  std::vector<lgs_kmap *> kmaps;
  std::vector<void *> allocs;      // pool allocations (no arena yet, or the arena was too small)
  int *d_err = nullptr;
  // arena: one device block per manager, bump-allocated (see "arena" below)
  char *arena = nullptr;
  size_t arena_cap = 0, arena_used = 0, arena_peak = 0;
  struct Blk { size_t off, size; bool freed; };
  std::vector<Blk> blks;           // live arena blocks in allocation order (a stack: freed blocks on top are popped)
  size_t pool_live = 0, pool_peak = 0;
  int64_t precount[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // rows of the maps at tensor stride 2^(i+1), counted by the insert (-1: unknown)
  int64_t precount_batches = -1;   // distinct batch indices of the insert = rows of the origin map
  int origin_key = -1;             // lgs_manager_origin's map (-1: not made yet)
  std::vector<lgs_segmap *> segmaps;
};

namespace {

// the entry points run on the manager's device and leave the caller's current device as they found it
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// The maps of step t+1 reuse step t's memory: map arrays come from a PRIVATE stream-ordered pool per device whose
// release threshold is unlimited (the process-wide default pool is left alone).
hipMemPool_t g_pool[64] = {nullptr};
int ensure_pool(int device) {
  if (g_pool[device]) return 0;
  hipMemPoolProps props;
  memset(&props, 0, sizeof(props));
  props.allocType = hipMemAllocationTypePinned;
  props.handleTypes = hipMemHandleTypeNone;
  props.location.type = hipMemLocationTypeDevice;
  props.location.id = device;
  hipMemPool_t pool = nullptr;
  LGS_HIP(hipMemPoolCreate(&pool, &props));
  uint64_t thr = UINT64_MAX;
  LGS_HIP(hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr));
  // blocks freed on a user stream (lgs_manager_destroy) are handed to the map stream only once that free has completed:
  // the allocator must not buy reuse with a stream dependency on the compute stream's tail
  int off = 0;
  (void)hipMemPoolSetAttribute(pool, hipMemPoolReuseAllowInternalDependencies, &off);
  g_pool[device] = pool;
  return 0;
}
// ---- arena.  A manager makes ~150 device allocations per step; as stream-ordered pool calls each of them (and each
// free when the manager dies) is a marker packet in a HIP stream, and freeing a manager cost ~3 ms of stream time per
// step.  Instead every manager owns ONE block, bump-allocated on the host: allocation and release are pointer
// arithmetic; temporaries are released as a stack (a freed block is reclaimed once everything above it is freed too --
// all users of the arena run on the map stream, in order).  Blocks are recycled through a per-device FIFO: when a manager
// dies its block is stamped with one event per user stream and queued; a new manager takes the OLDEST queued block (its
// users finished a step ago, so the wait on its events is already satisfied) or, while fewer than two are queued,
// allocates a new one sized to the largest need seen so far.  Steady state: three blocks in rotation, no allocator
// call at all.  Whatever does not fit (first step, growing scenes) falls back to the private stream-ordered pool.
struct ArenaBlock { char *base; size_t cap; std::vector<hipEvent_t> ready; };
std::vector<ArenaBlock> g_arenas[64];   // FIFO of released blocks per device
size_t g_arena_need[64] = {0};          // largest (arena peak + pool peak) any manager of this device has needed

inline hipError_t pool_alloc(lgs_manager *m, void **q, size_t bytes, hipStream_t s) {
  return hipMallocFromPoolAsync(q, bytes, m->pool, s);
}
int raw_alloc(lgs_manager *m, void **p, size_t bytes, hipStream_t s) {
  bytes = (bytes + 255) / 256 * 256;
  if (m->arena && m->arena_used + bytes <= m->arena_cap) {
    *p = m->arena + m->arena_used;
    m->blks.push_back({m->arena_used, bytes, false});
    m->arena_used += bytes;
    if (m->arena_used > m->arena_peak) m->arena_peak = m->arena_used;
    return 0;
  }
  void *q = nullptr;
  LGS_HIP(pool_alloc(m, &q, bytes, s));
  m->allocs.push_back(q);
  m->pool_live += bytes;
  if (m->pool_live > m->pool_peak) m->pool_peak = m->pool_live;
  *p = q;
  return 0;
}
template <typename T>
int dalloc(lgs_manager *m, T **p, int64_t count, hipStream_t s) {
  void *q = nullptr;
  if (raw_alloc(m, &q, sizeof(T) * (size_t)(count > 0 ? count : 1), s)) return 1;
  *p = reinterpret_cast<T *>(q);
  return 0;
}
int dfree_now(lgs_manager *m, void *q, hipStream_t s) {  // temp buffer: release early
  char *c = reinterpret_cast<char *>(q);
  if (m->arena && c >= m->arena && c < m->arena + m->arena_cap) {
    const size_t off = (size_t)(c - m->arena);
    for (size_t i = m->blks.size(); i-- > 0;)
      if (m->blks[i].off == off) { m->blks[i].freed = true; break; }
    while (!m->blks.empty() && m->blks.back().freed) { m->arena_used = m->blks.back().off; m->blks.pop_back(); }
    return 0;
  }
  for (size_t i = 0; i < m->allocs.size(); ++i)
    if (m->allocs[i] == q) { m->allocs[i] = m->allocs.back(); m->allocs.pop_back(); break; }
  LGS_HIP(hipFreeAsync(q, s));
  return 0;
}
// take a recycled block (or a new one) for a fresh manager; the map stream waits for the block's previous users
int arena_acquire(lgs_manager *m) {
  const int dev = m->device;
  const size_t need = g_arena_need[dev];
  if (need == 0) return 0;                       // first manager of the device: measure through the pool
  std::vector<ArenaBlock> &q = g_arenas[dev];
  // never the most recently released block (its users -- the previous step's backward -- are still running)
  for (size_t i = 0; q.size() >= 2 && i + 1 < q.size(); ++i) {
    if (q[i].cap >= need) {
      ArenaBlock b = q[i];
      q.erase(q.begin() + (long)i);
      if (tune(T_ARENA_DBG)) {
        int pending = 0;
        for (hipEvent_t e : b.ready) pending += hipEventQuery(e) == hipSuccess ? 0 : 1;
        fprintf(stderr, "[arena] reuse block %zu of %zu (cap %zu MB, need %zu MB): %d of %zu events still pending\n", i, q.size() + 1, b.cap >> 20,
                need >> 20, pending, b.ready.size());
      }
      for (hipEvent_t e : b.ready) { (void)hipStreamWaitEvent(m->ms, e, 0); (void)hipEventDestroy(e); }
      m->arena = b.base; m->arena_cap = b.cap;
      return 0;
    }
    if (i == 0 && q.size() >= 4) {               // an undersized block at the head of a long queue: retire it
      for (hipEvent_t e : q[0].ready) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); }
      (void)hipFree(q[0].base);
      q.erase(q.begin());
      i = (size_t)-1;
    }
  }
  const size_t cap = (need + need / 4 + (2u << 20)) / (2u << 20) * (2u << 20);
  if (tune(T_ARENA_DBG)) fprintf(stderr, "[arena] hipMalloc %zu MB (need %zu MB, %zu queued)\n", cap >> 20, need >> 20, q.size());
  void *p = nullptr;
  if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return 0; }   // no block: this manager uses the pool
  m->arena = reinterpret_cast<char *>(p); m->arena_cap = cap;
  return 0;
}
void arena_release(lgs_manager *m) {
  const size_t need = m->arena_peak + m->pool_peak;
  if (need > g_arena_need[m->device]) g_arena_need[m->device] = need;
  if (!m->arena) return;
  ArenaBlock b{m->arena, m->arena_cap, {}};
  std::vector<hipStream_t> streams = m->users;
  streams.push_back(m->ms);
  for (hipStream_t u : streams) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) {
      if (hipEventRecord(e, u) == hipSuccess) b.ready.push_back(e); else (void)hipEventDestroy(e);
    }
  }
  g_arenas[m->device].push_back(b);
  m->arena = nullptr;
}
void add_user(lgs_manager *m, hipStream_t caller) {
  for (hipStream_t u : m->users)
    if (u == caller) return;
  m->users.push_back(caller);
}
// inputs produced on the caller's stream must be complete before map work that reads them
int begin_from_caller(lgs_manager *m, hipStream_t caller) {
  LGS_HIP(hipEventRecord(m->ev_in, caller));
  LGS_HIP(hipStreamWaitEvent(m->ms, m->ev_in, 0));
  return 0;
}
// publish map work; if `caller` is given it is ordered after it (outputs written into caller-owned memory)
int publish(lgs_manager *m, hipStream_t caller, bool caller_waits) {
  LGS_HIP(hipEventRecord(m->ev_ready, m->ms));
  if (caller_waits) {
    LGS_HIP(hipStreamWaitEvent(caller, m->ev_ready, 0));
    add_user(m, caller);
  }
  return 0;
}
inline unsigned nblk(int64_t n, int t = 256) { return (unsigned)((n + t - 1) / t > 0 ? (n + t - 1) / t : 1); }

int ensure_hash(lgs_manager *m, CoordMap &cm, hipStream_t s) {
  if (cm.hkeys) return 0;
  int64_t cap = 1024;
  while (cap < 2 * cm.n) cap <<= 1;
  cm.hcap = cap;
  if (dalloc(m, &cm.hkeys, cap, s)) return 1;
  if (dalloc(m, &cm.hvals, cap, s)) return 1;
  LGS_KLAUNCH(k_hash_fill, nblk(cap), 256, 0, s, cm.hkeys, cap);
  if (cm.n > 0)
    LGS_KLAUNCH(k_hash_insert, nblk(cm.n), 256, 0, s, cm.skeys, cm.order, cm.n, cm.hkeys, cm.hvals,
                       (uint64_t)(cap - 1));
  LGS_HIP(hipGetLastError());
  return 0;
}

// the block directory of a map (MAP_BLOCK_DIR), built where the per-voxel hash would be.  A block of the map at tensor stride 2^t
// is a cell of the map two levels coarser, whose row count lgs_manager_insert already took (precount): the table is sized from
// it without a host synchronisation, and from n (one block per row at the worst) where that count is not known.
int ensure_dir(lgs_manager *m, CoordMap &cm, hipStream_t s) {
  if (cm.dir) return 0;
  int64_t blocks = cm.n;
  const int lv = cm.log2ts + 2;
  if (lv <= kPreLevels && m->precount[lv - 1] >= 0 && m->precount[lv - 1] < blocks) blocks = m->precount[lv - 1];
  int64_t cap = 1024;
  while (cap < 2 * blocks) cap <<= 1;
  cm.dcap = cap;
  if (dalloc(m, &cm.dir, cap, s)) return 1;
  LGS_KLAUNCH(k_dir_fill, nblk(cap), 256, 0, s, cm.dir, cap);
  if (cm.n > 0) LGS_KLAUNCH(k_dir_build, nblk(cm.n), 256, 0, s, cm.skeys, cm.n, 3 * cm.log2ts, cm.dir, (uint64_t)(cap - 1), m->d_err);
  LGS_HIP(hipGetLastError());
  return 0;
}
inline bool use_block_dir() { return tune(T_MAP_BLOCK_DIR) != 0; }
// the table the probe kernels look a map's keys up in: only the one the knob names is built
int ensure_lookup(lgs_manager *m, CoordMap &cm, hipStream_t s) { return use_block_dir() ? ensure_dir(m, cm, s) : ensure_hash(m, cm, s); }
inline HashRef hash_ref(const CoordMap &cm) { return HashRef{cm.hkeys, cm.hvals, (uint64_t)(cm.hcap - 1)}; }
inline DirRef dir_ref(const CoordMap &cm) { return DirRef{cm.dir, (uint64_t)(cm.dcap - 1), 3 * cm.log2ts, cm.order}; }

// several small fills as one launch (k_fill_segs)
int fill_segs(hipStream_t s, std::initializer_list<std::tuple<void *, int64_t, int32_t>> segs) {
  FillSegs f = {};
  int64_t total = 0;
  int j = 0;
  for (const auto &g : segs) {
    f.p[j] = reinterpret_cast<int32_t *>(std::get<0>(g)); f.n[j] = std::get<1>(g); f.v[j] = std::get<2>(g);
    total += f.n[j++];
  }
  LGS_KLAUNCH(k_fill_segs, nblk(total), 256, 0, s, f);
  return 0;
}

int scan_incl(lgs_manager *m, const int32_t *in, int32_t *out, int64_t n, hipStream_t s) {
  size_t tb = 0;
  LGS_HIP(rocprim::inclusive_scan(nullptr, tb, in, out, (size_t)n, rocprim::plus<int32_t>(), s));
  void *tmp = nullptr;
  if (raw_alloc(m, &tmp, tb ? tb : 16, s)) return 1;
  LGS_HIP(rocprim::inclusive_scan(tmp, tb, in, out, (size_t)n, rocprim::plus<int32_t>(), s));
  if (dfree_now(m, tmp, s)) return 1;
  return 0;
}

// radix sort of (key, value) pairs on key bits [begin_bit, end_bit); rocPRIM's temporary is taken from and returned to the arena's top
template <typename K, typename V>
int sort_pairs(lgs_manager *m, K *keys, K *keys_out, V *vals, V *vals_out, int64_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  size_t tb = 0;
  LGS_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys, keys_out, vals, vals_out, (size_t)n, begin_bit, end_bit, s));
  void *tmp = nullptr;
  if (raw_alloc(m, &tmp, tb ? tb : 16, s)) return 1;
  LGS_HIP(rocprim::radix_sort_pairs(tmp, tb, keys, keys_out, vals, vals_out, (size_t)n, begin_bit, end_bit, s));
  return dfree_now(m, tmp, s);
}

// head[p] = 1 where sorted key p starts a new batch index; cincl = its inclusive scan (the origin map's row of every position, + 1)
int batch_heads(lgs_manager *m, const uint64_t *skeys, int64_t n, int32_t *head, int32_t *cincl, hipStream_t s) {
  LGS_KLAUNCH(k_heads, nblk(n), 256, 0, s, skeys, n, ~((1ull << kBatchShift) - 1), head);
  return scan_incl(m, head, cincl, n, s);
}

// the window mask sort of a 27-slot table built in sorted-position order (nbr_tmp, pmask) and its permutation into the view's arrays:
// position q of the view is sorted position perm[q] and writes row order[perm[q]] (order == nullptr: the position itself).
// MAP_WINDOW_SORT: one k_window_sort launch where the window is a power of two that fits the LDS (window_sort_log2); else the radix
// sort of (window, code) keys with its four n_pad-sized temporaries.
int window_perm(lgs_manager *m, int64_t n, int64_t n_pad, const uint32_t *pmask, int32_t *perm, hipStream_t s) {
  const int64_t window = tune(T_MASK_WINDOW);   // tuning knob (default kMaskWindow)
  const int order = (int)tune(T_MASK_ORDER);
  const int log2w = tune(T_MAP_WINDOW_SORT) != 0 ? window_sort_log2(window) : -1;
  if (log2w >= 0) {
    static bool attr_set = false;
    if (!attr_set) {
      LGS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_window_sort), hipFuncAttributeMaxDynamicSharedMemorySize, (int)window_sort_lds(kWsMaxLog2)));
      attr_set = true;
    }
    // a map of one window sorts the smallest power of two that holds its positions (what lies beyond is padding, which sorts last)
    int l = log2w;
    while (l > kWsMinLog2 && n_pad <= (1ll << (l - 1))) --l;
    LGS_KLAUNCH(k_window_sort, (unsigned)((n_pad + (1ll << l) - 1) >> l), 1u << (l - 4), window_sort_lds(l), s, pmask, n, n_pad, l, order, perm);
    return 0;
  }
  uint64_t *keys, *skeys2; int32_t *vals;
  if (dalloc(m, &keys, n_pad, s) || dalloc(m, &skeys2, n_pad, s) || dalloc(m, &vals, n_pad, s)) return 1;
  LGS_KLAUNCH(k_mask_sort_keys, (unsigned)(n_pad / 256), 256, 0, s, pmask, n, n_pad, (int)window, order, keys, vals);
  if (sort_pairs(m, keys, skeys2, vals, perm, n_pad, 0, mask_sort_bits(n_pad, (int)window), s)) return 1;
  return dfree_now(m, keys, s) || dfree_now(m, skeys2, s) || dfree_now(m, vals, s);
}

// the permutation of (nbr_tmp, pmask) into the view's arrays.  MAP_PERMUTE_LDS: through LDS (k_permute_map3_lds) where a window's
// row segment fits it and windows are whole groups of 256 positions; else, and with the knob at 0, k_permute_map3
// Offsets per workgroup (MAP_PERMUTE_GROUP): a workgroup walks its offsets one after the other and a CU holds two workgroups, so
// a small map wants one offset per workgroup to fill the chip at all, and a large one as many as still leave the grid above
// kPlWorkgroups -- every offset group reads the window's perm again
constexpr int kPlWorkgroups = 640;
inline int permute_group(int64_t windows) {
  const int64_t g = tune(T_MAP_PERMUTE_GROUP);
  if (g >= 1 && g <= 27) return (int)g;
  const int64_t kg = 27 * windows / (g > 27 ? g : kPlWorkgroups);
  return (int)(kg < 1 ? 1 : (kg > 27 ? 27 : kg));
}
int permute_rows(const CoordMap &st, const int32_t *nbr_tmp, const uint32_t *pmask, const int32_t *perm, hipStream_t s, int32_t *nbr,
                 int32_t *orow, uint32_t *mask) {
  const int64_t window = tune(T_MASK_WINDOW), knob = tune(T_MAP_PERMUTE_LDS);
  if (knob <= 0 || window <= 0 || window > kPlMaxWindow || window % 256 != 0) {
    LGS_KLAUNCH(k_permute_map3, (unsigned)(st.n_pad / 256), 256, 0, s, nbr_tmp, pmask, perm, st.order, st.n, st.n_pad, nbr, orow, mask);
    return 0;
  }
  static bool attr_set = false;
  if (!attr_set) {
    LGS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_permute_map3_lds<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 16 * kPlThreads * 4));
    LGS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_permute_map3_lds<32>), hipFuncAttributeMaxDynamicSharedMemorySize, kPlMaxWindow * 4));
    attr_set = true;
  }
  const int64_t windows = (st.n_pad + window - 1) / window;
  const int kg = permute_group(windows);
  const dim3 grid((unsigned)windows, (unsigned)((27 + kg - 1) / kg));
  const size_t lds = (size_t)(st.n_pad < window ? st.n_pad : window) * sizeof(int32_t);
  if (window <= 16 * kPlThreads)
    LGS_KLAUNCH(k_permute_map3_lds<16>, grid, kPlThreads, lds, s, nbr_tmp, pmask, perm, st.order, st.n, st.n_pad, (int)window, kg, nbr, orow, mask);
  else
    LGS_KLAUNCH(k_permute_map3_lds<32>, grid, kPlThreads, lds, s, nbr_tmp, pmask, perm, st.order, st.n, st.n_pad, (int)window, kg, nbr, orow, mask);
  return 0;
}

// a 27-slot view over the rows of map `st` (the stationary side): table built by `build` into (nbr_tmp, pmask), then the window sort
template <typename Build>
int make_view27(lgs_manager *m, const CoordMap &st, int64_t n_in, hipStream_t s, View &v, Build &&build) {
  v = View();
  v.n_pad = st.n_pad; v.n_out = st.n; v.n_in = n_in; v.KS = 27; v.K = 27;
  if (st.n == 0) return 0;
  int32_t *nbr, *orow, *nbr_tmp, *perm; uint32_t *mask, *pmask;
  if (dalloc(m, &nbr, 27 * st.n_pad, s) || dalloc(m, &mask, st.n_pad / kGroup, s) || dalloc(m, &orow, st.n_pad, s) ||
      dalloc(m, &nbr_tmp, 27 * st.n_pad, s) || dalloc(m, &pmask, st.n_pad, s) || dalloc(m, &perm, st.n_pad, s))
    return 1;
  if (build(nbr_tmp, pmask)) return 1;
  if (window_perm(m, st.n, st.n_pad, pmask, perm, s)) return 1;
  if (permute_rows(st, nbr_tmp, pmask, perm, s, nbr, orow, mask)) return 1;
  LGS_HIP(hipGetLastError());
  if (dfree_now(m, nbr_tmp, s) || dfree_now(m, pmask, s) || dfree_now(m, perm, s)) return 1;
  v.nbr = nbr; v.mask64 = mask; v.out_row = orow;
  return 0;
}


// ---- kernel maps: one builder per relation (KmapRelation, lgs_common.h), all on the map stream
// identity 1x1: no table
void build_identity(const CoordMap &ci, lgs_kmap *km) {
  View v; v.n_pad = ci.n_pad; v.n_out = ci.n; v.n_in = ci.n; v.KS = 1; v.K = 1;
  km->fwd = v; km->bwd = v;
}

// a 27-slot view over the rows of `st` whose slot k holds the row of `probed` at c + off_k * scale: the 27 probes of k_build_map3
// from st's sorted keys into probed's lookup table (st == probed: the stride-1 maps; st = the coarse map: the coarse-stationary strided
// view).  A probed coordinate is always on the probed map's grid, so dilation needs no special case in either table.
int probe_view27(lgs_manager *m, const CoordMap &st, const CoordMap &probed, int scale, hipStream_t s, View &v) {
  return make_view27(m, st, probed.n, s, v, [&](int32_t *nbr_tmp, uint32_t *pmask) {
    if (use_block_dir())
      LGS_KLAUNCH(k_build_map3<DirRef>, (unsigned)(st.n_pad / 256), 256, 0, s, st.skeys, st.n, st.n_pad, scale, dir_ref(probed), nbr_tmp, pmask);
    else
      LGS_KLAUNCH(k_build_map3<HashRef>, (unsigned)(st.n_pad / 256), 256, 0, s, st.skeys, st.n, st.n_pad, scale, hash_ref(probed), nbr_tmp, pmask);
    return 0;
  });
}

// 3^3 stride 1, plain (dilation 1) or dilated: offsets scaled by dilation * ts; bwd = the same table read mirrored
int build_conv3(lgs_manager *m, CoordMap &ci, int dilation, hipStream_t s, lgs_kmap *km) {
  if (ci.n > 0 && ensure_lookup(m, ci, s)) return 1;
  View v;
  if (probe_view27(m, ci, ci, dilation * ci.ts, s, v)) return 1;
  km->fwd = v;
  km->bwd = v; km->bwd.mirror = 1;
  return 0;
}

// MAP_OWN_SORTS: rounds of 256 positions per workgroup of k_child_hist / k_child_scatter (MAP_CHILD_ROUNDS).  A round costs the
// workgroup two barriers and a dependent load, so a small map takes one round per workgroup and a large one as many as still leave
// kCpWorkgroups workgroups -- the prefix kernel is one workgroup and walks them all
constexpr int kCpWorkgroups = 512;
inline int child_rounds(int64_t n) {
  const int64_t k = tune(T_MAP_CHILD_ROUNDS);
  if (k >= 1) return (int)(k > kCpMaxRounds ? kCpMaxRounds : k);
  const int64_t r = (n + 255) / 256 / kCpWorkgroups;
  return (int)(r < 1 ? 1 : (r > kCpMaxRounds ? kCpMaxRounds : r));
}

// 2^3 stride 2: the children of a coarse row are one run of the fine Morton order
int build_conv2_s2(lgs_manager *m, const CoordMap &ci, const CoordMap &co, hipStream_t s, lgs_kmap *km) {
  int shift = 3 * ci.log2ts;
  View vf, vb;
  vf.KS = 8; vf.K = 8; vf.n_pad = co.n_pad; vf.n_out = co.n; vf.n_in = ci.n;
  vb.KS = 1; vb.K = 8; vb.n_out = ci.n; vb.n_in = co.n;
  if (ci.n > 0) {
    int32_t *nbr8; uint32_t *mask;
    if (dalloc(m, &nbr8, 8 * co.n_pad, s) || dalloc(m, &mask, co.n_pad / kGroup, s)) return 1;
    LGS_KLAUNCH(k_build_map2_coarse, (unsigned)(co.n_pad / 256), 256, 0, s, ci.skeys, ci.order, co.cstart, co.n,
                       co.n_pad, shift, nbr8, mask);
    vf.nbr = nbr8; vf.mask64 = mask;
    // grouped fine view
    int64_t n = ci.n, gp = pad_rows(n + 8 * kPadRows);
    if (tune(T_MAP_OWN_SORTS) != 0) {   // the stable 8-way partition (k_child_hist)
      const int rounds = child_rounds(n);
      const int32_t nwg = (int32_t)((n + 256 * rounds - 1) / (256 * rounds));
      int32_t *wg, *goff, *gsrc, *g_nbr, *g_out, *tile_k;
      if (dalloc(m, &g_nbr, gp, s) || dalloc(m, &g_out, gp, s) || dalloc(m, &tile_k, gp / kGroup, s) || dalloc(m, &wg, 8 * (int64_t)nwg, s) ||
          dalloc(m, &goff, 9, s) || dalloc(m, &gsrc, 9, s))
        return 1;
      if (fill_segs(s, {{g_nbr, gp, -1}, {g_out, gp, -1}, {tile_k, gp / kGroup, -1}})) return 1;
      LGS_KLAUNCH(k_child_hist, (unsigned)nwg, 256, 0, s, ci.skeys, n, shift, rounds, nwg, wg);
      LGS_KLAUNCH(k_child_prefix, 1, 512, 0, s, wg, nwg, goff, gsrc);
      LGS_KLAUNCH(k_child_scatter, (unsigned)nwg, 256, 0, s, ci.skeys, n, shift, rounds, nwg, wg, goff, co.fine_cidx, ci.order, g_nbr, g_out, tile_k);
      LGS_HIP(hipGetLastError());
      vb.nbr = g_nbr; vb.out_row = g_out; vb.tile_k = tile_k; vb.n_pad = gp;
      if (dfree_now(m, wg, s) || dfree_now(m, goff, s) || dfree_now(m, gsrc, s)) return 1;
      km->fwd = vf; km->bwd = vb;
      return 0;
    }
    uint32_t *kk, *kks; int32_t *pp, *pps, *cnt, *goff, *gsrc, *g_nbr, *g_out, *tile_k;
    if (dalloc(m, &kk, n, s) || dalloc(m, &kks, n, s) || dalloc(m, &pp, n, s) || dalloc(m, &pps, n, s) ||
        dalloc(m, &cnt, 8, s) || dalloc(m, &goff, 9, s) || dalloc(m, &gsrc, 9, s) || dalloc(m, &g_nbr, gp, s) ||
        dalloc(m, &g_out, gp, s) || dalloc(m, &tile_k, gp / kGroup, s))
      return 1;
    if (fill_segs(s, {{cnt, 8, 0}, {g_nbr, gp, -1}, {g_out, gp, -1}, {tile_k, gp / kGroup, -1}})) return 1;
    LGS_KLAUNCH(k_child_keys, nblk(n), 256, 0, s, ci.skeys, n, shift, kk, pp, cnt);
    if (sort_pairs(m, kk, kks, pp, pps, n, 0, 3, s)) return 1;
    LGS_KLAUNCH(k_group_offsets, 1, 64, 0, s, cnt, goff, gsrc);
    LGS_KLAUNCH(k_build_map2_fine, nblk(n), 256, 0, s, kks, pps, n, goff, gsrc, co.fine_cidx, ci.order, g_nbr,
                       g_out, tile_k);
    LGS_HIP(hipGetLastError());
    vb.nbr = g_nbr; vb.out_row = g_out; vb.tile_k = tile_k; vb.n_pad = gp;
    if (dfree_now(m, kk, s) || dfree_now(m, kks, s) || dfree_now(m, pp, s) || dfree_now(m, pps, s) ||
        dfree_now(m, cnt, s) || dfree_now(m, goff, s) || dfree_now(m, gsrc, s))
      return 1;
  }
  km->fwd = vf; km->bwd = vb;
  return 0;
}

// 3^3 stride 2.  Both views carry offset k in slot k (no mirroring): the fine-stationary one lists, per fine row, the coarse row of
// the pair (k, fine, coarse) under the k of the forward direction
int build_conv3_s2(lgs_manager *m, CoordMap &ci, CoordMap &co, hipStream_t s, lgs_kmap *km) {
  if (ci.n > 0 && (ensure_lookup(m, ci, s) || ensure_lookup(m, co, s))) return 1;
  // coarse-stationary: from the coarse rows' keys into the FINE map's table, offsets scaled by ts_in
  if (probe_view27(m, co, ci, ci.ts, s, km->fwd)) return 1;
  return make_view27(m, ci, co.n, s, km->bwd, [&](int32_t *nbr_tmp, uint32_t *pmask) {
    if (use_block_dir())
      LGS_KLAUNCH(k_build_map3_fine<DirRef>, (unsigned)(ci.n_pad / 256), 256, 0, s, ci.skeys, ci.n, ci.n_pad, ci.log2ts, dir_ref(co), nbr_tmp, pmask);
    else
      LGS_KLAUNCH(k_build_map3_fine<HashRef>, (unsigned)(ci.n_pad / 256), 256, 0, s, ci.skeys, ci.n, ci.n_pad, ci.log2ts, hash_ref(co), nbr_tmp, pmask);
    return 0;
  });
}

// 1x1 stride 2: plain nbr (/ out_row) pairs on the KS = 1 path
int build_conv1_s2(lgs_manager *m, const CoordMap &ci, const CoordMap &co, hipStream_t s, lgs_kmap *km) {
  View vf, vb;
  vf.KS = 1; vf.K = 1; vf.n_pad = co.n_pad; vf.n_out = co.n; vf.n_in = ci.n;
  vb.KS = 1; vb.K = 1; vb.n_pad = ci.n_pad; vb.n_out = ci.n; vb.n_in = co.n;
  if (ci.n > 0) {
    int32_t *nf, *nb, *ob;
    if (dalloc(m, &nf, co.n_pad, s) || dalloc(m, &nb, ci.n_pad, s) || dalloc(m, &ob, ci.n_pad, s)) return 1;
    LGS_KLAUNCH(k_build_map1_coarse, nblk(co.n_pad), 256, 0, s, ci.skeys, ci.order, co.skeys, co.cstart, co.n, co.n_pad, nf);
    LGS_KLAUNCH(k_build_map1_fine, nblk(ci.n_pad), 256, 0, s, ci.skeys, ci.order, co.fine_cidx, ci.n, ci.n_pad, 7ull << (3 * ci.log2ts), nb, ob);
    LGS_HIP(hipGetLastError());
    vf.nbr = nf; vb.nbr = nb; vb.out_row = ob;
  }
  km->fwd = vf; km->bwd = vb;
  return 0;
}

// both map entry points (`who` names the one that was called): argument checks, the classifier, the cache, the relation's builder
int kernel_map(bool ex, const char *who, lgs_manager *m, int in_key, int out_key, int ks, int dilation, lgs_kmap **out) {
  LGS_REQUIRE(m && out, std::string(who) + ": null argument");
  const int nm = (int)m->maps.size();
  LGS_REQUIRE(in_key >= 0 && in_key < nm && out_key >= 0 && out_key < nm, std::string(who) + ": bad key");
  CoordMap &ci = m->maps[in_key], &co = m->maps[out_key];
  KmapRelation rel = kRelIdentity;
  const char *refusal = classify_kmap(KmapRequest{ex, in_key == out_key, co.fine_key == in_key, co.order == nullptr, ci.origin || co.origin, ks,
                                                  dilation, ci.ts}, rel);
  LGS_REQUIRE(refusal == nullptr, refusal);
  const KmapTraits t = traits_of(rel);
  if (rel != kRelConv3Dilated) dilation = 1;
  for (lgs_kmap *k : m->kmaps)
    if (k->in_key == in_key && k->out_key == out_key && k->relation == rel && k->dilation == dilation) { *out = k; return 0; }
  hipStream_t s = m->ms;
  DeviceGuard guard(m->device);
  std::unique_ptr<lgs_kmap> km(new lgs_kmap());
  km->mgr = m; km->in_key = in_key; km->out_key = out_key; km->ks = t.ks; km->K = t.K; km->relation = rel; km->dilation = dilation;
  int rc = 0;
  switch (rel) {
    case kRelIdentity: build_identity(ci, km.get()); break;
    case kRelConv3:
    case kRelConv3Dilated: rc = build_conv3(m, ci, dilation, s, km.get()); break;
    case kRelConv2S2: rc = build_conv2_s2(m, ci, co, s, km.get()); break;
    case kRelConv3S2: rc = build_conv3_s2(m, ci, co, s, km.get()); break;
    case kRelConv1S2: rc = build_conv1_s2(m, ci, co, s, km.get()); break;
  }
  if (rc) return rc;
  m->kmaps.push_back(km.get());
  *out = km.release();
  return publish(m, nullptr, false);
}
}  // namespace

namespace lgs {
int kmap_wait(lgs_kmap *km, hipStream_t stream) {
  lgs_manager *m = km->mgr;
  LGS_HIP(hipStreamWaitEvent(stream, m->ev_ready, 0));
  add_user(m, stream);
  return 0;
}
int segmap_wait(lgs_segmap *sm, hipStream_t stream) {
  lgs_manager *m = sm->mgr;
  LGS_HIP(hipStreamWaitEvent(stream, m->ev_ready, 0));
  add_user(m, stream);
  return 0;
}
}  // namespace lgs

extern "C" {

int lgs_abi_version(void) { return LGS_ABI_VERSION; }
const char *lgs_last_error(void) { return g_err.c_str(); }

int lgs_manager_create(int device, lgs_manager **out) {
  LGS_REQUIRE(out != nullptr, "lgs_manager_create: null out");
  LGS_REQUIRE(device >= 0 && device < 64, "lgs_manager_create: device index out of range");
  DeviceGuard guard(device);
  if (ensure_pool(device)) return 1;
  lgs_manager *m = new lgs_manager();
  m->device = device;
  m->pool = g_pool[device];
  // one map stream per device for the whole process (creating / destroying a stream per batch costs host time and
  // can block): managers of consecutive steps simply queue behind each other on it
  static hipStream_t g_map_stream[64] = {nullptr};
  if (!g_map_stream[device]) LGS_HIP(hipStreamCreateWithFlags(&g_map_stream[device], hipStreamNonBlocking));
  m->ms = g_map_stream[device];
  LGS_HIP(hipEventCreateWithFlags(&m->ev_ready, hipEventDisableTiming));
  LGS_HIP(hipEventCreateWithFlags(&m->ev_in, hipEventDisableTiming));
  arena_acquire(m);
  *out = m;
  return 0;
}

int lgs_manager_destroy(lgs_manager *m) {
  if (!m) return 0;
  DeviceGuard guard(m->device);
  // Every stream that read the maps must be done with them before the (stream-ordered) frees.  The frees are queued on
  // one of the USER streams (after joining the others and the manager's last map work), not on the map stream: making the
  // map stream wait for the users -- i.e. for the end of this step's backward -- would hold back the map construction of
  // the NEXT step, which is queued on that stream and is meant to run during this backward (measured: +3.5 ms per step).
  hipStream_t fs = m->users.empty() ? m->ms : m->users.back();
  if (!m->users.empty()) {
    for (hipStream_t u : m->users) {
      if (u == fs) continue;
      if (hipEventRecord(m->ev_in, u) == hipSuccess) (void)hipStreamWaitEvent(fs, m->ev_in, 0);
    }
    (void)hipStreamWaitEvent(fs, m->ev_ready, 0);   // the manager's own last map work (as recorded by its last publish)
  }
  for (void *p : m->allocs) (void)hipFreeAsync(p, fs);   // pool fallbacks only (none in the steady state)
  arena_release(m);                                      // the block goes back to the device's FIFO, stamped per user stream
  for (lgs_kmap *k : m->kmaps) delete k;
  for (lgs_segmap *k : m->segmaps) delete k;
  (void)hipEventDestroy(m->ev_ready);
  (void)hipEventDestroy(m->ev_in);
  delete m;
  return 0;
}

int lgs_manager_insert(lgs_manager *m, const int32_t *coords, int64_t n, int64_t *unique_index, int64_t *inverse,
                       void *stream, int *key, int64_t *n_unique) {
  LGS_REQUIRE(m && key && n_unique, "lgs_manager_insert: null argument");
  LGS_REQUIRE(m->maps.empty(), "lgs_manager_insert: manager already holds a stride-1 map");
  LGS_REQUIRE(n >= 0 && n < (1ll << 31) - 1024, "lgs_manager_insert: row count out of range");
  hipStream_t caller = (hipStream_t)stream;
  hipStream_t s = m->ms;
  DeviceGuard guard(m->device);
  m->last_stream = caller;
  if (begin_from_caller(m, caller)) return 1;   // `coords` was produced on the caller's stream
  CoordMap cm;
  if (n == 0) {
    cm.n = 0; cm.n_pad = 0;
    m->maps.push_back(cm);
    *key = 0; *n_unique = 0;
    return 0;
  }
  if (!m->d_err) { if (dalloc(m, &m->d_err, 1, s)) return 1; }
  uint64_t *keys, *skeys; int32_t *vals, *svals, *head, *runid, *is_first, *urow, *lvl_counts;
  if (dalloc(m, &lvl_counts, kPreLevels + 1, s) || dalloc(m, &keys, n, s) || dalloc(m, &skeys, n, s) || dalloc(m, &vals, n, s) || dalloc(m, &svals, n, s) ||
      dalloc(m, &head, n, s) || dalloc(m, &runid, n, s) || dalloc(m, &is_first, n, s) || dalloc(m, &urow, n + 1, s))
    return 1;
  // d_err, the first slot of the exclusive scan and the level counters: one launch
  if (fill_segs(s, {{m->d_err, 1, 0}, {urow, 1, 0}, {lvl_counts, kPreLevels + 1, 0}})) return 1;
  LGS_KLAUNCH(k_pack_keys, nblk(n), 256, 0, s, coords, n, keys, vals, m->d_err);
  if (sort_pairs(m, keys, skeys, vals, svals, n, 0, 64, s)) return 1;
  LGS_KLAUNCH(k_heads, nblk(n), 256, 0, s, skeys, n, ~0ull, head);
  LGS_KLAUNCH(k_mark_first, nblk(n), 256, 0, s, svals, head, n, is_first);
  if (scan_incl(m, head, runid, n, s)) return 1;
  if (scan_incl(m, is_first, urow + 1, n, s)) return 1;   // exclusive scan of is_first = inclusive shifted: urow[0] = 0, urow[i+1] = incl[i]
  LGS_KLAUNCH(k_count_levels, (unsigned)((n + 256 * kCountPerThread - 1) / (256 * kCountPerThread)), 256, 0, s, skeys, n, lvl_counts);
  int32_t h_nu = 0; int h_err = 0; int32_t h_lvl[kPreLevels + 1];
  LGS_HIP(hipMemcpyAsync(&h_nu, urow + n, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(&h_err, m->d_err, sizeof(int), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipMemcpyAsync(h_lvl, lvl_counts, sizeof(int32_t) * (kPreLevels + 1), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < kPreLevels; ++i) m->precount[i] = h_lvl[i];
  m->precount_batches = h_lvl[kPreLevels];
  LGS_REQUIRE(h_err == 0,
              "lgs_manager_insert: coordinate out of range (batch must be in [0,1024), |x|,|y|,|z| < 131008)");
  int64_t nu = h_nu;
  cm.n = nu; cm.n_pad = pad_rows(nu);
  if (dalloc(m, &cm.coords, nu * 4, s) || dalloc(m, &cm.order, nu, s) || dalloc(m, &cm.skeys, nu, s)) return 1;
  LGS_KLAUNCH(k_emit_unique, nblk(n), 256, 0, s, coords, is_first, urow, n, cm.coords, unique_index);
  LGS_KLAUNCH(k_emit_sorted, nblk(n), 256, 0, s, skeys, svals, head, runid, urow, n, cm.skeys, cm.order);
  if (inverse) LGS_KLAUNCH(k_emit_inverse, nblk(n), 256, 0, s, svals, runid, cm.order, n, inverse);
  LGS_HIP(hipGetLastError());
  if (dfree_now(m, keys, s) || dfree_now(m, skeys, s) || dfree_now(m, vals, s) || dfree_now(m, svals, s) ||
      dfree_now(m, head, s) || dfree_now(m, runid, s) || dfree_now(m, is_first, s) || dfree_now(m, urow, s) || dfree_now(m, lvl_counts, s))
    return 1;
  m->maps.push_back(cm);
  *key = 0; *n_unique = nu;
  return publish(m, caller, true);   // unique_index / inverse live in caller memory; `coords` may be reused after this
}

int lgs_manager_stride2(lgs_manager *m, int in_key, void *stream, int *out_key, int64_t *n_out) {
  LGS_REQUIRE(m && out_key && n_out, "lgs_manager_stride2: null argument");
  LGS_REQUIRE(in_key >= 0 && in_key < (int)m->maps.size(), "lgs_manager_stride2: bad key");
  LGS_REQUIRE(!m->maps[in_key].origin, "lgs_manager_stride2: the origin map has no coarser map");
  hipStream_t s = m->ms;
  (void)stream;
  DeviceGuard guard(m->device);
  if (m->maps[in_key].coarse_key >= 0) {
    *out_key = m->maps[in_key].coarse_key; *n_out = m->maps[*out_key].n;
    return 0;
  }
  CoordMap f = m->maps[in_key];
  LGS_REQUIRE(f.log2ts < 12, "lgs_manager_stride2: tensor stride too large");
  CoordMap c;
  c.ts = f.ts * 2; c.log2ts = f.log2ts + 1; c.fine_key = in_key;
  int64_t n = f.n;
  if (n == 0) {
    m->maps.push_back(c);
    m->maps[in_key].coarse_key = (int)m->maps.size() - 1;
    *out_key = m->maps[in_key].coarse_key; *n_out = 0;
    return 0;
  }
  uint64_t keep = ~(7ull << (3 * f.log2ts));
  int32_t *head, *cincl;
  if (dalloc(m, &head, n, s) || dalloc(m, &cincl, n, s)) return 1;
  LGS_KLAUNCH(k_heads, nblk(n), 256, 0, s, f.skeys, n, keep, head);
  if (scan_incl(m, head, cincl, n, s)) return 1;
  int64_t nc;
  if (c.log2ts >= 1 && c.log2ts <= kPreLevels && m->precount[c.log2ts - 1] >= 0) {
    nc = m->precount[c.log2ts - 1];                 // counted by lgs_manager_insert: no host synchronisation here
  } else {
    int32_t h_nc = 0;
    LGS_HIP(hipMemcpyAsync(&h_nc, cincl + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    LGS_HIP(hipStreamSynchronize(s));
    nc = h_nc;
  }
  c.n = nc; c.n_pad = pad_rows(nc);
  if (dalloc(m, &c.coords, nc * 4, s) || dalloc(m, &c.skeys, nc, s) || dalloc(m, &c.cstart, nc + 1, s) ||
      dalloc(m, &c.fine_cidx, n, s))
    return 1;
  LGS_KLAUNCH(k_emit_coarse, nblk(n), 256, 0, s, f.skeys, head, cincl, n, keep, c.skeys, c.coords, c.cstart,
                     c.fine_cidx, nc, m->d_err);
  LGS_HIP(hipGetLastError());
  if (dfree_now(m, head, s) || dfree_now(m, cincl, s)) return 1;
  m->maps.push_back(c);
  int ck = (int)m->maps.size() - 1;
  m->maps[in_key].coarse_key = ck;
  *out_key = ck; *n_out = nc;
  return publish(m, nullptr, false);
}

int lgs_manager_check(lgs_manager *m, int *flags) {
  LGS_REQUIRE(m && flags, "lgs_manager_check: null argument");
  *flags = 0;
  if (!m->d_err) return 0;
  DeviceGuard guard(m->device);
  int h = 0;
  LGS_HIP(hipMemcpyAsync(&h, m->d_err, sizeof(int), hipMemcpyDeviceToHost, m->ms));
  LGS_HIP(hipStreamSynchronize(m->ms));
  *flags = h;
  return 0;
}

int lgs_manager_parent_of(lgs_manager *m, int key, int *fine_key) {
  LGS_REQUIRE(m && fine_key && key >= 0 && key < (int)m->maps.size(), "lgs_manager_parent_of: bad argument");
  *fine_key = m->maps[key].fine_key;
  return 0;
}

int lgs_manager_map_size(lgs_manager *m, int key, int64_t *n, int *tensor_stride) {
  LGS_REQUIRE(m && key >= 0 && key < (int)m->maps.size(), "lgs_manager_map_size: bad key");
  if (n) *n = m->maps[key].n;
  if (tensor_stride) *tensor_stride = m->maps[key].ts;
  return 0;
}

int lgs_manager_get_coords(lgs_manager *m, int key, int32_t *dst, void *stream) {
  LGS_REQUIRE(m && key >= 0 && key < (int)m->maps.size(), "lgs_manager_get_coords: bad key");
  const CoordMap &cm = m->maps[key];
  // `dst` was allocated on the caller's stream: a caching allocator may have handed out a block that kernels still
  // queued on that stream are using (e.g. a conv workspace released a moment ago), so the copy must be ordered after
  // the caller's pending work -- writing it early from the map stream corrupted a running conv's packed weights
  if (begin_from_caller(m, (hipStream_t)stream)) return 1;
  if (cm.n > 0)
    LGS_HIP(hipMemcpyAsync(dst, cm.coords, sizeof(int32_t) * 4 * (size_t)cm.n, hipMemcpyDeviceToDevice, m->ms));
  return publish(m, (hipStream_t)stream, true);
}

int lgs_manager_kernel_map(lgs_manager *m, int in_key, int out_key, int ks, void *stream, lgs_kmap **out) {
  (void)stream;
  return kernel_map(false, "lgs_manager_kernel_map", m, in_key, out_key, ks, 1, out);
}

int lgs_manager_kernel_map_ex(lgs_manager *m, int in_key, int out_key, int ks, int dilation, void *stream, lgs_kmap **out) {
  (void)stream;
  return kernel_map(true, "lgs_manager_kernel_map_ex", m, in_key, out_key, ks, dilation, out);
}

// what the two entry points above decide for a request given by plain facts, and what follows from it: no manager, no HIP call
int lgs_debug_kmap_relation(const lgs_kmap_relation_query *q, lgs_kmap_relation_info *out) {
  LGS_REQUIRE(q && out && (q->entry == 0 || q->entry == 1) && q->link >= 0 && q->link <= 3, "lgs_debug_kmap_relation: bad argument");
  *out = lgs_kmap_relation_info{};
  KmapRelation rel = kRelIdentity;
  const char *refusal = classify_kmap(KmapRequest{q->entry == 1, q->link == 0, q->link == 1, q->out_sorted != 0, q->in_origin || q->out_origin, q->ks,
                                                  q->dilation, q->tensor_stride}, rel);
  out->rc = refusal ? 2 : 0;
  out->relation = -1;
  LGS_REQUIRE(refusal == nullptr, refusal);
  const KmapTraits t = traits_of(rel);
  out->relation = rel; out->K = t.K; out->strided = t.strided; out->bwd_mirror = t.bwd_mirror; out->transposed_ok = t.transposed_ok;
  out->pairs_only[0] = t.wgrad_pairs_only(false); out->pairs_only[1] = t.wgrad_pairs_only(true);
  out->served_by_old_entry = t.old_entry;
  return 0;
}

// read-only: the tables of one view as they stand (exact-comparison tests of two build paths)
int lgs_debug_kmap_tables(lgs_kmap *km, int bwd, int32_t *nbr, int32_t *out_row, uint32_t *mask64, void *stream, int64_t *n_pad, int *slots,
                          int *present) {
  LGS_REQUIRE(km && n_pad && slots && present, "lgs_debug_kmap_tables: null argument");
  lgs_manager *m = km->mgr;
  const View &v = bwd ? km->bwd : km->fwd;
  *n_pad = v.n_pad; *slots = v.KS;
  *present = (v.nbr ? 1 : 0) | (v.out_row ? 2 : 0) | (v.mask64 ? 4 : 0);
  if (!nbr && !out_row && !mask64) return 0;
  hipStream_t caller = (hipStream_t)stream, s = m->ms;
  DeviceGuard guard(m->device);
  if (begin_from_caller(m, caller)) return 1;   // the output buffers were allocated on the caller's stream
  if (nbr && v.nbr && v.n_pad > 0) LGS_HIP(hipMemcpyAsync(nbr, v.nbr, sizeof(int32_t) * (size_t)(v.KS * v.n_pad), hipMemcpyDeviceToDevice, s));
  if (out_row && v.out_row && v.n_pad > 0) LGS_HIP(hipMemcpyAsync(out_row, v.out_row, sizeof(int32_t) * (size_t)v.n_pad, hipMemcpyDeviceToDevice, s));
  if (mask64 && v.mask64 && v.n_pad > 0) LGS_HIP(hipMemcpyAsync(mask64, v.mask64, sizeof(uint32_t) * (size_t)(v.n_pad / kGroup), hipMemcpyDeviceToDevice, s));
  return publish(m, caller, true);
}

int lgs_manager_origin(lgs_manager *m, void *stream, int *out_key, int64_t *n_out) {
  LGS_REQUIRE(m && out_key && n_out, "lgs_manager_origin: null argument");
  LGS_REQUIRE(!m->maps.empty(), "lgs_manager_origin: the manager holds no map yet");
  (void)stream;
  if (m->origin_key >= 0) {
    *out_key = m->origin_key; *n_out = m->maps[m->origin_key].n;
    return 0;
  }
  hipStream_t s = m->ms;
  DeviceGuard guard(m->device);
  const CoordMap f = m->maps[0];
  CoordMap o;
  o.ts = 0; o.log2ts = 0; o.origin = true;
  const int64_t n = f.n;
  const int64_t nb = n > 0 ? m->precount_batches : 0;   // counted by lgs_manager_insert: no host synchronisation here
  LGS_REQUIRE(nb >= 0, "lgs_manager_origin: batch count unknown");
  o.n = nb; o.n_pad = pad_rows(nb);
  if (n > 0) {
    int32_t *head, *cincl;
    if (dalloc(m, &o.coords, nb * 4, s) || dalloc(m, &head, n, s) || dalloc(m, &cincl, n, s)) return 1;
    if (batch_heads(m, f.skeys, n, head, cincl, s)) return 1;
    LGS_KLAUNCH(k_origin_coords, nblk(n), 256, 0, s, f.skeys, head, cincl, n, nb, o.coords, m->d_err);
    LGS_HIP(hipGetLastError());
    if (dfree_now(m, head, s) || dfree_now(m, cincl, s)) return 1;
  }
  m->maps.push_back(o);
  m->origin_key = (int)m->maps.size() - 1;
  *out_key = m->origin_key; *n_out = nb;
  return publish(m, nullptr, false);
}

int lgs_manager_segment_map(lgs_manager *m, int fine_key, int coarse_key, void *stream, lgs_segmap **out) {
  LGS_REQUIRE(m && out, "lgs_manager_segment_map: null argument");
  const int nm = (int)m->maps.size();
  LGS_REQUIRE(fine_key >= 0 && fine_key < nm && coarse_key >= 0 && coarse_key < nm, "lgs_manager_segment_map: bad key");
  LGS_REQUIRE(!m->maps[fine_key].origin, "lgs_manager_segment_map: the fine map is the origin map");
  for (lgs_segmap *k : m->segmaps)
    if (k->fine_key == fine_key && k->coarse_key == coarse_key) { *out = k; return 0; }
  (void)stream;
  const CoordMap &cf = m->maps[fine_key];
  const CoordMap &cc = m->maps[coarse_key];
  Chain ch;
  ch.k = 0;
  if (!cc.origin) {   // walk coarse -> fine through the maps stride2 made
    int levels[kMaxChain];
    int c = coarse_key;
    while (c != fine_key) {
      LGS_REQUIRE(c >= 0 && !m->maps[c].origin && ch.k < kMaxChain,
                  "lgs_manager_segment_map: the coarse map is neither the origin map nor a stride-2^k descendant of the fine map");
      levels[ch.k++] = c;
      c = m->maps[c].fine_key;
    }
    LGS_REQUIRE(ch.k >= 1, "lgs_manager_segment_map: fine and coarse map are the same map");
    for (int j = 0; j < ch.k; ++j) {           // levels[] runs coarse -> fine; the chain fine -> coarse
      const CoordMap &lv = m->maps[levels[ch.k - 1 - j]];
      ch.fine_cidx[j] = lv.fine_cidx;
      ch.cstart[j] = lv.cstart;
    }
  }
  hipStream_t s = m->ms;
  DeviceGuard guard(m->device);
  SegMap sm;
  sm.n_fine = cf.n; sm.n_coarse = cc.n;
  sm.fine_row = cf.order;
  sm.max_len = cc.origin ? 0 : (int64_t)1 << (3 * ch.k);
  const int64_t n = cf.n, nc = cc.n;
  if (n > 0) {
    if (cc.origin) {
      int32_t *head, *cincl, *seg_start, *coarse_of;
      if (dalloc(m, &seg_start, nc + 1, s) || dalloc(m, &coarse_of, n, s) || dalloc(m, &head, n, s) || dalloc(m, &cincl, n, s))
        return 1;
      if (batch_heads(m, cf.skeys, n, head, cincl, s)) return 1;
      LGS_KLAUNCH(k_origin_segments, nblk(n), 256, 0, s, head, cincl, n, nc, seg_start, coarse_of);
      LGS_HIP(hipGetLastError());
      if (dfree_now(m, head, s) || dfree_now(m, cincl, s)) return 1;
      sm.seg_start = seg_start; sm.coarse_of = coarse_of; sm.row_seg = coarse_of;
      if (cf.order) {   // level 0: rows are in the caller's order
        int32_t *row_seg;
        if (dalloc(m, &row_seg, n, s)) return 1;
        LGS_KLAUNCH(k_row_seg, nblk(n), 256, 0, s, cf.order, coarse_of, n, row_seg);
        LGS_HIP(hipGetLastError());
        sm.row_seg = row_seg;
      }
    } else if (ch.k == 1) {                    // one stride-2 step: its own arrays are the segment map
      sm.seg_start = ch.cstart[0]; sm.coarse_of = ch.fine_cidx[0];
    } else {
      int32_t *seg_start, *coarse_of;
      if (dalloc(m, &seg_start, nc + 1, s) || dalloc(m, &coarse_of, n, s)) return 1;
      LGS_KLAUNCH(k_compose_coarse_of, nblk(n), 256, 0, s, ch, n, coarse_of);
      LGS_KLAUNCH(k_compose_seg_start, nblk(nc + 1), 256, 0, s, ch, nc, seg_start);
      LGS_HIP(hipGetLastError());
      sm.seg_start = seg_start; sm.coarse_of = coarse_of;
    }
    if (!sm.single_pass()) {
      // at most n / kSegChunk + nc items: the tables are sized by that bound (no host synchronisation), unused slots -1
      const int64_t n_items = n / kSegChunk + nc + 1;
      int32_t *cnt, *item_start, *item_seg;
      if (dalloc(m, &item_start, nc + 1, s) || dalloc(m, &item_seg, n_items, s) || dalloc(m, &cnt, nc, s)) return 1;
      LGS_KLAUNCH(k_item_counts, nblk(nc), 256, 0, s, sm.seg_start, nc, cnt);
      LGS_HIP(hipMemsetAsync(item_start, 0, sizeof(int32_t), s));
      if (scan_incl(m, cnt, item_start + 1, nc, s)) return 1;
      LGS_KLAUNCH(k_fill_i32, nblk(n_items), 256, 0, s, item_seg, n_items, -1);
      LGS_KLAUNCH(k_item_fill, nblk(nc), 256, 0, s, item_start, nc, n_items, item_seg);
      LGS_HIP(hipGetLastError());
      if (dfree_now(m, cnt, s)) return 1;
      sm.item_start = item_start; sm.item_seg = item_seg; sm.n_items = n_items;
    }
  }
  lgs_segmap *h = new lgs_segmap();
  h->mgr = m; h->fine_key = fine_key; h->coarse_key = coarse_key; h->sm = sm;
  m->segmaps.push_back(h);
  *out = h;
  return publish(m, nullptr, false);
}

int lgs_kmap_export(lgs_kmap *km, int32_t *ek, int32_t *ein, int32_t *eout, void *stream, int64_t *mcount) {
  LGS_REQUIRE(km && mcount, "lgs_kmap_export: null argument");
  lgs_manager *m = km->mgr;
  hipStream_t caller = (hipStream_t)stream;
  hipStream_t s = m->ms;
  DeviceGuard guard(m->device);
  if (begin_from_caller(m, caller)) return 1;   // the output buffers were allocated on the caller's stream
  const View &v = km->fwd;
  int32_t *cnt;
  if (raw_alloc(m, (void **)&cnt, sizeof(int32_t), s)) return 1;
  LGS_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t), s));
  if (v.n_pad > 0) {
    if (ek) LGS_KLAUNCH(k_view_export, nblk(v.n_pad), 256, 0, s, v, cnt, ek, ein, eout);
    else LGS_KLAUNCH(k_view_count, nblk(v.n_pad), 256, 0, s, v, cnt);
  }
  int32_t h = 0;
  LGS_HIP(hipMemcpyAsync(&h, cnt, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  if (dfree_now(m, cnt, s)) return 1;
  *mcount = h;
  return publish(m, caller, true);
}

}  // extern "C"
