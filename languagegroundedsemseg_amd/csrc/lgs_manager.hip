// lgs_manager.hip -- coordinate manager + kernel-map construction for gfx950 (functionally MinkowskiEngine's CoordinateManager).
//
// Design: every coordinate is packed into ONE 64-bit Morton key
//   key = batch << 54 | interleave3(x + 2^17, y + 2^17, z + 2^17)
// Level-0 rows keep the caller's order, but every map also carries its rows in Morton order (`order`: sorted position -> row), so
// coarsening by 2 is a bit-mask on the key that preserves the sort, 3x3x3 maps are 27 probes per voxel into a table of the sorted keys
// (DirRef, or HashRef behind MAP_BLOCK_DIR = 0), and conv tiles are runs of 64 Morton-consecutive voxels with one offset mask each.
#include "lgs_common.h"

#include <cstring>   // rocprim.hpp calls memset without including it
#include <initializer_list>
#include <memory>
#include <tuple>
#include <rocprim/rocprim.hpp>

#include "lgs_arena.h"     // the arena's bump stack (host arithmetic, no HIP)
#include "lgs_mapkeys.h"   // Morton keys, HashRef / DirRef and their table kernels
#include "lgs_mapsort.h"   // window mask sort and row permutation kernels
#include "lgs_nearest.h"   // nearest-site query: ring search through the lookup table, exact scan for the rest

namespace lgs {

static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

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
  hipStream_t ms = nullptr;        // the map stream: all construction runs on it; consumers order themselves after `ev_ready` (lgs::kmap_wait)
  hipEvent_t ev_ready = nullptr, ev_in = nullptr;
  std::vector<hipStream_t> users;  // caller streams that consumed this manager's arrays (joined before freeing)
  std::vector<CoordMap> maps;
  std::vector<lgs_kmap *> kmaps;
  std::vector<void *> allocs;      // pool allocations (no arena yet, or the arena was too small)
  int *d_err = nullptr;
  char *arena = nullptr;           // one device block per manager, bump-allocated (see "arena" below)
  ArenaStack stack;                // where in the block each allocation lies (lgs_arena.h)
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

// what the managers of one device share for the whole process
struct ArenaBlock { char *base; size_t cap; std::vector<hipEvent_t> ready; };
struct DeviceState {
  hipMemPool_t pool = nullptr;      // the private stream-ordered pool (ensure_pool)
  hipStream_t map_stream = nullptr; // the one map stream (lgs_manager_create)
  std::vector<ArenaBlock> arenas;   // FIFO of released arena blocks
  size_t arena_need = 0;            // largest (arena peak + pool peak) any manager of this device has needed
} g_dev[64];

// The maps of step t+1 reuse step t's memory: map arrays come from a PRIVATE stream-ordered pool per device whose
// release threshold is unlimited (the process-wide default pool is left alone).
int ensure_pool(int device) {
  if (g_dev[device].pool) return 0;
  hipMemPoolProps props = {};
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
  g_dev[device].pool = pool;
  return 0;
}
// ---- arena ("Manager memory"): every manager owns ONE device block, bump-allocated on the host (ArenaStack); blocks are
// recycled through the device's FIFO.  Whatever does not fit (first step, growing scenes) falls back to the private stream-ordered pool.
int raw_alloc(lgs_manager *m, void **p, size_t bytes, hipStream_t s) {
  bytes = ArenaStack::rounded(bytes);
  size_t off = 0;
  if (m->arena && m->stack.take(bytes, &off)) {
    *p = m->arena + off;
    return 0;
  }
  LGS_HIP(hipMallocFromPoolAsync(p, bytes, m->pool, s));
  m->allocs.push_back(*p);
  m->pool_live += bytes;
  if (m->pool_live > m->pool_peak) m->pool_peak = m->pool_live;
  return 0;
}
template <typename T>
int dalloc(lgs_manager *m, T **p, int64_t count, hipStream_t s) {
  return raw_alloc(m, reinterpret_cast<void **>(p), sizeof(T) * (size_t)(count > 0 ? count : 1), s);
}
int dfree_now(lgs_manager *m, void *q, hipStream_t s) {  // temp buffer: release early
  char *c = reinterpret_cast<char *>(q);
  if (m->arena && c >= m->arena && c < m->arena + m->stack.capacity()) {
    m->stack.release((size_t)(c - m->arena));
    return 0;
  }
  for (size_t i = 0; i < m->allocs.size(); ++i)
    if (m->allocs[i] == q) { m->allocs[i] = m->allocs.back(); m->allocs.pop_back(); break; }
  LGS_HIP(hipFreeAsync(q, s));
  return 0;
}
// The temporaries of one entry point or builder ("the scratch-scope rule"): what is still held when the scope ends goes
// back, newest first, on every path out of it.  A fixed table, no heap: ~150 allocations per step pass through here on the host.
struct Scratch {
  lgs_manager *m;
  hipStream_t s;
  void *held[12];   // the largest scope, lgs_manager_insert, holds 9
  int n = 0;
  Scratch(lgs_manager *m_, hipStream_t s_) : m(m_), s(s_) {}
  Scratch(const Scratch &) = delete;
  ~Scratch() {      // (a failing hipFreeAsync of the pool fallback cannot be reported from here)
    while (n > 0)
      if (held[--n]) (void)dfree_now(m, held[n], s);
  }
  template <typename T>
  int take(T **p, int64_t count) {
    LGS_REQUIRE(n < 12, "Scratch: too many temporaries in one scope");
    if (dalloc(m, p, count, s)) return 1;
    held[n++] = *p;
    return 0;
  }
  int drop(void *p) {   // release one temporary before the scope ends
    for (int i = 0; i < n; ++i)
      if (held[i] == p) { held[i] = nullptr; return dfree_now(m, p, s); }
    return 0;
  }
};
// take a recycled block (or a new one) for a fresh manager; the map stream waits for the block's previous users
void arena_acquire(lgs_manager *m) {
  const int dev = m->device;
  const size_t need = g_dev[dev].arena_need;
  if (need == 0) return;                         // first manager of the device: measure through the pool
  std::vector<ArenaBlock> &q = g_dev[dev].arenas;
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
      m->arena = b.base; m->stack.reset(b.cap);
      return;
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
  if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return; }   // no block: this manager uses the pool
  m->arena = reinterpret_cast<char *>(p); m->stack.reset(cap);
}
void arena_release(lgs_manager *m) {
  DeviceState &d = g_dev[m->device];
  const size_t need = m->stack.peak() + m->pool_peak;
  if (need > d.arena_need) d.arena_need = need;
  if (!m->arena) return;
  ArenaBlock b{m->arena, m->stack.capacity(), {}};
  std::vector<hipStream_t> streams = m->users;
  streams.push_back(m->ms);
  for (hipStream_t u : streams) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess) {
      if (hipEventRecord(e, u) == hipSuccess) b.ready.push_back(e); else (void)hipEventDestroy(e);
    }
  }
  d.arenas.push_back(b);
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
// order `stream` after the published map work; it becomes a user of the manager's arrays
int wait_ready(lgs_manager *m, hipStream_t stream) {
  LGS_HIP(hipStreamWaitEvent(stream, m->ev_ready, 0));
  add_user(m, stream);
  return 0;
}
// publish map work; if `caller` is given it is ordered after it (outputs written into caller-owned memory)
int publish(lgs_manager *m, hipStream_t caller, bool caller_waits) {
  LGS_HIP(hipEventRecord(m->ev_ready, m->ms));
  return caller_waits ? wait_ready(m, caller) : 0;
}
inline unsigned nblk(int64_t n, int t = 256) { return (unsigned)((n + t - 1) / t > 0 ? (n + t - 1) / t : 1); }

int ensure_hash(lgs_manager *m, CoordMap &cm, hipStream_t s) {
  if (cm.hkeys) return 0;
  const int64_t cap = table_pow2(1024, 2 * cm.n);
  cm.hcap = cap;
  if (dalloc(m, &cm.hkeys, cap, s)) return 1;
  if (dalloc(m, &cm.hvals, cap, s)) return 1;
  LGS_KLAUNCH(k_hash_fill, nblk(cap), 256, 0, s, cm.hkeys, cap);
  if (cm.n > 0)
    LGS_KLAUNCH(k_hash_insert, nblk(cm.n), 256, 0, s, cm.skeys, cm.order, cm.n, cm.hkeys, cm.hvals, (uint64_t)(cap - 1), m->d_err);
  LGS_HIP(hipGetLastError());
  return 0;
}

// the block directory of a map (MAP_BLOCK_DIR; DESIGN.md, "Neighbour lookup"): sized from the insert's count of the map two levels coarser, else from n
int ensure_dir(lgs_manager *m, CoordMap &cm, hipStream_t s) {
  if (cm.dir) return 0;
  int64_t blocks = cm.n;
  const int lv = cm.log2ts + 2;
  if (lv <= kPreLevels && m->precount[lv - 1] >= 0 && m->precount[lv - 1] < blocks) blocks = m->precount[lv - 1];
  const int64_t cap = table_pow2(1024, 2 * blocks);
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
  Scratch tmp(m, s);   // rocPRIM's temporary: from and back to the arena's top
  char *t;
  if (tmp.take(&t, (int64_t)(tb ? tb : 16))) return 1;
  LGS_HIP(rocprim::inclusive_scan(t, tb, in, out, (size_t)n, rocprim::plus<int32_t>(), s));
  return 0;
}

// radix sort of (key, value) pairs on key bits [begin_bit, end_bit)
template <typename K, typename V>
int sort_pairs(lgs_manager *m, K *keys, K *keys_out, V *vals, V *vals_out, int64_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  size_t tb = 0;
  LGS_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys, keys_out, vals, vals_out, (size_t)n, begin_bit, end_bit, s));
  Scratch tmp(m, s);
  char *t;
  if (tmp.take(&t, (int64_t)(tb ? tb : 16))) return 1;
  LGS_HIP(rocprim::radix_sort_pairs(t, tb, keys, keys_out, vals, vals_out, (size_t)n, begin_bit, end_bit, s));
  return 0;
}

// head[p] = 1 where sorted key p starts a new run of (key & keep_mask); incl = its inclusive scan (the run of every position, + 1)
constexpr uint64_t kBatchMask = ~((1ull << kBatchShift) - 1);   // runs of one batch index: the rows of the origin map
int key_heads(lgs_manager *m, const uint64_t *skeys, int64_t n, uint64_t keep_mask, int32_t *head, int32_t *incl, hipStream_t s) {
  LGS_KLAUNCH(k_heads, nblk(n), 256, 0, s, skeys, n, keep_mask, head);
  return scan_incl(m, head, incl, n, s);
}

// the window mask sort of a 27-slot table (pmask) -> perm: position q of the view is sorted position perm[q].  MAP_WINDOW_SORT: one
// k_window_sort launch where the window fits the LDS (window_sort_log2); else the radix sort of (window, code) keys and its temporaries
int window_perm(lgs_manager *m, int64_t n, int64_t n_pad, const uint32_t *pmask, int32_t *perm, hipStream_t s) {
  const int64_t window = tune(T_MASK_WINDOW);   // tuning knob (default kMaskWindow)
  const int order = (int)tune(T_MASK_ORDER);
  const int log2w = tune(T_MAP_WINDOW_SORT) != 0 ? window_sort_log2(window) : -1;
  if (log2w >= 0) {
    static const hipError_t lds_attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_window_sort), hipFuncAttributeMaxDynamicSharedMemorySize, (int)window_sort_lds(kWsMaxLog2));
    LGS_HIP(lds_attr);   // once per process
    // a map of one window sorts the smallest power of two that holds its positions (what lies beyond is padding, which sorts last)
    int l = log2w;
    while (l > kWsMinLog2 && n_pad <= (1ll << (l - 1))) --l;
    LGS_KLAUNCH(k_window_sort, (unsigned)((n_pad + (1ll << l) - 1) >> l), 1u << (l - 4), window_sort_lds(l), s, pmask, n, n_pad, l, order, perm);
    return 0;
  }
  Scratch tmp(m, s);
  uint64_t *keys, *skeys2; int32_t *vals;
  if (tmp.take(&keys, n_pad) || tmp.take(&skeys2, n_pad) || tmp.take(&vals, n_pad)) return 1;
  LGS_KLAUNCH(k_mask_sort_keys, (unsigned)(n_pad / 256), 256, 0, s, pmask, n, n_pad, (int)window, order, keys, vals);
  return sort_pairs(m, keys, skeys2, vals, perm, n_pad, 0, mask_sort_bits(n_pad, (int)window), s);
}

// the permutation of (nbr_tmp, pmask) into the view's arrays.  MAP_PERMUTE_LDS: through LDS (k_permute_map3_lds) where a window's
// row segment fits it and windows are whole groups of 256 positions; else, and with the knob at 0, k_permute_map3
// Offsets per workgroup (MAP_PERMUTE_GROUP): as many as still leave the grid above kPlWorkgroups
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
  static const hipError_t lds16 = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_permute_map3_lds<16>), hipFuncAttributeMaxDynamicSharedMemorySize, 16 * kPlThreads * 4);
  static const hipError_t lds32 = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_permute_map3_lds<32>), hipFuncAttributeMaxDynamicSharedMemorySize, kPlMaxWindow * 4);
  LGS_HIP(lds16 != hipSuccess ? lds16 : lds32);   // once per process
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
  v = View(27, 27, st.n_pad, st.n, n_in);
  if (st.n == 0) return 0;
  int32_t *nbr, *orow, *nbr_tmp, *perm; uint32_t *mask, *pmask;
  if (dalloc(m, &nbr, 27 * st.n_pad, s) || dalloc(m, &mask, st.n_pad / kGroup, s) || dalloc(m, &orow, st.n_pad, s)) return 1;
  Scratch tmp(m, s);   // above the view's own arrays: they pop
  if (tmp.take(&nbr_tmp, 27 * st.n_pad) || tmp.take(&pmask, st.n_pad) || tmp.take(&perm, st.n_pad)) return 1;
  if (build(nbr_tmp, pmask)) return 1;
  if (window_perm(m, st.n, st.n_pad, pmask, perm, s)) return 1;
  if (permute_rows(st, nbr_tmp, pmask, perm, s, nbr, orow, mask)) return 1;
  LGS_HIP(hipGetLastError());
  v.nbr = nbr; v.mask64 = mask; v.out_row = orow;
  return 0;
}

// ---- kernel maps: one builder per relation (KmapRelation, lgs_common.h), all on the map stream
// identity 1x1: no table
void build_identity(const CoordMap &ci, lgs_kmap *km) { km->fwd = km->bwd = View(1, 1, ci.n_pad, ci.n, ci.n); }

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
  if (probe_view27(m, ci, ci, dilation * ci.ts, s, km->fwd)) return 1;
  km->bwd = km->fwd; km->bwd.mirror = 1;
  return 0;
}

// MAP_OWN_SORTS: rounds of 256 positions per workgroup of k_child_hist / k_child_scatter (MAP_CHILD_ROUNDS): as many as
// still leave kCpWorkgroups workgroups
constexpr int kCpWorkgroups = 512;
inline int child_rounds(int64_t n) {
  const int64_t k = tune(T_MAP_CHILD_ROUNDS);
  if (k >= 1) return (int)(k > kCpMaxRounds ? kCpMaxRounds : k);
  const int64_t r = (n + 255) / 256 / kCpWorkgroups;
  return (int)(r < 1 ? 1 : (r > kCpMaxRounds ? kCpMaxRounds : r));
}

// 2^3 stride 2: the children of a coarse row are one run of the fine Morton order
int build_conv2_s2(lgs_manager *m, const CoordMap &ci, const CoordMap &co, hipStream_t s, lgs_kmap *km) {
  const int shift = 3 * ci.log2ts;
  const int64_t n = ci.n, gp = n > 0 ? pad_rows(n + 8 * kPadRows) : 0;   // rows of the grouped fine view
  View vf = View(8, 8, co.n_pad, co.n, n), vb = View(1, 8, gp, n, co.n);
  if (n > 0) {
    int32_t *nbr8, *g_nbr, *g_out, *tile_k; uint32_t *mask;
    if (dalloc(m, &nbr8, 8 * co.n_pad, s) || dalloc(m, &mask, co.n_pad / kGroup, s)) return 1;
    LGS_KLAUNCH(k_build_map2_coarse, (unsigned)(co.n_pad / 256), 256, 0, s, ci.skeys, ci.order, co.cstart, co.n, co.n_pad, shift, nbr8, mask);
    // grouped fine view: the tables, all -1, and the radix path's child counters, zeroed by the same launch (MAP_OWN_SORTS = 1: cnt is
    // nullptr and its segment has count 0, which IS the zero-initialised fourth slot of FillSegs: the launch is the three-segment one)
    if (dalloc(m, &g_nbr, gp, s) || dalloc(m, &g_out, gp, s) || dalloc(m, &tile_k, gp / kGroup, s)) return 1;
    const bool own = tune(T_MAP_OWN_SORTS) != 0;
    Scratch tmp(m, s);
    int32_t *cnt = nullptr, *goff, *gsrc;
    if (!own && tmp.take(&cnt, 8)) return 1;
    if (fill_segs(s, {{g_nbr, gp, -1}, {g_out, gp, -1}, {tile_k, gp / kGroup, -1}, {cnt, own ? 0 : 8, 0}})) return 1;
    if (own) {   // the stable 8-way partition (k_child_hist)
      const int rounds = child_rounds(n);
      const int32_t nwg = (int32_t)((n + 256 * rounds - 1) / (256 * rounds));
      int32_t *wg;
      if (tmp.take(&wg, 8 * (int64_t)nwg) || tmp.take(&goff, 9) || tmp.take(&gsrc, 9)) return 1;
      LGS_KLAUNCH(k_child_hist, (unsigned)nwg, 256, 0, s, ci.skeys, n, shift, rounds, nwg, wg);
      LGS_KLAUNCH(k_child_prefix, 1, 512, 0, s, wg, nwg, goff, gsrc);
      LGS_KLAUNCH(k_child_scatter, (unsigned)nwg, 256, 0, s, ci.skeys, n, shift, rounds, nwg, wg, goff, co.fine_cidx, ci.order, g_nbr, g_out, tile_k);
    } else {     // (child, position) pairs through the radix sort
      uint32_t *kk, *kks; int32_t *pp, *pps;
      if (tmp.take(&kk, n) || tmp.take(&kks, n) || tmp.take(&pp, n) || tmp.take(&pps, n) || tmp.take(&goff, 9) || tmp.take(&gsrc, 9)) return 1;
      LGS_KLAUNCH(k_child_keys, nblk(n), 256, 0, s, ci.skeys, n, shift, kk, pp, cnt);
      if (sort_pairs(m, kk, kks, pp, pps, n, 0, 3, s)) return 1;
      LGS_KLAUNCH(k_group_offsets, 1, 64, 0, s, cnt, goff, gsrc);
      LGS_KLAUNCH(k_build_map2_fine, nblk(n), 256, 0, s, kks, pps, n, goff, gsrc, co.fine_cidx, ci.order, g_nbr, g_out, tile_k);
    }
    LGS_HIP(hipGetLastError());
    vf.nbr = nbr8; vf.mask64 = mask;
    vb.nbr = g_nbr; vb.out_row = g_out; vb.tile_k = tile_k;
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
  View vf = View(1, 1, co.n_pad, co.n, ci.n), vb = View(1, 1, ci.n_pad, ci.n, co.n);
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

// ---- segment maps (lgs_manager_segment_map): one construction per kind of coarse map, then the chunk items; sm carries the row counts
// the origin map over the fine map `cf`: one run of sorted positions per batch index
int seg_origin(lgs_manager *m, const CoordMap &cf, hipStream_t s, SegMap &sm) {
  const int64_t n = sm.n_fine, nc = sm.n_coarse;
  Scratch tmp(m, s);
  int32_t *head, *cincl, *seg_start, *coarse_of;
  if (dalloc(m, &seg_start, nc + 1, s) || dalloc(m, &coarse_of, n, s) || tmp.take(&head, n) || tmp.take(&cincl, n)) return 1;
  if (key_heads(m, cf.skeys, n, kBatchMask, head, cincl, s)) return 1;
  LGS_KLAUNCH(k_origin_segments, nblk(n), 256, 0, s, head, cincl, n, nc, seg_start, coarse_of);
  LGS_HIP(hipGetLastError());
  if (tmp.drop(head) || tmp.drop(cincl)) return 1;   // row_seg takes their place
  sm.seg_start = seg_start; sm.coarse_of = coarse_of; sm.row_seg = coarse_of;
  if (cf.order) {   // level 0: rows are in the caller's order
    int32_t *row_seg;
    if (dalloc(m, &row_seg, n, s)) return 1;
    LGS_KLAUNCH(k_row_seg, nblk(n), 256, 0, s, cf.order, coarse_of, n, row_seg);
    LGS_HIP(hipGetLastError());
    sm.row_seg = row_seg;
  }
  return 0;
}
// a stride-2^k descendant, k >= 2: the chain's steps composed
int seg_composed(lgs_manager *m, const Chain &ch, hipStream_t s, SegMap &sm) {
  const int64_t n = sm.n_fine, nc = sm.n_coarse;
  int32_t *seg_start, *coarse_of;
  if (dalloc(m, &seg_start, nc + 1, s) || dalloc(m, &coarse_of, n, s)) return 1;
  LGS_KLAUNCH(k_compose_coarse_of, nblk(n), 256, 0, s, ch, n, coarse_of);
  LGS_KLAUNCH(k_compose_seg_start, nblk(nc + 1), 256, 0, s, ch, nc, seg_start);
  LGS_HIP(hipGetLastError());
  sm.seg_start = seg_start; sm.coarse_of = coarse_of;
  return 0;
}
// the chunk items of a two-pass map: at most n / kSegChunk + nc, the tables are sized by that bound (no host synchronisation), unused slots -1
int seg_chunk_items(lgs_manager *m, hipStream_t s, SegMap &sm) {
  const int64_t nc = sm.n_coarse, n_items = sm.n_fine / kSegChunk + nc + 1;
  Scratch tmp(m, s);
  int32_t *cnt, *item_start, *item_seg;
  if (dalloc(m, &item_start, nc + 1, s) || dalloc(m, &item_seg, n_items, s) || tmp.take(&cnt, nc)) return 1;
  LGS_KLAUNCH(k_item_counts, nblk(nc), 256, 0, s, sm.seg_start, nc, cnt);
  LGS_HIP(hipMemsetAsync(item_start, 0, sizeof(int32_t), s));
  if (scan_incl(m, cnt, item_start + 1, nc, s)) return 1;
  LGS_KLAUNCH(k_fill_i32, nblk(n_items), 256, 0, s, item_seg, n_items, -1);
  LGS_KLAUNCH(k_item_fill, nblk(nc), 256, 0, s, item_start, nc, n_items, item_seg);
  LGS_HIP(hipGetLastError());
  sm.item_start = item_start; sm.item_seg = item_seg; sm.n_items = n_items;
  return 0;
}
}  // namespace

namespace lgs {
int kmap_wait(lgs_kmap *km, hipStream_t stream) { return wait_ready(km->mgr, stream); }
int segmap_wait(lgs_segmap *sm, hipStream_t stream) { return wait_ready(sm->mgr, stream); }
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
  DeviceState &d = g_dev[device];
  m->pool = d.pool;
  // one map stream per device for the whole process: managers of consecutive steps simply queue behind each other on it
  if (!d.map_stream) LGS_HIP(hipStreamCreateWithFlags(&d.map_stream, hipStreamNonBlocking));
  m->ms = d.map_stream;
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
  hipStream_t caller = (hipStream_t)stream, s = m->ms;
  DeviceGuard guard(m->device);
  if (begin_from_caller(m, caller)) return 1;   // `coords` was produced on the caller's stream
  CoordMap cm;
  if (n == 0) {
    m->maps.push_back(cm);
    *key = 0; *n_unique = 0;
    return 0;
  }
  if (!m->d_err) { if (dalloc(m, &m->d_err, 1, s)) return 1; }
  Scratch tmp(m, s);   // UNDER the map's own arrays, which are sized only after the host synchronisation: their room stays a hole
  uint64_t *keys, *skeys; int32_t *vals, *svals, *head, *runid, *is_first, *urow, *lvl_counts;
  if (tmp.take(&lvl_counts, kPreLevels + 1) || tmp.take(&keys, n) || tmp.take(&skeys, n) || tmp.take(&vals, n) || tmp.take(&svals, n) ||
      tmp.take(&head, n) || tmp.take(&runid, n) || tmp.take(&is_first, n) || tmp.take(&urow, n + 1))
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
  m->maps.push_back(cm);
  *key = 0; *n_unique = nu;
  return publish(m, caller, true);   // unique_index / inverse live in caller memory; `coords` may be reused after this
}

int lgs_manager_stride2(lgs_manager *m, int in_key, void *, int *out_key, int64_t *n_out) {
  LGS_REQUIRE(m && out_key && n_out, "lgs_manager_stride2: null argument");
  LGS_REQUIRE(in_key >= 0 && in_key < (int)m->maps.size(), "lgs_manager_stride2: bad key");
  LGS_REQUIRE(!m->maps[in_key].origin, "lgs_manager_stride2: the origin map has no coarser map");
  hipStream_t s = m->ms;
  DeviceGuard guard(m->device);
  if (m->maps[in_key].coarse_key >= 0) {
    *out_key = m->maps[in_key].coarse_key; *n_out = m->maps[*out_key].n;
    return 0;
  }
  CoordMap f = m->maps[in_key];
  LGS_REQUIRE(f.log2ts < 12, "lgs_manager_stride2: tensor stride too large");
  CoordMap c;
  c.ts = f.ts * 2; c.log2ts = f.log2ts + 1; c.fine_key = in_key;
  const int64_t n = f.n;
  auto add = [&]() {   // c becomes in_key's coarse map
    m->maps.push_back(c);
    *out_key = m->maps[in_key].coarse_key = (int)m->maps.size() - 1;
    *n_out = c.n;
  };
  if (n == 0) { add(); return 0; }
  uint64_t keep = ~(7ull << (3 * f.log2ts));
  Scratch tmp(m, s);   // under the coarse map's arrays, as in the insert
  int32_t *head, *cincl;
  if (tmp.take(&head, n) || tmp.take(&cincl, n)) return 1;
  if (key_heads(m, f.skeys, n, keep, head, cincl, s)) return 1;
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
  add();
  return publish(m, nullptr, false);
}

int lgs_manager_check(lgs_manager *m, int *flags) {
  LGS_REQUIRE(m && flags, "lgs_manager_check: null argument");
  *flags = 0;
  if (!m->d_err) return 0;
  DeviceGuard guard(m->device);
  LGS_HIP(hipMemcpyAsync(flags, m->d_err, sizeof(int), hipMemcpyDeviceToHost, m->ms));
  LGS_HIP(hipStreamSynchronize(m->ms));
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

// Nearest site of map `key` for m points (lgs_nearest.h).  Runs on the map stream, between the caller's pending work and its later
// work, like lgs_manager_get_coords: the lookup table may have to be built there, and the leftover list is scoped scratch of the arena,
// whose reuse is ordered by that stream alone.  No host synchronisation: the exact scan is launched with a fixed grid and reads the
// list's length on the device.
int lgs_manager_nearest(lgs_manager *m, int key, const float *points, int64_t mq, const int64_t *scene_offsets, int b, int batch_base,
                        const double *affines, double anchor, int64_t *rows, float *d2, void *stream) {
  LGS_REQUIRE(m != nullptr, "lgs_manager_nearest: null argument");
  LGS_REQUIRE(key >= 0 && key < (int)m->maps.size(), "lgs_manager_nearest: bad key");
  LGS_REQUIRE(!m->maps[key].origin, "lgs_manager_nearest: the origin map has no sites to search");
  LGS_REQUIRE(mq >= 0 && mq < (1ll << 31) - 1024, "lgs_manager_nearest: point count out of range");
  LGS_REQUIRE(mq == 0 || (points && scene_offsets && rows), "lgs_manager_nearest: null argument");   // no points: nothing is read or written
  LGS_REQUIRE(b >= 1 && b <= kNearestScenes, "lgs_manager_nearest: 1 <= b <= LGS_AUG_MAX_SCENES");
  LGS_REQUIRE(batch_base >= 0 && batch_base + b <= 1024, "lgs_manager_nearest: batch index out of range");
  LGS_REQUIRE(anchor == anchor && anchor - anchor == 0.0, "lgs_manager_nearest: anchor must be finite");
  if (mq == 0) return 0;
  hipStream_t caller = (hipStream_t)stream, s = m->ms;
  DeviceGuard guard(m->device);
  if (begin_from_caller(m, caller)) return 1;   // points, scene_offsets and the outputs belong to the caller's stream
  CoordMap &cm = m->maps[key];
  if (cm.n == 0) {
    LGS_KLAUNCH(k_nearest_none, nblk(mq), 256, 0, s, mq, rows, d2);
    LGS_HIP(hipGetLastError());
    return publish(m, caller, true);
  }
  if (ensure_lookup(m, cm, s)) return 1;
  NearestArgs q = {points, scene_offsets, mq, b, affines ? 1 : 0, batch_base, cm.log2ts, 1.0 / (double)cm.ts, anchor};
  NearestAffines A = {};
  if (affines) std::memcpy(&A, affines, sizeof(double) * 12 * (size_t)b);
  int64_t ring = tune(T_NEAREST_MAX_RING);
  ring = ring < 0 ? 0 : (ring > 64 ? 64 : ring);
  Scratch tmp(m, s);
  int32_t *left, *n_left;
  if (tmp.take(&n_left, 1) || tmp.take(&left, mq)) return 1;
  LGS_HIP(hipMemsetAsync(n_left, 0, sizeof(int32_t), s));
  if (use_block_dir())
    LGS_KLAUNCH(k_nearest_ring<DirRef>, nblk(mq), 256, 0, s, q, A, dir_ref(cm), (int)ring, rows, d2, left, n_left);
  else
    LGS_KLAUNCH(k_nearest_ring<HashRef>, nblk(mq), 256, 0, s, q, A, hash_ref(cm), (int)ring, rows, d2, left, n_left);
  LGS_KLAUNCH(k_nearest_scan, kNearestScanGrid, 256, 0, s, q, A, cm.skeys, cm.order, cm.n, left, n_left, rows, d2);
  LGS_HIP(hipGetLastError());
  return publish(m, caller, true);
}

int lgs_manager_kernel_map(lgs_manager *m, int in_key, int out_key, int ks, void *, lgs_kmap **out) {
  return kernel_map(false, "lgs_manager_kernel_map", m, in_key, out_key, ks, 1, out);
}

int lgs_manager_kernel_map_ex(lgs_manager *m, int in_key, int out_key, int ks, int dilation, void *, lgs_kmap **out) {
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

int lgs_manager_origin(lgs_manager *m, void *, int *out_key, int64_t *n_out) {
  LGS_REQUIRE(m && out_key && n_out, "lgs_manager_origin: null argument");
  LGS_REQUIRE(!m->maps.empty(), "lgs_manager_origin: the manager holds no map yet");
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
    Scratch tmp(m, s);
    int32_t *head, *cincl;
    if (dalloc(m, &o.coords, nb * 4, s) || tmp.take(&head, n) || tmp.take(&cincl, n)) return 1;
    if (key_heads(m, f.skeys, n, kBatchMask, head, cincl, s)) return 1;
    LGS_KLAUNCH(k_origin_coords, nblk(n), 256, 0, s, f.skeys, head, cincl, n, nb, o.coords, m->d_err);
    LGS_HIP(hipGetLastError());
  }
  m->maps.push_back(o);
  m->origin_key = (int)m->maps.size() - 1;
  *out_key = m->origin_key; *n_out = nb;
  return publish(m, nullptr, false);
}

int lgs_manager_segment_map(lgs_manager *m, int fine_key, int coarse_key, void *, lgs_segmap **out) {
  LGS_REQUIRE(m && out, "lgs_manager_segment_map: null argument");
  const int nm = (int)m->maps.size();
  LGS_REQUIRE(fine_key >= 0 && fine_key < nm && coarse_key >= 0 && coarse_key < nm, "lgs_manager_segment_map: bad key");
  LGS_REQUIRE(!m->maps[fine_key].origin, "lgs_manager_segment_map: the fine map is the origin map");
  for (lgs_segmap *k : m->segmaps)
    if (k->fine_key == fine_key && k->coarse_key == coarse_key) { *out = k; return 0; }
  const CoordMap &cf = m->maps[fine_key], &cc = m->maps[coarse_key];
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
  if (cf.n > 0) {
    if (!cc.origin && ch.k == 1) {             // one stride-2 step: its own arrays are the segment map
      sm.seg_start = ch.cstart[0]; sm.coarse_of = ch.fine_cidx[0];
    } else if (cc.origin ? seg_origin(m, cf, s, sm) : seg_composed(m, ch, s, sm)) return 1;
    if (!sm.single_pass() && seg_chunk_items(m, s, sm)) return 1;
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
  hipStream_t caller = (hipStream_t)stream, s = m->ms;
  DeviceGuard guard(m->device);
  if (begin_from_caller(m, caller)) return 1;   // the output buffers were allocated on the caller's stream
  const View &v = km->fwd;
  Scratch tmp(m, s);
  int32_t *cnt;
  if (tmp.take(&cnt, 1)) return 1;
  LGS_HIP(hipMemsetAsync(cnt, 0, sizeof(int32_t), s));
  if (v.n_pad > 0) {
    if (ek) LGS_KLAUNCH(k_view_export, nblk(v.n_pad), 256, 0, s, v, cnt, ek, ein, eout);
    else LGS_KLAUNCH(k_view_count, nblk(v.n_pad), 256, 0, s, v, cnt);
  }
  int32_t h = 0;
  LGS_HIP(hipMemcpyAsync(&h, cnt, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LGS_HIP(hipStreamSynchronize(s));
  *mcount = h;
  return publish(m, caller, true);
}

}  // extern "C"
