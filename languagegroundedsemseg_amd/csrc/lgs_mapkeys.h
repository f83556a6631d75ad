// lgs_mapkeys.h -- the lookup tables over Morton keys (lgs_keypack.h), HashRef / DirRef and the kernels that fill them: k_hash_insert
// claims its slots through table_claim (lgs_idioms.h), k_dir_build walks the same bounded probe sequence spelled out; the find() loops
// are tuned for loads in flight and stay their own.
// Included by lgs_manager.hip only.
#pragma once
#include "lgs_common.h"
#include "lgs_keypack.h"

namespace lgs {

__global__ void k_hash_fill(uint64_t *hkeys, int64_t cap) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cap) hkeys[i] = kEmpty;
}
// one slot per key by table_claim (lgs_idioms.h; the keys are unique, so no slot is found already held).  The table holds at least
// twice the keys, so the probe sequence ends; a full table (impossible by that sizing) sets d_err bit 3 instead of spinning.
__global__ void k_hash_insert(const uint64_t *skeys, const int32_t *order, int64_t n, uint64_t *hkeys,
                              int32_t *hvals, uint64_t capm1, int *d_err) {
  int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint64_t key = skeys[p];
  const int64_t s = table_claim(hkeys, hash64(key) & capm1, capm1, key, kEmpty, capm1 + 1);
  if (s >= 0) hvals[s] = order ? order[p] : (int32_t)p;
  else if (d_err) atomicOr(d_err, 8);
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
// the entry with table_claim's probe sequence, spelled out: the kernel is on the training step's map-build stream, and through the
// helper (a stride of four words, an equality case that unique block ids never meet) it came out three instructions longer
// (profiles/device_idioms.md).  The table holds at least twice the block count; a full one sets d_err bit 3 instead of spinning.
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

}  // namespace lgs
