// lgs_keypack.h -- the engine's packed voxel key: a 10-bit batch field above three 18-bit coordinates in Morton order, and the hash
// of the open-addressing tables keyed by it (a slot is claimed by table_claim's probe sequence, lgs_idioms.h, from hash64(key) & (cap - 1)).
// Functions only, no kernels: lgs_mapkeys.h (the coordinate manager) and lgs_paste.hip (the per-instance voxel table) include it.
#pragma once
#include "lgs_common.h"

namespace lgs {

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

}  // namespace lgs
