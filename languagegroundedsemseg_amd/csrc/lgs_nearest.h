// lgs_nearest.h -- nearest-site query over a coordinate map's lookup table (DirRef / HashRef).  Included by lgs_manager.hip only.
//
// THE SITE FRAME (the contract of lgs_manager_nearest, DESIGN.md section 4, tests/test_gpu_nearest.py).  The sites of the probed map are
// the integer lattice points c / ts (ts = the map's tensor stride).  A point q of scene s becomes, in double, p = (A_s (q, 1)) / ts - anchor
// (A_s evaluated as k_voxelize does: ((x a0 + y a1) + z a2) + a3, every step rounded; the identity without affines).  Its home cell is
// h = rint(p), its fraction f = p - h is formed once in double and rounded to fp32 ONCE.  The squared distance to the site at integer
// offset k from h is
//     d2 = ((f.x - k.x)^2 + (f.y - k.y)^2) + (f.z - k.z)^2        in fp32, every operation rounded to nearest, in exactly this order
// (site_d2 below: both stages call it, so they agree bit for bit).  The answer is the minimum of (d2, row) in lexicographic order:
// among equal d2 the smallest ROW INDEX wins, not the smallest sorted position.
//
// Stage A (k_nearest_ring), one query per lane: rings r = 0, 1, ... NEAREST_MAX_RING of cells at Chebyshev distance r from h.  |f| <= 1/2
// on every axis, so a site at Chebyshev distance k is at |f - k| >= k - 1/2 on one axis, and because fp32 subtraction, squaring and the
// additions of non-negative terms are monotonic and (r + 1/2)^2 is an fp32 number, every site NOT visited after ring r has a computed
// d2 >= (r + 1/2)^2.  A query is finished after ring r when best d2 < (r + 1/2)^2.  The comparison is strict: at d2 == (r + 1/2)^2 exactly
// (a point on a cell face) a site of ring r + 1 can tie, and the tie rule may prefer it.  What is not finished after the last ring, and
// what has its home cell outside the key range, is appended to a list.
// Stage B (k_nearest_scan), one workgroup per listed query: the exact scan of the scene's run of sorted keys (the batch index is the
// top key field, so the run is contiguous), same d2, same tie rule, minimum over the wave and then the workgroup.
// Every loop is bounded before it starts: rings by the knob, blocks and cells of a ring by its size, bits of an occupancy word by 64,
// probe sequences as in DirRef::find / HashRef::find (tables at most half full), binary searches by their halving, the scan by the run length.
#pragma once
#include "lgs_mapkeys.h"

namespace lgs {

constexpr int kNearestScenes = LGS_AUG_MAX_SCENES;   // affines travel as a by-value table, as in k_voxelize_batched
constexpr int kNearestScanGrid = 1024;               // workgroups of k_nearest_scan: fixed, the list length is read on the device
constexpr int kSceneShift = 54;                      // pack_key's batch field: the keys of one batch index are one run of the sort
struct NearestAffines { double a[kNearestScenes][12]; };
struct NearestArgs {
  const float *pts;       // [m, 3]
  const int64_t *off;     // [b + 1] scene offsets (device)
  int64_t m;
  int b, has_affine, batch_base, log2ts;
  double inv_ts, anchor;  // 1 / ts is exact: ts is a power of two
};

struct SiteQuery {
  double h[3];   // home cell (an integer, kept in double: it may lie far outside the key range)
  float f[3];    // p - h, rounded once
  int scene;
  bool finite;
};
struct Best { float d2; int32_t row; };

__device__ inline int nearest_scene_of(const int64_t *__restrict__ off, int b, int64_t i) { return last_not_above(off, 1, b, i); }
__device__ inline SiteQuery site_query(const NearestArgs &q, const NearestAffines &A, int64_t i) {
  SiteQuery o;
  o.scene = nearest_scene_of(q.off, q.b, i);
  const double x = (double)q.pts[3 * i], y = (double)q.pts[3 * i + 1], z = (double)q.pts[3 * i + 2];
  o.finite = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double v = r == 0 ? x : (r == 1 ? y : z);
    if (q.has_affine) v = affine_row(A.a[o.scene] + 4 * r, x, y, z);
    const double p = __dsub_rn(__dmul_rn(v, q.inv_ts), q.anchor);
    o.finite = o.finite && isfinite(p);
    o.h[r] = rint(p);
    o.f[r] = (float)__dsub_rn(p, o.h[r]);
  }
  return o;
}
__device__ inline float site_d2(const float (&f)[3], float kx, float ky, float kz) {
  const float dx = __fsub_rn(f[0], kx), dy = __fsub_rn(f[1], ky), dz = __fsub_rn(f[2], kz);
  return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}
__device__ inline void best_take(Best &b, float d2, int32_t row) {
  if (d2 < b.d2 || (d2 == b.d2 && (b.row < 0 || row < b.row))) { b.d2 = d2; b.row = row; }
}
__device__ inline bool ring_done(const Best &b, int r) {
  const float e = (float)r + 0.5f;
  return b.d2 < e * e;
}

// ---- stage A with the block directory.  The cells of a 4 x 4 x 4 block are numbered by 6 Morton bits (x0 y0 z0 x1 y1 z1); the cells of
// the block with local coordinate lo .. hi on one axis are a fixed 64-bit pattern, a cube is the AND of three of them.
template <int AXIS>
__device__ inline uint64_t axis_mask(int lo, int hi) {
  constexpr uint64_t m0 = AXIS == 0 ? 0x5555555555555555ull : (AXIS == 1 ? 0x3333333333333333ull : 0x0f0f0f0f0f0f0f0full);   // cell bit AXIS clear
  constexpr uint64_t m1 = AXIS == 0 ? 0x00ff00ff00ff00ffull : (AXIS == 1 ? 0x0000ffff0000ffffull : 0x00000000ffffffffull);   // cell bit AXIS + 3 clear
  uint64_t m = 0;
#pragma unroll
  for (int v = 0; v < 4; ++v)
    if (v >= lo && v <= hi) m |= ((v & 1) ? ~m0 : m0) & ((v & 2) ? ~m1 : m1);
  return m;
}
// cells of the block at lattice origin b0 that lie in the cube [h - r, h + r] (r < 0: none)
__device__ inline uint64_t cube_mask(const int (&b0)[3], const int (&h)[3], int r) {
  if (r < 0) return 0ull;
  return axis_mask<0>(h[0] - r - b0[0], h[0] + r - b0[0]) & axis_mask<1>(h[1] - r - b0[1], h[1] + r - b0[1]) &
         axis_mask<2>(h[2] - r - b0[2], h[2] + r - b0[2]);
}
// the entries of NP block ids: DirRef::find's probe sequence, all first reads in flight before any is consumed
template <int NP>
__device__ inline void dir_fetch(const DirRef &t, const uint64_t (&id)[NP], const bool (&ok)[NP], uint64_t (&occ)[NP], int32_t (&first)[NP]) {
  uint32_t slot[NP];
  ulonglong2 e[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) slot[j] = (uint32_t)(hash64(id[j]) & t.capm1);
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    e[j] = ok[j] ? *reinterpret_cast<const ulonglong2 *>(t.ent + slot[j]) : make_ulonglong2(kEmpty, 0ull);
    first[j] = ok[j] ? t.ent[slot[j]].first : 0;
  }
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    if (ok[j]) {
      uint32_t sl = slot[j];
      while (e[j].x != id[j] && e[j].x != kEmpty) {
        sl = (sl + 1) & (uint32_t)t.capm1;
        e[j] = *reinterpret_cast<const ulonglong2 *>(t.ent + sl);
        first[j] = t.ent[sl].first;
      }
    }
    occ[j] = e[j].x == id[j] ? e[j].y : 0ull;
  }
}
// rings r0 .. r1 around the home cell hb (biased lattice coordinates, in range).  The blocks that cover the cube of r1 are read eight
// at a time; rings are consumed in order with the termination test between them, which needs the whole cube in ONE batch of eight: a
// cube of <= 5 cells per axis touches <= 2 blocks per axis, so r1 <= 2 always qualifies, and a wider ring is asked for alone (r0 == r1).
__device__ inline bool dir_rings(const DirRef &t, int batch, int log2ts, const int (&hb)[3], const float (&f)[3], int r0, int r1, Best &best) {
  const int nbl = 1 << (kCoordBits - log2ts - 2);   // blocks per axis of the key range
  int lo[3], nb[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) { lo[a] = (hb[a] - r1) >> 2; nb[a] = ((hb[a] + r1) >> 2) - lo[a] + 1; }
  const int total = nb[0] * nb[1] * nb[2];
  const bool whole = total <= 8;
  for (int c0 = 0; c0 < total; c0 += 8) {
    uint64_t id[8], occ[8];
    int32_t first[8];
    int b0[8][3];
    bool ok[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      const int bx = lo[0] + c % nb[0], by = lo[1] + (c / nb[0]) % nb[1], bz = lo[2] + c / (nb[0] * nb[1]);
      b0[j][0] = bx * 4; b0[j][1] = by * 4; b0[j][2] = bz * 4;
      ok[j] = c < total && (((unsigned)bx | (unsigned)by | (unsigned)bz) < (unsigned)nbl) &&
              (cube_mask(b0[j], hb, r1) & ~cube_mask(b0[j], hb, r0 - 1)) != 0ull;
      id[j] = ok[j] ? pack_key(batch, (bx * 4) << log2ts, (by * 4) << log2ts, (bz * 4) << log2ts) >> (3 * log2ts + 6) : 0ull;
    }
    dir_fetch<8>(t, id, ok, occ, first);
    for (int r = r0; r <= r1; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint64_t w = occ[j] ? occ[j] & cube_mask(b0[j], hb, r) & ~cube_mask(b0[j], hb, r - 1) : 0ull;
        while (w) {   // <= 64 bits
          const int c = __ffsll((unsigned long long)w) - 1;
          w &= w - 1;
          const int cx = (c & 1) | ((c >> 2) & 2), cy = ((c >> 1) & 1) | ((c >> 3) & 2), cz = ((c >> 2) & 1) | ((c >> 4) & 2);
          const float d = site_d2(f, (float)(b0[j][0] + cx - hb[0]), (float)(b0[j][1] + cy - hb[1]), (float)(b0[j][2] + cz - hb[2]));
          if (d <= best.d2) {   // the row is one more random read: only for a candidate
            const int32_t pos = first[j] + __popcll(occ[j] & ((1ull << c) - 1ull));
            best_take(best, d, t.order ? t.order[pos] : pos);
          }
        }
      }
      if (whole && ring_done(best, r)) return true;
    }
  }
  return ring_done(best, r1);
}
__device__ inline bool ring_search(const DirRef &t, int batch, int log2ts, const int (&hb)[3], const float (&f)[3], int max_ring, Best &best) {
  // rings 0 and 1 share their directory reads: the <= 8 entries of the 3^3 cube serve both
  int r = max_ring >= 1 ? 2 : 1;
  bool done = dir_rings(t, batch, log2ts, hb, f, 0, r - 1, best);
  for (; !done && r <= max_ring; ++r) done = dir_rings(t, batch, log2ts, hb, f, r, r, best);
  return done;
}

// ---- stage A with the hash table: the cells of a shell, nine probes in flight (as k_build_map3)
__device__ inline bool hash_ring(const HashRef &t, int batch, int log2ts, const int (&hb)[3], const float (&f)[3], int r, Best &best) {
  const int side = 2 * r + 1, total = side * side * side;
  const unsigned ncell = 1u << (kCoordBits - log2ts);
  for (int i0 = 0; i0 < total; i0 += 9) {
    uint64_t key[9];
    bool ok[9];
    int k[9][3];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      const int i = i0 + j;
      k[j][0] = i % side - r; k[j][1] = (i / side) % side - r; k[j][2] = i / (side * side) - r;
      const int ux = hb[0] + k[j][0], uy = hb[1] + k[j][1], uz = hb[2] + k[j][2];
      const bool shell = k[j][0] == r || k[j][0] == -r || k[j][1] == r || k[j][1] == -r || k[j][2] == r || k[j][2] == -r;
      ok[j] = i < total && shell && (((unsigned)ux | (unsigned)uy | (unsigned)uz) < ncell);
      key[j] = ok[j] ? pack_key(batch, ux << log2ts, uy << log2ts, uz << log2ts) : 0ull;
    }
    int32_t row[9];
    t.find<9>(key, ok, row);
#pragma unroll
    for (int j = 0; j < 9; ++j)
      if (ok[j]) best_take(best, site_d2(f, (float)k[j][0], (float)k[j][1], (float)k[j][2]), row[j]);
  }
  return ring_done(best, r);
}
__device__ inline bool ring_search(const HashRef &t, int batch, int log2ts, const int (&hb)[3], const float (&f)[3], int max_ring, Best &best) {
  bool done = false;
  for (int r = 0; !done && r <= max_ring; ++r) done = hash_ring(t, batch, log2ts, hb, f, r, best);
  return done;
}

template <typename L>
__global__ __launch_bounds__(256) void k_nearest_ring(NearestArgs q, NearestAffines A, L look, int max_ring, int64_t *__restrict__ rows,
                                                      float *__restrict__ d2, int32_t *__restrict__ left, int32_t *__restrict__ n_left) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= q.m) return;
  const SiteQuery sq = site_query(q, A, i);
  Best best{__builtin_inff(), -1};
  bool done = !sq.finite;   // a non-finite point: row -1, d2 = +inf, no search
  if (!done) {
    const double bias = (double)(kBias >> q.log2ts), ncell = (double)(1 << (kCoordBits - q.log2ts));
    const double u0 = sq.h[0] + bias, u1 = sq.h[1] + bias, u2 = sq.h[2] + bias;
    if (u0 >= 0.0 && u0 < ncell && u1 >= 0.0 && u1 < ncell && u2 >= 0.0 && u2 < ncell) {
      const int hb[3] = {(int)u0, (int)u1, (int)u2};
      done = ring_search(look, q.batch_base + sq.scene, q.log2ts, hb, sq.f, max_ring, best);
    }
  }
  if (!done) {   // the exact scan's (left has room for all m queries)
    left[atomicAdd(n_left, 1)] = (int32_t)i;
    return;
  }
  rows[i] = best.row;
  if (d2) d2[i] = best.d2;
}

__global__ __launch_bounds__(256) void k_nearest_scan(NearestArgs q, NearestAffines A, const uint64_t *__restrict__ skeys, const int32_t *__restrict__ order,
                                                      int64_t n, const int32_t *__restrict__ left, const int32_t *__restrict__ n_left,
                                                      int64_t *__restrict__ rows, float *__restrict__ d2) {
  __shared__ float s_d[4];
  __shared__ int32_t s_r[4];
  const int32_t cnt = *n_left;   // <= m; the same in every thread, so the barriers below are reached by the whole workgroup
  const int bias = kBias >> q.log2ts;
  for (int32_t it = (int32_t)blockIdx.x; it < cnt; it += (int32_t)gridDim.x) {
    const int64_t i = left[it];
    const SiteQuery sq = site_query(q, A, i);
    const int batch = q.batch_base + sq.scene;
    const int64_t lo = lower_bound(skeys, (int64_t)0, n, (uint64_t)batch << kSceneShift);
    const int64_t hi = batch + 1 >= 1024 ? n : lower_bound(skeys, (int64_t)0, n, (uint64_t)(batch + 1) << kSceneShift);
    Best best{__builtin_inff(), -1};
    for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
      int bb, xb, yb, zb;
      unpack_key(skeys[p], bb, xb, yb, zb);
      // the offset from the home cell is formed in double (h may be far outside the key range) and is exact wherever stage A reaches
      const float kx = (float)((double)((xb >> q.log2ts) - bias) - sq.h[0]), ky = (float)((double)((yb >> q.log2ts) - bias) - sq.h[1]),
                  kz = (float)((double)((zb >> q.log2ts) - bias) - sq.h[2]);
      const float d = site_d2(sq.f, kx, ky, kz);
      if (d <= best.d2) best_take(best, d, order ? order[p] : (int32_t)p);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float od = __shfl_down(best.d2, o, 64);
      const int32_t orow = __shfl_down(best.row, o, 64);
      if (orow >= 0) best_take(best, od, orow);
    }
    if ((threadIdx.x & 63) == 0) { s_d[threadIdx.x >> 6] = best.d2; s_r[threadIdx.x >> 6] = best.row; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (s_r[w] >= 0) best_take(best, s_d[w], s_r[w]);
      rows[i] = best.row;
      if (d2) d2[i] = best.d2;
    }
    __syncthreads();   // s_d / s_r are rewritten by the next query
  }
}
// a map without sites: every query answers row -1, d2 = +inf
__global__ void k_nearest_none(int64_t m, int64_t *__restrict__ rows, float *__restrict__ d2) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  rows[i] = -1;
  if (d2) d2[i] = __builtin_inff();
}

}  // namespace lgs
