// lgs_conv.hip -- sparse convolution on gfx950: forward, dgrad, wgrad.
//
// Replaces the arithmetic of MinkowskiConvolution / MinkowskiConvolutionTranspose as called from
//   /root/reference/models/modules/common.py:195-203,228-236  (conv(), conv_tr())
//   /root/reference/models/modules/resnet_block.py:41-57       (BasicBlock.forward)
//   /root/reference/models/res16unet.py:196-270                 (Res16UNetBase.forward)
//
// Formulation: OUTPUT-STATIONARY IMPLICIT GEMM.  A workgroup owns a tile of
// Morton-consecutive output positions and a tile of output channels; for every kernel offset that has
// any neighbour in the tile (wavefront-ballot bitmask built with the kernel map) it gathers the
// neighbour rows straight from HBM into MFMA operand registers (16 B per lane, whole 32/64-byte row
// pieces), multiplies by the offset's weight slice staged once per workgroup in LDS (pre-packed in
// MFMA fragment order so the copy is linear and ds_read_b128 is conflict-free), and accumulates in
// fp32.  Every output row is written exactly once: no atomics, deterministic.  dgrad is the same
// kernel on transposed (and, for 3x3x3, mirrored) weights; transposed convs use the grouped view.
//
// MFMA use: v_mfma_f32_32x32x16_bf16 for bf16 storage, v_mfma_f32_32x32x2_f32 (exact fp32) for fp32.
// Operands are swapped (weights = A, voxels = B) so a lane ends up owning 4 consecutive output
// channels of one voxel -> 8/16-byte stores.  The reduction index (channel) is permuted identically on
// both operands so every lane's load is 16 contiguous bytes.
#include "lgs_common.h"

#include <type_traits>

#include <stdlib.h>
#include <string.h>

namespace lgs {


// fp32 STORAGE whose products run on the bf16 matrix pipe (round 5): every fp32 operand is split exactly into three bf16 pieces
// x = hi + mid + lo (8 + 8 + 8 significant bits, by truncation: each remainder is exact), and x * w is accumulated in fp32 from
// the six products hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid -- what is dropped (mid*lo, lo*mid, lo*lo) is below 2^-24 |x w|.
// v_mfma_f32_32x32x16_bf16 runs 16 x the flops per cycle of v_mfma_f32_32x32x2_f32: six products are 2.7 x faster on the pipe.
// The feature operand is split in registers as it streams through (11 VALU instructions per pair of elements, reused by every
// output-channel block of the wave); the weights are split once, when the packed image is made (three pieces per element).
struct f32s_t { float v; };
constexpr int kDtF32Split = 2;      // lgs_pack_desc.dtype of an image packed for f32s_t (internal; tensors are LGS_F32)
template <typename T> struct Tr;
template <> struct Tr<float> {
  static constexpr int EPL = 4;  // elements per 16-byte load
  static constexpr int LD = 4;   // 16-byte loads per lane per 32-channel chunk
  static constexpr int WLD = 4;  // 16-byte weight fragments per lane, chunk and output block
  static constexpr bool SPLIT = false;
};
template <> struct Tr<bf16_t> {
  static constexpr int EPL = 8;
  static constexpr int LD = 2;
  static constexpr int WLD = 2;
  static constexpr bool SPLIT = false;
};
template <> struct Tr<f32s_t> {
  static constexpr int EPL = 4;
  static constexpr int LD = 4;
  static constexpr int WLD = 6;  // [k-step of 16 channels: 2][piece hi / mid / lo: 3]
  static constexpr bool SPLIT = true;
};


// one 16-byte operand pair: bf16 = one 32x32x16 MFMA, fp32 = four 32x32x2 MFMAs
// 16-byte operands are native ext-vectors (not the HIP_vector_type struct): struct copies between address spaces
// lower to llvm.memcpy, which keeps the staging array in scratch memory instead of registers.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <typename T> __device__ inline void mma16(f32x16 &acc, const u32x4 &w, const u32x4 &f);
template <> __device__ inline void mma16<bf16_t>(f32x16 &acc, const u32x4 &w, const u32x4 &f) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, f), acc, 0, 0, 0);
}
// one fp32 value -> its three bf16 pieces as the upper halves of three dwords (hi + mid + lo == x exactly)
__device__ inline void split3(uint32_t x, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
  hi = x & 0xffff0000u;
  const float r1 = __uint_as_float(x) - __uint_as_float(hi);
  mid = __float_as_uint(r1) & 0xffff0000u;
  lo = __float_as_uint(r1 - __uint_as_float(mid));          // <= 8 significant bits: its lower half is zero
}
// eight consecutive fp32 reduction elements (two 16-byte loads) -> three bf16x8 MFMA operands
__device__ inline void split8(const u32x4 &a, const u32x4 &b, u32x4 &hi, u32x4 &mid, u32x4 &lo) {
  const uint32_t x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t h[8], m[8], l[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) split3(x[i], h[i], m[i], l[i]);
  // element 2i in the low half, 2i + 1 in the high half of dword i: v_perm_b32 picks the upper halves of both
#define LGS_PK(v, i) __builtin_amdgcn_perm(v[2 * (i) + 1], v[2 * (i)], 0x07060302u)
  hi = u32x4{LGS_PK(h, 0), LGS_PK(h, 1), LGS_PK(h, 2), LGS_PK(h, 3)};
  mid = u32x4{LGS_PK(m, 0), LGS_PK(m, 1), LGS_PK(m, 2), LGS_PK(m, 3)};
  lo = u32x4{LGS_PK(l, 0), LGS_PK(l, 1), LGS_PK(l, 2), LGS_PK(l, 3)};
#undef LGS_PK
}
template <> __device__ inline void mma16<float>(f32x16 &acc, const u32x4 &w, const u32x4 &f) {
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.x), __uint_as_float(f.x), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.y), __uint_as_float(f.y), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.z), __uint_as_float(f.z), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(w.w), __uint_as_float(f.w), acc, 0, 0, 0);
}

// Missing neighbours / padded channels are not branched around (hipcc would fence every such load with
// s_waitcnt vmcnt(0) and serialise the whole gather pipeline): their lane gets an out-of-range buffer offset, for
// which the hardware returns zeros.

// ------------------------------------------------------------------------------------ weight packing
// dst[kd][c][nb][t][lane] (16 B each): element e of lane (j = lane&31, h = lane>>5) is
//   Wsrc[g = c*32 + h*16 + t*EPL + e][o = nb*32 + j]   of weight matrix kd
// where (g = gathered/reduction channel, o = output channel):
//   plain      : Wsrc[g][o] = w[ks][g][o],        ks = kd
//   transposed : Wsrc[g][o] = w[ks][o][g]                                        (dgrad)
// with ks = mirror ? K-1-kd : kd in both: slot kd of a mirrored view (the shared 3^3 stride-1 table read from the other side: its
// dgrad, and the forward of its transposed conv) carries offset K-1-kd.
// Out-of-range g / o are zero (channel padding to multiples of 32).
template <typename T>
__device__ inline uint4 pack_one(const float *__restrict__ w, int K, int cin_w, int cout_w, int transposed, int mirror, int g_real,
                                 int o_real, int nc, int nb_total, int64_t idx) {
  constexpr int EPL = Tr<T>::EPL, LD = Tr<T>::WLD;
  int lane = (int)(idx & 63);
  int64_t r = idx >> 6;
  int t = (int)(r % LD); r /= LD;
  int nb = (int)(r % nb_total); r /= nb_total;
  int c = (int)(r % nc);
  int kd = (int)(r / nc);
  int ks = mirror ? K - 1 - kd : kd;
  int j = lane & 31, h = lane >> 5;
  int o = nb * 32 + j;
  if constexpr (Tr<T>::SPLIT) {
    // fragment t = 3 tt + piece: the eight reduction elements g = c*32 + h*16 + tt*8 + e of k-step tt, as bf16 piece `piece`
    const int tt = t / 3, piece = t % 3;
    uint32_t pc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int g = c * 32 + h * 16 + tt * 8 + e;
      float x = 0.f;
      if (g < g_real && o < o_real)
        x = transposed ? w[((int64_t)ks * cin_w + o) * cout_w + g] : w[((int64_t)ks * cin_w + g) * cout_w + o];
      uint32_t hi, mid, lo;
      split3(__float_as_uint(x), hi, mid, lo);
      pc[e] = piece == 0 ? hi : (piece == 1 ? mid : lo);
    }
    return make_uint4((pc[0] >> 16) | pc[1], (pc[2] >> 16) | pc[3], (pc[4] >> 16) | pc[5], (pc[6] >> 16) | pc[7]);
  }
  float vals[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    int g = c * 32 + h * 16 + t * EPL + e;
    float x = 0.f;
    if (g < g_real && o < o_real)
      x = transposed ? w[((int64_t)ks * cin_w + o) * cout_w + g] : w[((int64_t)ks * cin_w + g) * cout_w + o];
    vals[e] = x;
  }
  uint4 out;
  if constexpr (EPL == 4) {
    out = make_uint4(__float_as_uint(vals[0]), __float_as_uint(vals[1]), __float_as_uint(vals[2]), __float_as_uint(vals[3]));
  } else {
    out.x = (uint32_t)f32_to_bf16(vals[0]) | ((uint32_t)f32_to_bf16(vals[1]) << 16);
    out.y = (uint32_t)f32_to_bf16(vals[2]) | ((uint32_t)f32_to_bf16(vals[3]) << 16);
    out.z = (uint32_t)f32_to_bf16(vals[4]) | ((uint32_t)f32_to_bf16(vals[5]) << 16);
    out.w = (uint32_t)f32_to_bf16(vals[6]) | ((uint32_t)f32_to_bf16(vals[7]) << 16);
  }
  return out;
}

template <typename T>
__global__ void k_pack_weights(const float *__restrict__ w, int K, int cin_w, int cout_w, int transposed, int mirror,
                               int g_real, int o_real, int nc /*padded chunks*/, int nb_total /*padded blocks*/,
                               uint4 *__restrict__ dst) {
  constexpr int LD = Tr<T>::WLD;
  int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)K * nc * nb_total * LD * 64;
  if (idx >= total) return;
  dst[idx] = pack_one<T>(w, K, cin_w, cout_w, transposed, mirror, g_real, o_real, nc, nb_total, idx);
}

// every cached packed image of the model in ONE launch (after the optimiser step): blockIdx.y = descriptor
__global__ void k_pack_weights_batch(const lgs_pack_desc *__restrict__ descs) {
  const lgs_pack_desc e = descs[blockIdx.y];
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= e.total) return;
  uint4 *dst = reinterpret_cast<uint4 *>(e.packed);
  if (e.dtype == LGS_BF16) dst[idx] = pack_one<bf16_t>(e.weight, e.K, e.cin_w, e.cout_w, e.transposed, e.mirror, e.g_real, e.o_real, e.ncp, e.nbp, idx);
  else if (e.dtype == kDtF32Split) dst[idx] = pack_one<f32s_t>(e.weight, e.K, e.cin_w, e.cout_w, e.transposed, e.mirror, e.g_real, e.o_real, e.ncp, e.nbp, idx);
  else dst[idx] = pack_one<float>(e.weight, e.K, e.cin_w, e.cout_w, e.transposed, e.mirror, e.g_real, e.o_real, e.ncp, e.nbp, idx);
}

// inverse of k_pad_rows (lgs_common.h): [n, cpad] -> [n, c]
template <typename T>
__global__ void k_unpad_rows(const T *__restrict__ src, int64_t n, int c, int cpad, T *__restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * c) return;
  dst[i] = src[(i / c) * cpad + (i % c)];
}

// ------------------------------------------------------------------------------------ CLIP-loss epilogue (EPI = 1)
// The contraction S = normalize(F) . normalize(T)^T of ContrastiveLanguageLoss.feat_dist / feature_sim
// (/root/reference/lib/losses/ContrastiveLanguageLoss.py:73-95,185-192, lib/losses/utils.py:80-103) never needs its
// [N, n_anchor] result in memory: the loss reads 1 + K entries per row and the metrics read the arg-max.  With EPI = 1
// the tile's accumulators are reduced in the epilogue to  d_pos = 1 - s[label],  d_neg = 1 - mean_j s[neg_j],
// pred = argmax_a s[a]  and  1/|f|  (|f|^2 is accumulated from the operand fragments as they stream through, so the
// features are read exactly once); the similarity matrix itself is written only when the caller asks for it.
struct ClipEpi {
  const int64_t *labels = nullptr;   // [n]
  const int64_t *neg = nullptr;      // [n, k_neg] negative anchor indices
  int k_neg = 0;                     // 1..7
  int n_anchor = 0;
  int64_t ignore = -1;
  float *d_pos = nullptr, *d_neg = nullptr, *inv_norm = nullptr;
  int64_t *pred = nullptr;
};
// BatchNorm statistics from the conv epilogue (EPI = 0): when `partial` is set, every workgroup also writes, for its
// rows and channels, sum(y - pivot) and sum((y - pivot)^2) of the values it STORES (after the bf16 rounding, so they
// are the statistics of the tensor BatchNorm will read) to partial[tile][2][cout]: the [N, C] output is not read again
// for the statistics pass (k_colreduce<0> was ~6 % of the step).  pivot (may be NULL = 0) is a per-channel shift that
// keeps var = E[d^2] - E[d]^2 well conditioned; the caller passes BatchNorm's running mean.
struct BnEpi {
  float *partial = nullptr;     // [gridDim.x][2][cout_real]
  const float *pivot = nullptr; // [cout_real] or NULL
  int accum = 0;                // 1: out += result (lgs_conv_dgrad_accumulate: the residual branch's gradient is already in `out`)
};
// four adjacent stored elements -> fp32 (one 8- or 16-byte access)
__device__ inline void load4(const float *p, float (&v)[4]) { const float4 t = *reinterpret_cast<const float4 *>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
__device__ inline void load4(const bf16_t *p, float (&v)[4]) {
  const uint2 t = *reinterpret_cast<const uint2 *>(p);
  v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u); v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}
__device__ inline void load4(const f32s_t *p, float (&v)[4]) { load4(reinterpret_cast<const float *>(p), v); }
template <typename T> __device__ inline float stored_value(float x);
template <> __device__ inline float stored_value<f32s_t>(float x) { return x; }
template <> __device__ inline float stored_value<float>(float x) { return x; }
template <> __device__ inline float stored_value<bf16_t>(float x) { return bf16_to_f32(f32_to_bf16(x)); }
template <typename T> __device__ inline float sq16(const u32x4 &f, float s) {   // four fp32 (float and f32s_t rows)
  const float a = __uint_as_float(f.x), b = __uint_as_float(f.y), c = __uint_as_float(f.z), d = __uint_as_float(f.w);
  return fmaf(d, d, fmaf(c, c, fmaf(b, b, fmaf(a, a, s))));
}
template <> __device__ inline float sq16<bf16_t>(const u32x4 &f, float s) {
  // two bf16 per dword: the high one IS an fp32 with the low half masked off, the low one is a 16-bit shift away
  const uint32_t w[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = __uint_as_float(w[i] << 16), hi = __uint_as_float(w[i] & 0xffff0000u);
    s = fmaf(hi, hi, fmaf(lo, lo, s));
  }
  return s;
}

// ------------------------------------------------------------------------------------ forward / dgrad
// Tile: WM x WN waves; each wave owns RB*32 positions x NCB*32 output channels.
// SCL = chunks FETCHED AND STAGED per slab (see below); ROW1 = the gathered rows are one 16-byte piece wide (conv0's padded
// colour rows): only the t = 0 gather is issued, the fragments of the pieces beyond the row are zero registers.
// BN = the instance carries the BatchNorm statistics epilogue (BnEpi::partial).  The epilogue's vst[32 * NCB] butterfly is the
// register peak of every instance that has it, although it sits behind a kernel-uniform branch no default launch takes: tile 7
// is allocated 204 registers with it and 164 without (137 where it is built for three waves per SIMD).  gather_instance() picks the variant per launch.
// ONEBUF = ONE weight slab in LDS instead of two: the next slab still waits in registers while this one is multiplied, but it
// is staged between two barriers at the slab's end instead of beside the MFMAs.  For the walk whose two slabs cost the CU a
// workgroup (tile 7, one slab of three chunks: 62 KB -> 38 KB).
//
// THE instance table of k_conv_gather: every instance that exists, one row each.  Which tile a launch gets is gather_id()'s
// choice, which row of the tile gather_instance()'s; tile_of(), the dispatch (with_gather_kernel), the launch-site names, the
// residency static_asserts and the debug queries are all generated from these rows (kF32 = the instance multiplies fp32).
//   TILE(ID, RB, NCB, WM, WN, SC, D, BF16, LEAN, BUILT): the tile's own instance, walking the image's SC-chunk slabs.  SC = chunks
//        per weight slab (sized to ~6-8 staging registers per thread), D = depth of the gather ring.  BF16: no fp32 instance.
//        LEAN: the bf16 instance has a twin without the statistics epilogue (BN = false); BUILT = workgroups per CU the twins of
//        the tile and of its walks are built for (__launch_bounds__; 0 = nothing stated).
//   WALK(ID, RB, NCB, WM, WN, SC, D, SCL, ROW1, ONEBUF, OCC): the same tile (bf16) walked with SCL-chunk slabs, on one-piece rows
//        (ROW1); both epilogue variants exist, ONEBUF: the lean one keeps ONE slab in LDS.  OCC = workgroups per CU of the tile's
//        own instance with the statistics epilogue (registers, from the ISA): the walk may not take more LDS than leaves that many.
//   CLIP(ID, RB, NCB, WM, WN, SC, D): the EPI = 1 instances of the fused CLIP loss, one column tile of NCB blocks; ID = -NCB.
// The six tile parameters are spelled as the launch sites are named (tests and profiles key on that text), so walks repeat them.
#define LGS_GATHER_TABLE(TILE, WALK, CLIP)                                                                                 \
  TILE(0, 2, 1, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), false, true, 0)                                                      \
  WALK(0, 2, 1, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 1, false, false, 3)                                                  \
  WALK(0, 2, 1, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 1, true, false, 3)                                                   \
  WALK(0, 2, 1, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 2, false, false, 3)                                                  \
  WALK(0, 2, 1, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 3, false, false, 3)                                                  \
  TILE(1, 2, 2, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), false, true, 0)                                                      \
  WALK(1, 2, 2, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 1, false, false, 2)                                                  \
  WALK(1, 2, 2, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 2, false, false, 2)                                                  \
  WALK(1, 2, 2, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 3, false, false, 2)                                                  \
  TILE(2, 2, 3, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), false, true, 0)                                                      \
  WALK(2, 2, 3, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 1, false, false, 2)                                                  \
  WALK(2, 2, 3, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 2, false, false, 2)                                                  \
  WALK(2, 2, 3, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4), 3, false, false, 2)                                                  \
  TILE(3, 2, 4, 4, 1, (kF32 ? 1 : 2), (kF32 ? 2 : 3), false, false, 0) /* 256 positions x 128 channels (64 x 128 per wave) */ \
  TILE(4, 1, 1, 2, 1, (kF32 ? 2 : 4), (kF32 ? 4 : 8), false, false, 0)                                                     \
  TILE(5, 1, 1, 2, 2, (kF32 ? 2 : 4), (kF32 ? 4 : 8), false, false, 0)                                                     \
  TILE(6, 1, 7, 4, 1, (kF32 ? 1 : 2), (kF32 ? 3 : 4), false, true, 0)                                                      \
  /* 128 positions x 128 channels (32 x 128 per wave).  Without the statistics epilogue it is BUILT for three workgroups per CU  \
     (one wave of each per SIMD): 168 registers at most; 30 / 46 KB of LDS on its 1- and 2-chunk walks, 38 KB on the 3-chunk walk \
     with one slab buffer (with two it would hold 62 KB: two workgroups).  With the epilogue: 204 registers, two per CU */   \
  TILE(7, 1, 4, 4, 1, 2, 4, true, true, 3)                                                                                 \
  WALK(7, 1, 4, 4, 1, 2, 4, 1, false, false, 2)                                                                            \
  WALK(7, 1, 4, 4, 1, 2, 4, 3, false, true, 2)                                                                             \
  TILE(8, 1, 2, 4, 1, 4, 6, true, false, 0)                                                                                \
  TILE(9, 1, 2, 2, 2, 4, 6, true, false, 0)                                                                                \
  TILE(10, 1, 2, 2, 1, 4, 6, true, false, 0)                                                                               \
  TILE(11, 1, 4, 2, 1, 4, 6, true, false, 0)                                                                               \
  TILE(12, 1, 2, 4, 1, 8, 6, true, false, 0) /* as 8 with 8-chunk (256-channel) weight slabs: half the slab barriers */     \
  TILE(13, 1, 4, 4, 1, 8, 4, true, false, 0) /* 128 positions x 128 channels, 8-chunk slabs */                             \
  TILE(16, 1, 8, 8, 1, 2, 4, true, true, 0)  /* eight waves of 32 positions x 256 channels */                              \
  CLIP(-1, 1, 1, 4, 1, (kF32 ? 4 : 8), (kF32 ? 4 : 8))                                                                     \
  CLIP(-2, 1, 2, 4, 1, (kF32 ? 2 : 4), (kF32 ? 3 : 4))                                                                     \
  CLIP(-4, 1, 4, 4, 1, (kF32 ? 1 : 2), (kF32 ? 3 : 4))                                                                     \
  CLIP(-7, 1, 7, 4, 1, (kF32 ? 1 : 2), (kF32 ? 3 : 4))
#define LGS_NO_ROW(...)

// workgroups per CU the instance is built for (four waves: one of each per SIMD), 0 = nothing stated: BUILT of its tile's row
template <typename T, int RB, int NCB, int WM, int WN, int SC, int D, int EPI, int SCL, bool BN, bool ONEBUF>
constexpr int gather_waves_per_simd() {
  constexpr bool kF32 = (sizeof(T) == 4);
  if (kF32 || EPI != 0 || BN) return 0;
#define LGS_BUILT(ID, RB_, NCB_, WM_, WN_, SC_, D_, BF16, LEAN, BUILT) \
  if (RB == RB_ && NCB == NCB_ && WM == WM_ && WN == WN_ && SC == SC_ && D == D_) return BUILT;
  LGS_GATHER_TABLE(LGS_BUILT, LGS_NO_ROW, LGS_NO_ROW)
#undef LGS_BUILT
  return 0;
}
template <typename T, int RB, int NCB, int WM, int WN, int SC, int D, int EPI = 0, int SCL = SC, bool ROW1 = false, bool BN = (EPI == 0),
          bool ONEBUF = false>
__global__ __launch_bounds__(WM *WN * 64, (gather_waves_per_simd<T, RB, NCB, WM, WN, SC, D, EPI, SCL, BN, ONEBUF>())) void k_conv_gather(View v, const T *__restrict__ in, int cin_real, int nc,
                                                             const u32x4 *__restrict__ wp, int nb_total,
                                                             int ncp, int nbp,
                                                             T *__restrict__ out, int cout_real,
                                                             const float *__restrict__ bias,
                                                             float *__restrict__ out_f32_arg,
                                                             const float *__restrict__ row_scale,
                                                             unsigned in_bytes, unsigned w_bytes, int64_t zstride,
                                                             ClipEpi ce, BnEpi be, int gc, int in_ld) {
  static_assert(EPI == 0 || (RB == 1 && WN == 1), "the CLIP epilogue owns whole rows: one row block, all columns per wave");
  // SC = 32-channel chunks per weight SLAB: the weights of (offset, slab) are staged in LDS once per workgroup
  // and one barrier separates slabs, while the gathered feature fragments stream chunk by chunk through a
  // D-deep register ring (loads issued D-1 chunks = several hundred MFMA cycles ahead of their use) that runs
  // across slab and offset boundaries.
  // SC is the slab length of the packed IMAGE (plan_image() rounds the chunks of an offset up to whole SC-chunk slabs, zero
  // filled); SCL is the slab length this instance WALKS it with.  The image is chunk-major -- chunk c of offset kw starts at
  // (kw * ncp + c) * nbp * WLD * 64 -- so any SCL that divides nc reads exactly the real chunks and never the zero padding
  // (launch_gather picks it; SCL = SC is the walk of the image's own slabs, padding included).
  static_assert(SCL >= 1 && (EPI == 0 || SCL == SC), "the CLIP epilogue parks its similarity tile in the weight LDS of the image's own slabs");
  static_assert(!ROW1 || EPI == 0, "the one-piece row is a convolution input");
  static_assert(!BN || EPI == 0, "BatchNorm statistics are a convolution epilogue");
  static_assert(!ONEBUF || (EPI == 0 && !BN), "both epilogues that use the weight LDS count on two slabs of it");
  constexpr int EPL = Tr<T>::EPL, LD = Tr<T>::LD, WLD = Tr<T>::WLD;
  constexpr int NT = WM * WN * 64;
  constexpr int TM = WM * RB * 32;
  constexpr int WB = WN * NCB;                 // weight blocks per chunk
  constexpr int WCH = WB * WLD * 64;           // uint4 per chunk
  constexpr int SLAB = SCL * WCH;              // uint4 per slab
  constexpr int WR = (SLAB + NT - 1) / NT;     // staging registers per thread
  __shared__ u32x4 lds[ONEBUF ? 1 : 2][SLAB];
  static_assert(!BN || WM * 2 * WB * 32 * 4 <= 2 * SLAB * 16, "the statistics epilogue folds the waves through the weight LDS");

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int vx = lane & 31, h = lane >> 5;
  // XCD-aware tile order: the dispatcher places workgroup b on XCD b % 8 (speed only, never correctness), so give
  // every XCD a CONTIGUOUS run of position tiles -- neighbouring tiles share most of their gathered rows and
  // now hit the same private L2.  Bijective for any tile count.
  int64_t tile;
  {
    const unsigned nt = gridDim.x, xcd = blockIdx.x & 7u, j = blockIdx.x >> 3, q = nt >> 3, r = nt & 7u;
    tile = (int64_t)(xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
  }
  const int64_t pos_wg = tile * TM;
  const int64_t pos_w = pos_wg + (int64_t)wm * RB * 32;
  // Eight-wave tiles (one 32-row block per wave) INTERLEAVE the tile's rows over the waves (row i -> wave i % 8): the
  // rows are sorted by neighbourhood shape, so contiguous blocks would leave whole waves without work at an offset while
  // the others run their MFMAs, and everybody meets at the next slab barrier.
  constexpr bool ILV = (WM == 8 && RB == 1 && EPI == 0);
  auto row_of = [&](int rb) __attribute__((always_inline)) { return ILV ? vx * WM + wm : wm * RB * 32 + rb * 32 + vx; };
  const int nb_wg = blockIdx.y * WB;  // first cout block of the workgroup
  const int nb_w = nb_wg + wn * NCB;  // first cout block of this wave

  // ---- which slots does this workgroup visit, with which weight matrix
  uint32_t smask = 1;  // single slot
  int kw_single = 0;
  if (v.KS > 1) {
    smask = 0;
#pragma unroll
    for (int g = 0; g < (TM + 63) / 64; ++g) smask |= v.mask64[pos_wg / 64 + g];
  } else if (v.tile_k) {
    kw_single = v.tile_k[pos_wg / 64];
    if (kw_single < 0) {        // padding group: nothing to write (its statistics row is all zeros)
      if constexpr (BN) {
        if (be.partial != nullptr)
          for (int e = tid; e < 2 * WB * 32; e += NT) {
            const int st = e / (WB * 32), ch = nb_wg * 32 + e % (WB * 32);
            if (ch < cout_real) be.partial[((int64_t)tile * 2 + st) * cout_real + ch] = 0.f;
          }
      }
      return;
    }
  }
  // Slot split (gridDim.z == 3, 3^3 maps of the coarse levels): this workgroup sums only 9 of the 27 offsets into
  // its own fp32 partial image; k_sum_partials adds the three in a fixed order.  A coarse level has too few row
  // tiles to fill the chip and every tile streams ALL weights, so the split buys parallelism, not traffic.
  float *out_f32 = out_f32_arg;
  if (gridDim.z > 1) {
    smask &= 0x1ffu << (9 * blockIdx.z);
    out_f32 += (int64_t)blockIdx.z * zstride;
  }

  f32x16 acc[RB][NCB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb)
#pragma unroll
    for (int nb = 0; nb < NCB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rb][nb][r] = 0.f;

  // ---- gather indices of every visited slot are parked in LDS once (coalesced), so that the per-offset index
  // fetch is a ds_read (lgkmcnt) and never sits in the VMEM queue in front of the gather ring
  __shared__ __attribute__((aligned(16))) int32_t l_idx[27 * TM];
  // ---- feature-side iterator: flat sequence of (slot, chunk)
  // Order of the reduction: channel GROUPS of gc chunks outermost, then the offsets, then the chunks of the group.
  // gc = nc (one group) is the plain "offset by offset" order.  With wide rows (512 channels = 1 KB) the plain order
  // touches every gathered row in sixteen 64-byte pieces per offset and comes back to it ~14 offsets later: the rows of
  // the co-resident tiles plus 14 MB of weights do not fit the XCD's 4 MB L2 (PMC: L2 hit 51 %, 19x the compulsory HBM
  // bytes); with 128-channel groups a row's 256-byte segment serves all offsets back to back.
  const uint32_t fmask = smask;  // offsets the feature side walks
  uint32_t rem = smask;
  int islot = -1, gbase = 0, gend = min(gc, nc), ichunk = gend;  // forces "advance to first slot" on the first call
  int32_t idx_i[RB];
  auto advance = [&]() __attribute__((always_inline)) -> bool {
    if (++ichunk < gend) return true;
    if (rem == 0) {                       // next channel group: all offsets again
      gbase = gend;
      if (gbase >= nc) return false;
      gend = min(gbase + gc, nc);
      rem = fmask;
    }
    islot = __builtin_ctz(rem);
    rem &= rem - 1;
    ichunk = gbase;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int r = row_of(rb);
      const int64_t p = pos_wg + r;
      idx_i[rb] = v.nbr ? l_idx[islot * TM + r] : (p < v.n_in ? (int32_t)p : -1);
    }
    return true;
  };
  // Gathers and weight fetches are BUFFER loads (scalar descriptor + one 32-bit lane offset): a missing neighbour or
  // a padded channel simply gets an out-of-range offset, for which the hardware returns zeros -- no branches, no
  // 64-bit address arithmetic, no selects (the gather loop was spending ~10 VALU instructions per MFMA on those).
  constexpr unsigned kOOB = 0xfffff000u;   // > any descriptor size accepted by the host wrapper, no wrap with small immediates
  const __amdgpu_buffer_rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(in), 0, (int)in_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<u32x4 *>(wp), 0, (int)w_bytes, 0x00020000);
  // in_ld = row stride of the gathered tensor in elements (> cin_real when it is a column slice of a wider buffer, e.g.
  // the skip half of a zero-copy ME.cat)
  const unsigned row_bytes = (unsigned)in_ld * (unsigned)sizeof(T);
  const bool ch_tail = (cin_real & 31) != 0;   // kernel-uniform: only then a chunk can run past the row
  auto issue = [&](u32x4 (&F)[RB][LD], uint32_t &act) __attribute__((always_inline)) {
    act = 0;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const bool ok = idx_i[rb] >= 0;
      if (__ballot(idx_i[rb] >= 0)) act |= 1u << rb;
      const unsigned base = ok ? (unsigned)idx_i[rb] * row_bytes + (unsigned)(ichunk * 32 + h * 16) * (unsigned)sizeof(T) : kOOB;
#pragma unroll
      for (int t = 0; t < LD; ++t) {
        unsigned off = base + t * 16;
        if (ch_tail && (ichunk * 32 + h * 16 + t * EPL + EPL > cin_real)) off = kOOB;
        if (ROW1 && t > 0) F[rb][t] = u32x4{0u, 0u, 0u, 0u};     // beyond the row in every lane: no instruction for it
        else F[rb][t] = __builtin_amdgcn_raw_buffer_load_b128(rs_in, off, 0, 0);
      }
    }
  };
  // ---- weight-side iterator: (slot, slab) in the same order
  const int nslab = (nc + SCL - 1) / SCL, gs = (gc + SCL - 1) / SCL;   // slabs per channel group (gc is a multiple of SCL or = nc)
  uint32_t wrem = smask;
  int wslot = -1, wgbase = 0, wgend = min(gs, nslab), wslab = wgend;
  auto wadvance = [&]() __attribute__((always_inline)) -> bool {
    if (++wslab < wgend) return true;
    if (wrem == 0) {
      wgbase = wgend;
      if (wgbase >= nslab) return false;
      wgend = min(wgbase + gs, nslab);
      wrem = smask;
    }
    wslot = __builtin_ctz(wrem);
    wrem &= wrem - 1;
    wslab = wgbase;
    return true;
  };
  // The packed weights are padded to whole slabs (ncp chunks) and whole cout tiles (nbp blocks), zero filled, so a
  // slab is fetched with unconditional, fully coalesced 16-byte buffer loads: per-thread offsets are loop invariant,
  // the slab's base goes in the scalar offset.  (With SCL < SC the last slab read ends at chunk nc - 1 <= ncp - 1.)
  unsigned woff[WR];
#pragma unroll
  for (int i = 0; i < WR; ++i) {
    const int e = min(tid + i * NT, SLAB - 1);
    const int cw = e / WCH, ee = e - cw * WCH;
    woff[i] = (unsigned)(cw * nbp * (WLD * 64) + ee) * 16u;
  }
  auto wissue = [&](u32x4 (&wreg)[WR]) __attribute__((always_inline)) {
    const int kw = v.KS > 1 ? wslot : kw_single;  // 3^3 dgrad mirroring (K-1-k) is folded into the weight packing
    const unsigned sbase = (unsigned)((((int64_t)kw * ncp + wslab * SCL) * nbp + nb_wg) * (WLD * 64) * 16);
#pragma unroll
    for (int i = 0; i < WR; ++i) wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, woff[i], sbase, 0);
  };
  auto wstage = [&](int buf, const u32x4 (&wreg)[WR]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < WR; ++i) {
      const int e = tid + i * NT;
      if (e < SLAB) lds[buf][e] = wreg[i];
    }
  };
  float sumsq = 0.f;   // EPI = 1: |f|^2 of this lane's channel half of row vx
  auto compute = [&](int buf, int cc, const u32x4 (&F)[RB][LD], uint32_t act) __attribute__((always_inline)) {
    if (act == 0) return;
    if constexpr (EPI == 1) {
#pragma unroll
      for (int t = 0; t < LD; ++t) sumsq = sq16<T>(F[0][t], sumsq);
    }
    const u32x4 *wl = &lds[buf][cc * WCH + (wn * NCB) * WLD * 64 + lane];
    if constexpr (Tr<T>::SPLIT) {
      // split fp32: per k-step of 16 channels (two of the lane's four loads) the feature fragment becomes three bf16 operands,
      // reused by all NCB column blocks; the six products go smallest first into the same fp32 accumulator
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        u32x4 wf3[3][NCB];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
          for (int nb = 0; nb < NCB; ++nb) wf3[pc][nb] = wl[(nb * WLD + tt * 3 + pc) * 64];
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          if (act & (1u << rb)) {
            u32x4 fh, fm, fl;
            split8(F[rb][2 * tt], F[rb][2 * tt + 1], fh, fm, fl);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<bf16_t>(acc[rb][nb], wf3[2][nb], fh);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<bf16_t>(acc[rb][nb], wf3[0][nb], fl);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<bf16_t>(acc[rb][nb], wf3[1][nb], fm);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<bf16_t>(acc[rb][nb], wf3[1][nb], fh);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<bf16_t>(acc[rb][nb], wf3[0][nb], fm);
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<bf16_t>(acc[rb][nb], wf3[0][nb], fh);
          }
        }
      }
    } else {
      // all weight fragments of the chunk are requested up front: the LDS latency of step t+1 hides under the
      // MFMAs of step t (the compiler otherwise waits lgkmcnt(0) in front of every MFMA triple)
      u32x4 wf[LD][NCB];
#pragma unroll
      for (int t = 0; t < LD; ++t)
#pragma unroll
        for (int nb = 0; nb < NCB; ++nb) wf[t][nb] = wl[(nb * LD + t) * 64];
#pragma unroll
      for (int t = 0; t < LD; ++t) {
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
          if (act & (1u << rb)) {
#pragma unroll
            for (int nb = 0; nb < NCB; ++nb) mma16<T>(acc[rb][nb], wf[t][nb], F[rb][t]);
          }
        }
      }
    }
  };

  u32x4 F[D][RB][LD], wreg[WR];
  uint32_t act[D];
  int buf = 0, cc = 0;       // LDS buffer holding the current slab, chunk index inside it
  int ncs = 0;               // chunks in the current slab
  bool wnext = false;        // is a following slab prefetched in wreg?
  int issued = 0, computed = 0;
  int pslab = -1;               // slab index of the prefetched weight slab
  // Prologue: the first weight slab and ALL index loads of the tile are in flight together, one barrier publishes
  // both (a slot-by-slot index copy loop was a chain of ~16 dependent global-load latencies at the head of every
  // workgroup -- a quarter of its lifetime -- and the first weight fetch only started behind it).
  const bool whave = wadvance();
  if (whave) wissue(wreg);
  // kernel-map rows of the tile: SIXTEEN-byte loads, four consecutive positions of one offset per lane (the table is
  // offset-major and position tiles are 16-byte aligned): 27 x TM / 4 / 64 wave-instructions per tile instead of one 4-byte
  // load per (offset, wave) -- 27 instead of 108 per 256-position tile of the ~900 vector-memory instructions the kernel is
  // bound by.  Offsets the tile does not visit get an out-of-range address (zeros, never read).
  const uint64_t idx_bytes = (uint64_t)v.KS * (uint64_t)v.n_pad * 4ull;
  if (v.nbr && idx_bytes < 0xfffff000ull) {     // kernel-uniform
    constexpr int Q = TM / 4, NU = (27 * Q + NT - 1) / NT;
    const __amdgpu_buffer_rsrc_t rs_idx = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(v.nbr), 0, (int)idx_bytes, 0x00020000);
    u32x4 t4[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int e = tid + i * NT, sl = e / Q, q = e - sl * Q;
      const bool ok = sl < v.KS && ((smask >> sl) & 1u);
      const unsigned off = ok ? (unsigned)(((int64_t)sl * v.n_pad + pos_wg + 4 * q) * 4) : 0xfffff000u;
      t4[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_idx, off, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int e = tid + i * NT, sl = e / Q, q = e - sl * Q;
      if (sl < 27) *reinterpret_cast<u32x4 *>(&l_idx[sl * TM + 4 * q]) = t4[i];
    }
  } else if (v.nbr) {
    constexpr int IT = (TM + NT - 1) / NT;
    int32_t tmp[27][IT];
#pragma unroll
    for (int sl = 0; sl < 27; ++sl) {
      if ((smask >> sl) & 1u) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          const int r = tid + it * NT;
          tmp[sl][it] = r < TM ? v.nbr[(int64_t)sl * v.n_pad + pos_wg + r] : -1;
        }
      }
    }
#pragma unroll
    for (int sl = 0; sl < 27; ++sl) {
      if ((smask >> sl) & 1u) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          const int r = tid + it * NT;
          if (r < TM) l_idx[sl * TM + r] = tmp[sl][it];
        }
      }
    }
  }
  if (whave) {
    wstage(0, wreg);
    ncs = min(SCL, nc - wslab * SCL);
    wnext = wadvance();
    if (wnext) { pslab = wslab; wissue(wreg); }
  }
  __syncthreads();   // indices and the first weight slab are visible
  const int total = __builtin_popcount(fmask) * nc;  // chunks of this wave
#pragma unroll
  for (int d = 0; d < D - 1; ++d) {
    act[d] = 0;
    if (issued < total) { advance(); issue(F[d], act[d]); ++issued; }
  }
  act[D - 1] = 0;
  // at the end of a slab publish the prefetched next slab and cross one barrier
  auto slab_end = [&]() __attribute__((always_inline)) {
    if constexpr (ONEBUF) {
      if (wnext) {           // workgroup-uniform.  (After the last slab nobody touches the weight LDS again: no barrier.)
        __syncthreads();     // every wave has multiplied the slab that is overwritten now
        wstage(0, wreg);
        __syncthreads();
      }
    } else {
      if (wnext) wstage(buf ^ 1, wreg);
      __syncthreads();
      buf ^= 1;
    }
    cc = 0;
    if (wnext) {
      ncs = min(SCL, nc - pslab * SCL);
      wnext = wadvance();
      if (wnext) { pslab = wslab; wissue(wreg); }
    }
  };
  // steady state: every sub-step issues one chunk and computes one chunk UNCONDITIONALLY, so the compiler can
  // count outstanding loads (s_waitcnt vmcnt(N), N > 0) instead of draining the queue before every MFMA group
  while (total - issued >= D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      advance();
      issue(F[(d + D - 1) % D], act[(d + D - 1) % D]);
      compute(buf, cc, F[d], act[d]);
      if (++cc == ncs) slab_end();
    }
    issued += D;
    computed += D;
  }
  // tail (< 2D chunks)
  while (computed < total) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (computed < total) {
        if (issued < total) { advance(); issue(F[(d + D - 1) % D], act[(d + D - 1) % D]); ++issued; }
        compute(buf, cc, F[d], act[d]);
        ++computed;
        if (++cc == ncs) slab_end();
      }
    }
  }

  if constexpr (EPI == 1) {
    // ---- CLIP-loss epilogue.  The weight LDS is idle now: every wave parks one 32 x 32 block of its similarity tile
    // there at a time (row stride 36 floats) so that a lane can pick the entries of ITS row's label / negatives with
    // an indexed ds_read (registers cannot be indexed per lane); the arg-max runs on the registers.
    __syncthreads();
    float *tile = reinterpret_cast<float *>(&lds[0][0]) + wave * (32 * 36);
    sumsq += __shfl_xor(sumsq, 32);
    const float inv = 1.f / fmaxf(sqrtf(sumsq), 1e-12f);
    const int64_t p = pos_w + vx;
    const bool live = p < v.n_out;
    // half h of row vx handles targets j = h, h + 2, ...  (j = 0: the positive, j >= 1: negative j - 1)
    int tcol[4];
    int64_t lab = ce.ignore;
    if (live) lab = ce.labels[p];
    const bool valid = live && lab != ce.ignore && lab >= 0 && lab < ce.n_anchor;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int j = 2 * jj + h;
      int t = -1;
      if (valid && j <= ce.k_neg) {
        const int64_t tt = j == 0 ? lab : ce.neg[p * ce.k_neg + (j - 1)];
        t = (tt >= 0 && tt < ce.n_anchor) ? (int)tt : -1;
      }
      tcol[jj] = t;
    }
    float best = -3.0e38f, spos = 0.f, sneg = 0.f;
    int bi = 0;
#pragma unroll
    for (int nb = 0; nb < NCB; ++nb) {
      if (nb_w + nb >= nb_total) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c0 = (nb_w + nb) * 32 + 8 * q + 4 * h;
        const float s0 = acc[0][nb][4 * q + 0] * inv, s1 = acc[0][nb][4 * q + 1] * inv, s2 = acc[0][nb][4 * q + 2] * inv,
                    s3 = acc[0][nb][4 * q + 3] * inv;
        *reinterpret_cast<float4 *>(tile + vx * 36 + 8 * q + 4 * h) = make_float4(s0, s1, s2, s3);
        if (c0 + 0 < ce.n_anchor && s0 > best) { best = s0; bi = c0 + 0; }
        if (c0 + 1 < ce.n_anchor && s1 > best) { best = s1; bi = c0 + 1; }
        if (c0 + 2 < ce.n_anchor && s2 > best) { best = s2; bi = c0 + 2; }
        if (c0 + 3 < ce.n_anchor && s3 > best) { best = s3; bi = c0 + 3; }
        if (out_f32 && live && c0 < cout_real)
          *reinterpret_cast<float4 *>(out_f32 + p * cout_real + c0) = make_float4(s0, s1, s2, s3);
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int t = tcol[jj];
        if (t >= 0 && (t >> 5) == nb_w + nb) {
          const float sv = tile[vx * 36 + (t & 31)];
          if (jj == 0 && h == 0) spos = sv; else sneg += sv;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    {  // the two halves of a row: first maximum (lowest index on ties), sums
      const float ob = __shfl_xor(best, 32);
      const int oi = __shfl_xor(bi, 32);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
      sneg += __shfl_xor(sneg, 32);
      spos += __shfl_xor(spos, 32);
    }
    if (live && h == 0) {
      ce.d_pos[p] = valid ? 1.f - spos : 0.f;
      ce.d_neg[p] = valid ? 1.f - sneg / (float)ce.k_neg : 0.f;
      if (ce.pred) ce.pred[p] = bi;
      if (ce.inv_norm) ce.inv_norm[p] = inv;
    }
    return;
  }
  // ---- epilogue: lane (voxel vx, half h) owns channels nb*32 + 8q + 4h + {0..3}
  // bf16 rows on the 8-channel grid: SIXTEEN-byte stores.  The accumulator layout gives a lane four 4-channel pieces (8 bytes of
  // bf16 each) 16 bytes apart; the two half-wave lanes of a voxel hold interleaved pieces.  v_permlane32_swap trades piece
  // q = 2p+1 of the h = 0 lane for piece q = 2p of the h = 1 lane, so that lane h owns the 8 contiguous channels
  // nb*32 + 16p + 8h .. + 7: half as many store instructions (the kernel sits on the CU's vector-memory instruction rate, and
  // the classifier's 200-channel rows are mostly stores).  Same values, same rounding -- only who writes them changes.
  if constexpr (EPL == 8 && EPI == 0) {
    if (!out_f32 && (cout_real & 7) == 0) {      // kernel-uniform
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        int64_t p = pos_wg + row_of(rb);
        int32_t orow = v.out_row ? v.out_row[p] : (p < v.n_out ? (int32_t)p : -1);
        T *dst = out + (int64_t)(orow < 0 ? 0 : orow) * cout_real;
#pragma unroll
        for (int nb = 0; nb < NCB; ++nb) {
          if (nb_w + nb >= nb_total) continue;
#pragma unroll
          for (int pq = 0; pq < 2; ++pq) {
            uint32_t pk[2][2];                   // [piece q = 2pq, 2pq+1][dword]
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const int q = 2 * pq + e, c0 = (nb_w + nb) * 32 + 8 * q + 4 * h;
              float o0 = acc[rb][nb][4 * q + 0], o1 = acc[rb][nb][4 * q + 1], o2 = acc[rb][nb][4 * q + 2], o3 = acc[rb][nb][4 * q + 3];
              if (bias && c0 < cout_real) { o0 += bias[c0]; o1 += bias[c0 + 1]; o2 += bias[c0 + 2]; o3 += bias[c0 + 3]; }
              pk[e][0] = (uint32_t)f32_to_bf16(o0) | ((uint32_t)f32_to_bf16(o1) << 16);
              pk[e][1] = (uint32_t)f32_to_bf16(o2) | ((uint32_t)f32_to_bf16(o3) << 16);
            }
            // after the swaps: lane h holds [pk0 | pk1] = channels nb*32 + 16 pq + 8h + {0..3 | 4..7}
            const auto s0 = __builtin_amdgcn_permlane32_swap(pk[0][0], pk[1][0], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(pk[0][1], pk[1][1], false, false);
            const int c8 = (nb_w + nb) * 32 + 16 * pq + 8 * h;
            if (orow >= 0 && c8 < cout_real) {
              u32x4 val = {s0[0], s1[0], s0[1], s1[1]};
              if (be.accum) {     // kernel-uniform: rounded exactly like "store the result, then add the two tensors"
                const u32x4 prev = *reinterpret_cast<const u32x4 *>(dst + c8);
                const uint32_t a[4] = {val.x, val.y, val.z, val.w}, b[4] = {prev.x, prev.y, prev.z, prev.w};
                uint32_t r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  const float lo = __uint_as_float(a[i] << 16) + __uint_as_float(b[i] << 16);
                  const float hi = __uint_as_float(a[i] & 0xffff0000u) + __uint_as_float(b[i] & 0xffff0000u);
                  r[i] = (uint32_t)f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
                }
                val = u32x4{r[0], r[1], r[2], r[3]};
              }
              *reinterpret_cast<u32x4 *>(dst + c8) = val;
            }
          }
        }
      }
      goto stats;
    }
  }
  // ---- epilogue: lane (voxel vx, half h) owns channels nb*32 + 8q + 4h + {0..3}
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    int64_t p = pos_wg + row_of(rb);
    int32_t orow = v.out_row ? v.out_row[p] : (p < v.n_out ? (int32_t)p : -1);
    if (orow < 0) continue;
    T *dst = out + (int64_t)orow * cout_real;
    const float rs = (out_f32 && row_scale) ? row_scale[orow] : 1.f;
#pragma unroll
    for (int nb = 0; nb < NCB; ++nb) {
      if (nb_w + nb >= nb_total) continue;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        int c0 = (nb_w + nb) * 32 + 8 * q + 4 * h;
        if (c0 >= cout_real) continue;
        float o0 = acc[rb][nb][4 * q + 0], o1 = acc[rb][nb][4 * q + 1], o2 = acc[rb][nb][4 * q + 2],
              o3 = acc[rb][nb][4 * q + 3];
        if (bias) { o0 += bias[c0]; o1 += bias[c0 + 1]; o2 += bias[c0 + 2]; o3 += bias[c0 + 3]; }
        if constexpr (EPI == 0) {
          if (be.accum) {   // kernel-uniform.  The sum is rounded exactly like "store the result, then add the two tensors"
            float prev[4];
            load4(dst + c0, prev);
            o0 = stored_value<T>(o0) + prev[0]; o1 = stored_value<T>(o1) + prev[1];
            o2 = stored_value<T>(o2) + prev[2]; o3 = stored_value<T>(o3) + prev[3];
          }
        }
        if (out_f32) {  // CLIP similarity: fp32 output, per-row scale (1/|f|)
          *reinterpret_cast<float4 *>(out_f32 + (int64_t)orow * cout_real + c0) = make_float4(o0 * rs, o1 * rs, o2 * rs, o3 * rs);
        } else if constexpr (EPL == 4) {
          *reinterpret_cast<float4 *>(dst + c0) = make_float4(o0, o1, o2, o3);
        } else {
          uint2 pk;
          pk.x = (uint32_t)f32_to_bf16(o0) | ((uint32_t)f32_to_bf16(o1) << 16);
          pk.y = (uint32_t)f32_to_bf16(o2) | ((uint32_t)f32_to_bf16(o3) << 16);
          *reinterpret_cast<uint2 *>(dst + c0) = pk;
        }
      }
    }
  }
stats:
  if constexpr (BN) {
    if (be.partial != nullptr) {   // kernel-uniform
      // ---- BatchNorm statistics of this workgroup's rows.  Lane (vx, h) holds, per row block, the 16 NCB channels
      // nb*32 + 8q + 4h + i of voxel vx: sum the row blocks in registers, then a HALVING butterfly over the 32 lanes of a
      // half wave (step k: a lane keeps one half of its values and adds the partner's copy of that half) -- V values cost
      // ~V shuffles instead of 5 V -- leaves every lane with NCB finished column sums; the WM waves are folded through
      // the (now idle) weight LDS in wave order, i.e. deterministically.
      constexpr int V = 32 * NCB;              // [stat][nb][r]: 16 NCB sums + 16 NCB sums of squares
      float vst[V];
#pragma unroll
      for (int j = 0; j < V; ++j) vst[j] = 0.f;
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) {
        const int64_t p = pos_wg + row_of(rb);
        const int32_t orow = v.out_row ? v.out_row[p] : (p < v.n_out ? (int32_t)p : -1);
        const bool live = orow >= 0;
#pragma unroll
        for (int nb = 0; nb < NCB; ++nb) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c0 = (nb_w + nb) * 32 + 8 * q + 4 * h;
            float pv[4] = {0.f, 0.f, 0.f, 0.f};
            if (be.pivot && c0 < cout_real) { const float4 t4 = *reinterpret_cast<const float4 *>(be.pivot + c0); pv[0] = t4.x; pv[1] = t4.y; pv[2] = t4.z; pv[3] = t4.w; }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              float o = acc[rb][nb][4 * q + i];
              if (bias && c0 + i < cout_real) o += bias[c0 + i];
              const float d = (live && c0 < cout_real) ? stored_value<T>(o) - pv[i] : 0.f;
              vst[nb * 16 + 4 * q + i] += d;
              vst[16 * NCB + nb * 16 + 4 * q + i] += d * d;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const int n = V >> k;                  // values held before this step
        const bool up = (vx >> k) & 1;         // this lane keeps the upper half
#pragma unroll
        for (int i = 0; i < n / 2; ++i) {
          const float keep = up ? vst[n / 2 + i] : vst[i];
          const float send = up ? vst[i] : vst[n / 2 + i];
          vst[i] = keep + __shfl_xor(send, 1 << k);
        }
      }
      // lane (vx, h) now holds original indices j = sum_k bit_k(vx) * (V >> (k+1)) + t, t < NCB
      __syncthreads();                         // every wave is done with the weight LDS
      float *stage = reinterpret_cast<float *>(&lds[0][0]);     // [WM][2][WB*32]
      constexpr int CT = WB * 32;
      int jbase = 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) jbase += ((vx >> k) & 1) * (V >> (k + 1));
#pragma unroll
      for (int t = 0; t < NCB; ++t) {
        const int j = jbase + t, st = j / (16 * NCB), jj = j % (16 * NCB), nb = jj / 16, r = jj % 16;
        const int cl = (wn * NCB + nb) * 32 + 8 * (r >> 2) + 4 * h + (r & 3);       // channel inside the workgroup's tile
        stage[(wm * 2 + st) * CT + cl] = vst[t];
      }
      __syncthreads();
      for (int e = tid; e < 2 * CT; e += NT) {
        const int st = e / CT, cl = e % CT, ch = nb_wg * 32 + cl;
        if (ch < cout_real) {
          float sum = 0.f;
#pragma unroll
          for (int w = 0; w < WM; ++w) sum += stage[(w * 2 + st) * CT + cl];
          be.partial[((int64_t)tile * 2 + st) * cout_real + ch] = sum;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------ host side

// What the packed image and the grid need of a row of LGS_GATHER_TABLE (TILE and CLIP rows): chunks per weight slab, column
// blocks and positions per workgroup; lean = the tile has instances without the statistics epilogue.
struct GatherCfg { int id, sc, wb, tm; bool lean; };   // tm = positions per workgroup tile
constexpr GatherCfg tile_of(int id, bool kF32) {
#define LGS_TILE(ID, RB, NCB, WM, WN, SC, D, BF16, LEAN, BUILT) if (id == ID) return {ID, SC, WN * NCB, WM * RB * 32, LEAN && !kF32};
#define LGS_CLIP(ID, RB, NCB, WM, WN, SC, D) if (id == ID) return {ID, SC, WN * NCB, WM * RB * 32, false};
  LGS_GATHER_TABLE(LGS_TILE, LGS_NO_ROW, LGS_CLIP)
#undef LGS_TILE
#undef LGS_CLIP
  return {id, 2, 8, 256, false};   // 17: k_conv_wide, on the image of tile 16
}

// Tile choice: 256 positions x up to 128 channels when the map fills the chip, otherwise 128-position x 64-channel
// tiles, one 32 x 64 block per wave (coarse levels: few rows, many channels).
template <typename T>
int gather_id(const View &v, int nb_total) {
  constexpr bool kF32 = (sizeof(T) == 4);
  if (v.n_pad >= 256 * 256) {
    // 5..7 blocks (e.g. the 200 classes / 200 CLIP anchors = 7 blocks): one 128-position tile spans ALL output
    // channels, so the [N, C] feature matrix is streamed exactly once (dense GEMM with a small N)
    if (nb_total >= 5 && nb_total <= 7 && v.nbr == nullptr && tune(T_HEAD_TILE) == 0) return 6;
    if (nb_total == 1) return 0;
    if (nb_total == 2) return 1;
    if (nb_total == 3 || (nb_total % 3 == 0 && nb_total % 4 != 0)) return 2;
    // wide outputs (>= 256 channels, e.g. the 512-d CLIP representation model): id 17 = the 2-D blocked LDS-DMA kernel of
    // lgs_conv_wide.hip (round 3; L0 512 -> 512: 9.4 ms); id 16 = eight waves of 32 positions x 256 channels on this kernel
    // (round 2: 12.0 ms; still what 1x1 layers below 512 output channels and CONV_WIDE=0 take)
    if (!kF32 && tune(T_CONV_WIDE) != 0 && (nb_total % 8 == 0 || nb_total >= 16) && !(v.KS == 1 && v.nbr == nullptr && nb_total < 16))
      return 17;
    if (!kF32 && nb_total % 8 == 0) return 16;
    // bf16: 128-position tiles, 4 column blocks per wave.  The main loop needs 137 - 147 registers: three waves per SIMD, i.e. three
    // workgroups per CU; the 204 registers and two workgroups recorded here before were the BatchNorm statistics epilogue's, which
    // only the instance of a launch that writes statistics carries now (k_conv_gather's BN flag, CONV_LEAN_EPI)
    return kF32 ? 3 : 7;
  }
  if (nb_total == 1) return 4;
  if (kF32) return 5;
  const int small_override = (int)tune(T_SMALL_CFG);  // tuning knob
  if (small_override == 5 || (small_override >= 9 && small_override <= 13)) return small_override;
  if ((small_override == 3 || small_override == 7) && nb_total % 4 == 0) return small_override;
  // 3^3 maps of 16 k+ positions with 256 output channels (level 3 of the 8-scene batch): 128 positions x 128 channels per workgroup
  // gathers every row half as often as the 64-channel tile (stand-alone 256 -> 256 at 19.6 k rows: 0.127 vs 0.147 ms; the other
  // coarse shapes -- level 3 128 -> 128, level 4 256 -> 256 at 5 k rows -- are faster on the small tile, r04_experiments.txt)
  if (nb_total == 8 && v.KS > 1 && v.n_pad >= 16384) return 7;
  return 8;   // measured best on the other L3/L4 shapes (tools/microbench.py coarse): 128 positions x 64 channels
}

// out = p0 + p1 + p2 (+ bias), fixed order; 4 elements per thread
template <typename T>
__global__ void k_sum_partials(const float *__restrict__ part, int64_t n4, int64_t zstride, const float *__restrict__ bias,
                               int cout, T *__restrict__ out, int accum) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float4 a = reinterpret_cast<const float4 *>(part)[i];
  const float4 b = reinterpret_cast<const float4 *>(part + zstride)[i];
  const float4 c = reinterpret_cast<const float4 *>(part + 2 * zstride)[i];
  float o0 = a.x + b.x + c.x, o1 = a.y + b.y + c.y, o2 = a.z + b.z + c.z, o3 = a.w + b.w + c.w;
  if (bias) { const int c0 = (int)((i * 4) % cout); o0 += bias[c0]; o1 += bias[c0 + 1]; o2 += bias[c0 + 2]; o3 += bias[c0 + 3]; }
  if (accum) {
    float prev[4];
    load4(out + 4 * i, prev);
    o0 = stored_value<T>(o0) + prev[0]; o1 = stored_value<T>(o1) + prev[1];
    o2 = stored_value<T>(o2) + prev[2]; o3 = stored_value<T>(o3) + prev[3];
  }
  if constexpr (sizeof(T) == 4) {
    reinterpret_cast<float4 *>(out)[i] = make_float4(o0, o1, o2, o3);
  } else {
    uint2 pk;
    pk.x = (uint32_t)f32_to_bf16(o0) | ((uint32_t)f32_to_bf16(o1) << 16);
    pk.y = (uint32_t)f32_to_bf16(o2) | ((uint32_t)f32_to_bf16(o3) << 16);
    reinterpret_cast<uint2 *>(out)[i] = pk;
  }
}

constexpr int64_t kSplitMaxBytes = 16ll << 20;   // fp32 partial images of the slot split (larger ones cost more than the split gains)

// ------------------------------------------------------------------------------------ the launch plan
// Everything a forward / dgrad launch decides on the host, computed ONCE by conv_plan() from the view, the channel counts, the
// kernel instance, the requested epilogue and the tuning table: which kernel runs, its tile and grid, the layout of the packed
// weight image, whether the launch takes the slot split, and where every piece of the workspace lies.  The op, the launcher and
// every public query (workspace size, statistic rows, pack descriptor, accumulate) read this struct and nothing else, so they
// cannot disagree.  It is the plan part of lgs_conv_plan_info, which lgs_debug_conv_plan hands out as it stands.
using ConvPlan = lgs_conv_plan_info;
enum ConvPath { kPathEmpty = 0, kPathPointwise = 1, kPathPointwiseF32 = 2, kPathWide = 3, kPathGather = 4 };
// requested epilogue: BatchNorm statistics and accumulation exist on k_conv_gather only (they keep a 1x1 layer off the pointwise
// kernels); kEpiF32Out = fp32 output with a row scale (the CLIP similarity), which also never splits
enum ConvEpi { kEpiNone = 0, kEpiBnStats = 1, kEpiAccum = 2, kEpiF32Out = 3 };

// layout of a packed weight image: K matrices of nc x nb_total 32 x 32 blocks, rounded up to whole slabs and column tiles
inline void plan_image(ConvPlan &p, const GatherCfg &cfg, int K, int g_real, int o_real, int wld) {
  p.tile_id = cfg.id; p.sc = cfg.sc; p.wb = cfg.wb; p.tm = cfg.tm;
  p.nc = pad32(g_real) / 32; p.nb_total = pad32(o_real) / 32;
  p.ncp = (p.nc + cfg.sc - 1) / cfg.sc * cfg.sc;
  p.nbp = (p.nb_total + cfg.wb - 1) / cfg.wb * cfg.wb;
  p.wld = wld;
  p.total = (int64_t)K * p.ncp * p.nbp * wld * 64;
}

// T = storage type of the tensors, TK = the kernel instance that multiplies them (TK = f32s_t: fp32 tensors, split-bf16 products).
// Pure: no HIP call, no table of the view is read.
template <typename T, typename TK = T>
ConvPlan conv_plan(const View &v, int K, int g_real, int o_real, ConvEpi epi, int64_t in_ld = 0) {
  constexpr int EPL = Tr<T>::EPL;
  ConvPlan p = {};
  plan_image(p, tile_of(gather_id<TK>(v, pad32(o_real) / 32), sizeof(TK) == 4), K, g_real, o_real, Tr<TK>::WLD);
  // channel groups of the reduction (see the kernel): rows wider than 8 chunks (256 channels) are walked in 4-chunk groups
  p.gc = p.nc > 8 ? 4 : p.nc;
  p.bytes_total = 256;             // never an empty buffer: the entry points insist on a workspace pointer
  if (v.n_pad == 0) return p;      // the maps of an empty batch: no row to write, nothing is packed
  p.pad_input = g_real % EPL != 0;      // e.g. the 3-channel colour input of conv0p1s1: rows padded to one 16-byte piece
  p.scratch_out = o_real % 4 != 0;      // rows are written in 4-channel groups: odd widths go through a 4-aligned scratch image
  p.packed_ext_ok = !p.pad_input && !p.scratch_out;     // a caller-owned packed image (and a strided input) can be used
  // 1x1 layers of the big maps: streaming GEMMs with persistent workgroups (lgs_pointwise.hip), no packed image, no workspace;
  // fp32 on the exact-fp32 MFMA, whichever instance multiplies the 3^3 layers
  const int64_t ld = in_ld > 0 ? in_ld : g_real;
  if (epi == kEpiNone && std::is_same<TK, bf16_t>::value && pointwise_supported(v, K, g_real, o_real, ld)) { p.path = kPathPointwise; return p; }
  if (epi == kEpiNone && std::is_same<T, float>::value && o_real % 4 == 0 && pointwise_f32_supported(v, K, g_real, o_real, ld)) { p.path = kPathPointwiseF32; return p; }
  p.path = p.tile_id == 17 ? kPathWide : kPathGather;
  const int o4 = (o_real + 3) / 4 * 4;
  if (p.path == kPathGather) {
    p.grid_x = v.n_pad / p.tm; p.grid_y = (p.nb_total + p.wb - 1) / p.wb;
    // Slot split: bf16 storage only.  The fp32 path is the parity mode and keeps ONE accumulator per output (a different summation
    // order moves results by ~1e-7, which BatchNorm over a handful of coarse rows with near-zero variance amplifies into
    // ReLU gate flips against the oracle -- measured on the 14A fixture).  The chip holds >= 512 of these workgroups.
    p.split = tune(T_CONV_SPLIT) != 0 && sizeof(TK) == 2 && epi != kEpiF32Out && !p.scratch_out && v.KS > 1 && K == 27 &&
              v.n_out > 0 && 3 * v.n_out * (int64_t)o_real * 4 <= kSplitMaxBytes && p.grid_x * p.grid_y < 600;
    p.grid_z = p.split ? 3 : 1;
    // rows of BatchNorm statistics the launch writes (= its position tiles): a split launch sums partial images afterwards and
    // the scratch route unpads them, neither has the statistics; the same two and the wide kernel cannot accumulate
    p.bn_rows = (p.split || p.scratch_out) ? 0 : (int)p.grid_x;
    p.can_accumulate = !p.scratch_out;
  }
  // workspace: the regions in the order they are taken, each 256-byte aligned
  int64_t used = 0;
  auto take = [&](int64_t bytes) { const lgs_conv_plan_region r = {used, align256(bytes)}; used += r.bytes; return r; };
  p.packed = take(p.total * 16);
  if (p.pad_input) p.padded_in = take(v.n_in * (int64_t)((g_real + EPL - 1) / EPL * EPL) * (int64_t)sizeof(T));
  if (p.scratch_out) {    // + the bias padded to the scratch width (e.g. the 3-channel offset head of the instance-segmentation model)
    p.scratch = take(v.n_out * (int64_t)o4 * (int64_t)sizeof(T));
    p.bias = take(4 * (int64_t)o4);
  }
  if (p.split) p.partials = take(3 * v.n_out * (int64_t)o_real * 4);
  if (used > p.bytes_total) p.bytes_total = used;
  return p;
}

// ---- instances that issue no load of a value that is zero by construction (CONV_SLAB_TRIM, CONV_ROW_TRIM)
// The image's slab length sc comes from the tile (plan_image); the kernel may walk the chunk-major image with a shorter or
// longer slab as long as it stops at chunk nc - 1.  -> chunks per slab of the instance to run, 0 = the tile's own instance.
// Only a single reduction group of at most 8 chunks (gc == nc) is trimmed, and only on the big-map bf16 tiles 0, 1, 2 and 7,
// whose step shapes fetch zero chunks today: 32 -> 32 and 3 -> 32 (nc 1 on sc 4), 64 -> 64 (2 on 4), 96 -> 96 (3 on 4) and
// the 96 -> 128 dgrad (3 on sc 2: two slabs of 2).
inline int trimmed_slab(int tile_id, int sc, int nc, int gc) {
  const int64_t knob = tune(T_CONV_SLAB_TRIM);
  if (knob == 0 || gc != nc || nc > 8 || !(tile_id <= 2 || tile_id == 7)) return 0;
  if (nc < sc) return nc;
  // tile 7 walks three chunks on 2-chunk slabs: ONE slab of three, or with the knob at 2 three slabs of one.  Two slabs of three in
  // LDS are 62 KB, which fits twice per CU: the instance with the statistics epilogue (two per CU by its registers anyway) keeps
  // them, the one without holds ONE slab (ONEBUF, 38 KB) and runs three per CU.  Level-0 96 -> 128 dgrad, stand-alone: 692 us with
  // the epilogue, 638 us one slab of three at three per CU, 647 us three slabs of one at four (profiles/conv_lean_epilogue.txt)
  if (tile_id == 7 && nc == 3) return knob == 2 ? 1 : 3;
  if (nc % sc == 0) return 0;              // whole slabs: nothing to trim
  for (int d = sc - 1; d > 1; --d)         // the largest divisor of nc below sc; none (5, 7): the tile's own instance
    if (nc % d == 0) return d;
  return 0;
}
// ---- which row of the instance table a launch runs
// scl = chunks per slab of the walk, 0 = the tile's own instance on the image's slabs; row1 = the one-piece-row walk;
// bn = the instance with the statistics epilogue; onebuf = one weight slab in LDS
struct GatherInstance { int tile_id, scl; bool row1, bn, onebuf; };
constexpr bool walk_onebuf(int id, int scl, bool row1) {
#define LGS_WALK(ID, RB, NCB, WM, WN, SC, D, SCL, ROW1, ONEBUF, OCC) if (id == ID && scl == SCL && row1 == ROW1) return ONEBUF;
  LGS_GATHER_TABLE(LGS_NO_ROW, LGS_WALK, LGS_NO_ROW)
#undef LGS_WALK
  return false;
}
// THE choice, from the plan, the row width the launch gathers, whether it writes statistics and the tuning table.  Pure, like
// conv_plan(); it picks an instance and never a plan.
// Epilogue: on the bf16 tiles that have both variants (the big-map tiles 0, 1, 2, 6, 7, 16 and their walks) a launch that writes no
// statistics runs the instance built without them (every dgrad, every forward without `partial`); CONV_LEAN_EPI=0, the fp32
// instances and the small-map tiles (whose registers the epilogue does not set: within 4 either way) run the one with them.
// Tile 7 decides per launch: its lean instances hold three workgroups per CU instead of two, which a grid of at most two per CU
// cannot use -- level 3 of the 8-scene batch (256 -> 256, 308 workgroups) measured 1 % SLOWER on them and keeps the instance it
// had; 128 -> 128 at level 2 (633) gains 14 %, the 96 -> 128 dgrad 6 - 13 % (profiles/conv_lean_epilogue.txt section 2).
// Walk: trimmed_slab(); rows of one 16-byte piece (conv0: 3 colour channels padded to 8) take the walk whose second gather of a
// chunk, out of range in every lane, is not issued.  The 3-chunk walk of tile 7 keeps one slab in LDS where it has no epilogue.
template <typename T>
GatherInstance gather_instance(const ConvPlan &pl, int cin_real, bool statistics) {
  GatherInstance g = {pl.tile_id, 0, false, true, false};
  if (sizeof(T) == 4) return g;
  constexpr int64_t kTwoPerCu = 2 * 256;
  const int64_t lean = tune(T_CONV_LEAN_EPI);
  g.bn = !(tile_of(pl.tile_id, false).lean && !statistics && lean != 0 &&
           (pl.tile_id != 7 || pl.grid_x * pl.grid_y * pl.grid_z > kTwoPerCu || lean == 2));
  g.scl = trimmed_slab(pl.tile_id, pl.sc, pl.nc, pl.gc);
  g.row1 = g.scl == 1 && pl.tile_id == 0 && cin_real <= Tr<T>::EPL && tune(T_CONV_ROW_TRIM) != 0;
  g.onebuf = !g.bn && walk_onebuf(g.tile_id, g.scl, g.row1);
  return g;
}

constexpr int kLdsPerCu = 160 * 1024;
constexpr int gather_lds_bytes(int tm, int wb, int wld, int scl, int slabs = 2) { return slabs * scl * wb * wld * 64 * 16 + 27 * tm * 4; }
// an instance BUILT for a number of workgroups per CU (gather_waves_per_simd) must also fit that often in the CU's LDS
template <typename T, int RB, int NCB, int WM, int WN, int SC, int D, int SCL, bool ONEBUF = false>
constexpr bool lean_residency_fits() {
  constexpr int w = gather_waves_per_simd<T, RB, NCB, WM, WN, SC, D, 0, SCL, false, ONEBUF>();
  return w == 0 || (WM * WN == 4 && gather_lds_bytes(WM * RB * 32, WN * NCB, Tr<bf16_t>::WLD, SCL, ONEBUF ? 1 : 2) * w <= kLdsPerCu);
}

// ---- the dispatch: the kernel of the row `g` names -> f(GatherKernel<...>(), launch-site text).  The site names tile and walk,
// not the epilogue variant ("k_conv_gather<T,...>", a walk with "SlabWalk<SCL,ROW1>::" in front, as tests and profiles know
// them).  EPI = 0: the convolution rows, fp32 instances of the tiles that have one; EPI = 1: the CLIP rows.
template <typename T, int RB, int NCB, int WM, int WN, int SC, int D, int EPI, int SCL, bool ROW1, bool BN, bool ONEBUF>
struct GatherKernel {
  static constexpr auto fn = &k_conv_gather<T, RB, NCB, WM, WN, SC, D, EPI, SCL, ROW1, BN, ONEBUF>;
  static constexpr int rb = RB, ncb = NCB, wm = WM, wn = WN, sc = SC, d = D, threads = WM * WN * 64;
};
#define LGS_SITE(...) #__VA_ARGS__
template <typename T, int EPI = 0, typename F>
int with_gather_kernel(const GatherInstance &g, F &&f) {
  constexpr bool kF32 = (sizeof(T) == 4);
#define LGS_TILE(ID, RB, NCB, WM, WN, SC, D, BF16, LEAN, BUILT)                                                              \
  if constexpr (EPI == 0 && !(BF16 && kF32))                                                                               \
    if (g.tile_id == ID && g.scl == 0) {                                                                                   \
      constexpr const char *site = LGS_SITE(k_conv_gather<T, RB, NCB, WM, WN, SC, D>);                                      \
      if constexpr (LEAN && !kF32) {                                                                                       \
        static_assert(lean_residency_fits<T, RB, NCB, WM, WN, SC, D, SC>(), "the lean instance is built for more workgroups than its LDS admits"); \
        if (!g.bn) return f(GatherKernel<T, RB, NCB, WM, WN, SC, D, 0, SC, false, false, false>(), site);                   \
      }                                                                                                                    \
      LGS_REQUIRE(g.bn, "k_conv_gather: this tile has no instance without the statistics epilogue (internal error)");       \
      return f(GatherKernel<T, RB, NCB, WM, WN, SC, D, 0, SC, false, true, false>(), site);                                 \
    }
#define LGS_WALK(ID, RB, NCB, WM, WN, SC, D, SCL, ROW1, ONEBUF, OCC)                                                         \
  if constexpr (EPI == 0 && !kF32)                                                                                         \
    if (g.tile_id == ID && g.scl == SCL && g.row1 == ROW1) {                                                               \
      static_assert(gather_lds_bytes(WM * RB * 32, WN * NCB, Tr<bf16_t>::WLD, SCL) * OCC <= kLdsPerCu, "the slab walk costs the tile occupancy"); \
      static_assert(lean_residency_fits<T, RB, NCB, WM, WN, SC, D, SCL, ONEBUF>(), "the lean instance is built for more workgroups than its LDS admits"); \
      constexpr const char *site = LGS_SITE(SlabWalk<SCL, ROW1>::k_conv_gather<T, RB, NCB, WM, WN, SC, D>);                 \
      return g.bn ? f(GatherKernel<T, RB, NCB, WM, WN, SC, D, 0, SCL, ROW1, true, false>(), site)                           \
                  : f(GatherKernel<T, RB, NCB, WM, WN, SC, D, 0, SCL, ROW1, false, ONEBUF>(), site);                        \
    }
#define LGS_CLIP(ID, RB, NCB, WM, WN, SC, D)                                                                                \
  if constexpr (EPI == 1)                                                                                                  \
    if (g.tile_id == ID)                                                                                                   \
      return f(GatherKernel<T, RB, NCB, WM, WN, SC, D, 1, SC, false, false, false>(), LGS_SITE(k_conv_gather<T, RB, NCB, WM, WN, SC, D, 1>));
  LGS_GATHER_TABLE(LGS_TILE, LGS_WALK, LGS_CLIP)
#undef LGS_TILE
#undef LGS_WALK
#undef LGS_CLIP
  LGS_REQUIRE(false, "k_conv_gather: no such instance (tile " + std::to_string(g.tile_id) + ", " + std::to_string(g.scl) + "-chunk walk)");
}
// the launch of kernel `k` of the table, counted at `site_text` under the template bindings of the calling function (`pretty`)
#define LGS_GATHER_LAUNCH(k, site_text, pretty, ...)                                                                       \
  do {                                                                                                                     \
    static const int _lgs_site = lgs::dispatch_site(site_text, pretty);                                                    \
    lgs::dispatch_hit(_lgs_site);                                                                                          \
    hipLaunchKernelGGL(decltype(k)::fn, __VA_ARGS__);                                                                      \
  } while (0)

template <typename T>
int launch_gather(const View &v, const ConvPlan &pl, const T *in, int cin_real, const uint4 *wp, int K, T *out, int cout_real,
                  const float *bias, hipStream_t s, float *out_f32 = nullptr, const float *row_scale = nullptr,
                  float *zpartial = nullptr, const BnEpi *bn = nullptr, int in_ld = 0) {
  if (v.n_pad == 0) return 0;
  const int nc = pl.nc, nb_total = pl.nb_total, ncp = pl.ncp, nbp = pl.nbp, gc = pl.gc;
  const uint64_t in_bytes64 = (uint64_t)v.n_in * (uint64_t)(in_ld > 0 ? in_ld : cin_real) * sizeof(T);
  const uint64_t w_bytes64 = (uint64_t)pl.total * 16;
  LGS_REQUIRE(in_bytes64 < 0xfffff000ull && w_bytes64 < 0xfffff000ull,
              "sparse conv: a feature or weight tensor of 4 GiB or more is beyond the 32-bit buffer-descriptor path");
  const unsigned in_bytes = (unsigned)in_bytes64, w_bytes = (unsigned)w_bytes64;
  if (pl.path == kPathWide) {
    LGS_REQUIRE(sizeof(T) == 2 && !out_f32 && !row_scale && !(bn && bn->partial), "wide conv: bf16 feature output only (internal error)");
    LGS_REQUIRE(!(bn && bn->accum), "wide conv: no accumulating epilogue (lgs_conv_dgrad_can_accumulate says so)");
    return launch_conv_wide(v, in, cin_real, in_ld > 0 ? in_ld : cin_real, wp, nb_total, ncp, nbp, K, out, cout_real, bias,
                            gc >= nc ? 0 : (gc + 1) / 2, s);
  }
  // a slot-split launch writes fp32 partial images: bias and accumulation happen in k_sum_partials, statistics not at all
  const bool split = pl.split;
  LGS_REQUIRE(!split || zpartial, "sparse conv: a split launch without its partial images (internal error)");
  const int64_t zstride = v.n_out * (int64_t)cout_real;
  const BnEpi be = (bn && !split) ? *bn : BnEpi();
  const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y, (unsigned)pl.grid_z);
  // both epilogue variants are counted at the same launch site, the lean ones by a counter of their own
  const GatherInstance g = gather_instance<T>(pl, cin_real, be.partial != nullptr);
  if (!g.bn) LGS_COUNT("k_conv_gather:no_statistics_epilogue");
  const char *const here = __PRETTY_FUNCTION__;
  const int rc = with_gather_kernel<T>(g, [&](auto k, const char *site) {
    LGS_GATHER_LAUNCH(k, site, here, grid, dim3(k.threads), 0, s, v, in, cin_real, nc, reinterpret_cast<const u32x4 *>(wp), nb_total, ncp, nbp,
                      out, cout_real, split ? nullptr : bias, split ? zpartial : out_f32, row_scale, in_bytes, w_bytes, zstride, ClipEpi(), be,
                      gc, in_ld > 0 ? in_ld : cin_real);
    return 0;
  });
  if (rc) return rc;
  if (split) {
    const int64_t n4 = zstride / 4;
    if (n4 > 0) LGS_KLAUNCH((k_sum_partials<T>), (unsigned)((n4 + 255) / 256), 256, 0, s, zpartial, n4, zstride, bias, cout_real, out,
                                   (bn && bn->accum) ? 1 : 0);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

// what launch_gather<T> would run and count for this plan (lgs_debug_conv_gather_instance): the choice, the numbers of its row,
// the launch site by its registered name -- the function's only template binding is T, as launch_gather's
template <typename T>
int describe_gather(const ConvPlan &pl, int cin_real, bool statistics, lgs_conv_gather_instance *out) {
  const GatherInstance g = gather_instance<T>(pl, cin_real, statistics);
  const char *const here = __PRETTY_FUNCTION__;
  return with_gather_kernel<T>(g, [&](auto k, const char *site) {
    *out = {g.tile_id, g.scl, g.row1, g.bn, g.onebuf, k.rb, k.ncb, k.wm, k.wn, k.sc, k.d, {0}};
    snprintf(out->site, sizeof(out->site), "%s", dispatch_site_name(site, here).c_str());
    return 0;
  });
}

template <typename T, typename TK = T>
int conv_gather_op(const View &v, const void *in_v, int g_real, const float *weight, int K, int cin_w, int cout_w,
                   int transposed_w, int o_real, const float *bias, void *out_v, void *workspace, hipStream_t s,
                   const BnEpi *bn = nullptr, void *packed_ext = nullptr, int pack_mode = 0, int in_ld = 0) {
  constexpr int EPL = Tr<T>::EPL;
  const ConvPlan pl = conv_plan<T, TK>(v, K, g_real, o_real, !bn ? kEpiNone : bn->accum ? kEpiAccum : kEpiBnStats, in_ld);
  const int64_t ld = in_ld > 0 ? in_ld : g_real;
  if (pl.path == kPathEmpty) return 0;
  if (pl.path == kPathPointwise) return launch_pointwise(v, in_v, ld, g_real, weight, cin_w, cout_w, transposed_w, o_real, bias, out_v, s);
  LGS_REQUIRE(in_ld == 0 || in_ld == g_real || (pl.packed_ext_ok && in_ld > g_real && (in_ld * (int)sizeof(T)) % 16 == 0),
              "sparse conv: a strided input needs 16-byte aligned rows and channel counts on the 16-byte grid");
  if (pl.path == kPathPointwiseF32) return launch_pointwise_f32(v, in_v, ld, g_real, weight, cin_w, cout_w, transposed_w, o_real, bias, out_v, s);
  char *ws = reinterpret_cast<char *>(workspace);
  T *out = reinterpret_cast<T *>(out_v);
  int o_launch = o_real;
  if (pl.scratch_out) {     // (statistics, accumulation and a caller's packed image do not exist on this route)
    out = reinterpret_cast<T *>(ws + pl.scratch.offset);
    o_launch = (o_real + 3) / 4 * 4;
    bn = nullptr;
    if (v.n_out > 0) LGS_HIP(hipMemsetAsync(out, 0, (size_t)v.n_out * o_launch * sizeof(T), s));
    if (bias) {
      float *bp = reinterpret_cast<float *>(ws + pl.bias.offset);
      LGS_HIP(hipMemsetAsync(bp, 0, sizeof(float) * o_launch, s));
      LGS_HIP(hipMemcpyAsync(bp, bias, sizeof(float) * o_real, hipMemcpyDeviceToDevice, s));
      bias = bp;
    }
  }
  const T *in = reinterpret_cast<const T *>(in_v);
  int g_stride = g_real;
  if (pl.pad_input) {
    // rows are padded to ONE 16-byte piece multiple (3 -> 8 bf16 / 4 fp32 channels), not to the 32-channel chunk: the
    // pieces beyond the row are masked by the gather's channel-tail test, so neighbours cost 16 instead of 64 bytes
    T *padded = reinterpret_cast<T *>(ws + pl.padded_in.offset);
    g_stride = (g_real + EPL - 1) / EPL * EPL;
    const int64_t tot = v.n_in * g_stride;
    if (tot > 0) LGS_KLAUNCH((k_pad_rows<T>), (unsigned)((tot + 255) / 256), 256, 0, s, in, v.n_in, g_real, g_stride, padded);
    in = padded;
  }
  // packed_ext: a caller-owned image of exactly this layout (lgs_conv_pack_desc); pack_mode 2 = it is up to date
  const bool ext = packed_ext && pl.packed_ext_ok;
  uint4 *wp = ext ? reinterpret_cast<uint4 *>(packed_ext) : reinterpret_cast<uint4 *>(ws + pl.packed.offset);
  if (!ext || pack_mode != 2)
    LGS_KLAUNCH((k_pack_weights<TK>), (unsigned)((pl.total + 255) / 256), 256, 0, s, weight, K, cin_w, cout_w, transposed_w,
                       v.mirror, g_real, o_real, pl.ncp, pl.nbp, wp);
  LGS_HIP(hipGetLastError());
  int rc = launch_gather<TK>(v, pl, reinterpret_cast<const TK *>(in), g_stride, wp, K, reinterpret_cast<TK *>(out), o_launch, bias, s, nullptr,
                            nullptr, pl.split ? reinterpret_cast<float *>(ws + pl.partials.offset) : nullptr, bn,
                            (in_ld > g_real && !pl.pad_input) ? in_ld : 0);
  if (rc || !pl.scratch_out) return rc;
  const int64_t tot = v.n_out * (int64_t)o_real;
  if (tot > 0)
    LGS_KLAUNCH((k_unpad_rows<T>), (unsigned)((tot + 255) / 256), 256, 0, s, out, v.n_out, o_real, o_launch, reinterpret_cast<T *>(out_v));
  LGS_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------ CLIP contraction
// S = normalize(F) . normalize(T)^T is the 1x1 "convolution" of the voxel features with the
// normalised text anchors as the weight matrix, scaled per row by 1/|f|: it reuses the MFMA gather
// kernel with the identity view.  (ContrastiveLanguageLoss.py:73-95, lib/losses/utils.py:80-103)
template <typename T>
__global__ void k_row_invnorm(const T *__restrict__ f, int64_t n, int c, float *__restrict__ inv) {
  // one wavefront per row
  int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int lane = threadIdx.x & 63;
  if (row >= n) return;
  float s = 0.f;
  for (int ch = lane; ch < c; ch += 64) { float x = ld_elem(f + row * c + ch); s += x * x; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) inv[row] = 1.f / fmaxf(sqrtf(s), 1e-12f);
}
__global__ void k_normalize_anchors(const float *__restrict__ a, int na, int c, float *__restrict__ out) {
  int row = blockIdx.x;
  int lane = threadIdx.x;
  if (row >= na) return;
  float s = 0.f;
  for (int ch = lane; ch < c; ch += 64) { float x = a[(int64_t)row * c + ch]; s += x * x; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  float inv = 1.f / fmaxf(sqrtf(s), 1e-12f);
  for (int ch = lane; ch < c; ch += 64) out[(int64_t)row * c + ch] = a[(int64_t)row * c + ch] * inv;
}

// room for the packed anchor image of the CLIP launches: what lgs_clip_workspace_bytes / lgs_clip_loss_workspace_bytes promise the
// caller (who does not know the tile yet) and what the launches check their image against
inline int64_t clip_image_room(int c, int n_anchor, int dtype) {
  return align256((int64_t)(pad32(c) + 96) * (pad32(n_anchor) + 96) * esize(dtype));
}
inline int64_t clip_loss_image_room(int c, int dtype) {   // <= (nc + 7) chunks x 7 blocks
  return align256((int64_t)(pad32(c) + 256) * 256 * esize(dtype));
}

template <typename T>
int clip_similarity_t(const void *feat, int64_t n, int c, const float *anchors, int na, float *sim, float *inv_norm_f,
                      void *workspace, hipStream_t s) {
  constexpr int dtype = sizeof(T) == 2 ? LGS_BF16 : LGS_F32;
  LGS_REQUIRE(c % Tr<T>::EPL == 0, "lgs_clip_similarity: feature dim must be a multiple of the 16-byte load width");
  LGS_REQUIRE(na % 4 == 0, "lgs_clip_similarity: anchor count must be a multiple of 4");
  if (n == 0) return 0;
  char *ws = reinterpret_cast<char *>(workspace);
  float *tn = reinterpret_cast<float *>(ws);
  uint4 *wp = reinterpret_cast<uint4 *>(ws + align256((int64_t)na * c * 4));
  const T *f = reinterpret_cast<const T *>(feat);
  LGS_KLAUNCH(k_normalize_anchors, na, 64, 0, s, anchors, na, c, tn);
  View v;
  v.n_pad = pad_rows(n); v.n_out = n; v.n_in = n; v.KS = 1; v.K = 1;
  const ConvPlan pl = conv_plan<T>(v, 1, c, na, kEpiF32Out);
  LGS_REQUIRE(pl.total * 16 <= clip_image_room(c, na, dtype),
              "lgs_clip_similarity: the packed anchor image is larger than its workspace region (SMALL_CFG 12 / 13 on a narrow feature)");
  // T^[a][c] read as w[o = a][g = c]  ("transposed" form of the packer with cin_w = na, cout_w = c)
  LGS_KLAUNCH((k_pack_weights<T>), (unsigned)((pl.total + 255) / 256), 256, 0, s, tn, 1, na, c, 1, 0, c, na, pl.ncp, pl.nbp, wp);
  LGS_KLAUNCH((k_row_invnorm<T>), (unsigned)((n * 64 + 255) / 256), 256, 0, s, f, n, c, inv_norm_f);
  LGS_HIP(hipGetLastError());
  return launch_gather<T>(v, pl, f, c, wp, 1, (T *)nullptr, na, nullptr, s, sim, inv_norm_f);
}

// Fused CLIP loss forward: one launch of the EPI = 1 instance.  The wave owns whole rows (all anchor columns), so
// the anchor count is limited to 7 column blocks (224); the 200 ScanNet200 anchors use the 7-block tile.
template <typename T>
int clip_loss_forward_t(const void *feat, int64_t n, int c, const float *anchors, int na, const ClipEpi &ce_in, float *anchors_n,
                        float *sim, void *workspace, hipStream_t s) {
  constexpr bool kF32 = (sizeof(T) == 4);
  LGS_REQUIRE(c % Tr<T>::EPL == 0, "lgs_clip_loss_forward: feature dim must be a multiple of the 16-byte load width");
  LGS_REQUIRE(na % 4 == 0 && na >= 4 && na <= 224, "lgs_clip_loss_forward: anchor count must be a multiple of 4 in [4, 224]");
  LGS_REQUIRE(ce_in.k_neg >= 1 && ce_in.k_neg <= 7, "lgs_clip_loss_forward: 1..7 negatives per row");
  if (n == 0) return 0;
  const int nb_total = pad32(na) / 32;
  const int ncb = nb_total <= 1 ? 1 : nb_total <= 2 ? 2 : nb_total <= 4 ? 4 : 7;
  ConvPlan pl = {};  // the image of the EPI = 1 instances: one column tile of ncb blocks
  plan_image(pl, tile_of(-ncb, kF32), 1, c, na, Tr<T>::WLD);
  const int nc = pl.nc, ncp = pl.ncp, nbp = pl.nbp;
  uint4 *wp = reinterpret_cast<uint4 *>(workspace);
  LGS_KLAUNCH(k_normalize_anchors, na, 64, 0, s, anchors, na, c, anchors_n);
  LGS_REQUIRE(pl.total * 16 <= clip_loss_image_room(c, kF32 ? LGS_F32 : LGS_BF16),
              "lgs_clip_loss_forward: the packed anchor image is larger than its workspace region (internal error)");
  // T^[a][c] read as w[o = a][g = c]  ("transposed" form of the packer with cin_w = na, cout_w = c)
  LGS_KLAUNCH((k_pack_weights<T>), (unsigned)((pl.total + 255) / 256), 256, 0, s, anchors_n, 1, na, c, 1, 0, c, na, ncp, nbp, wp);
  View v;
  v.n_pad = pad_rows(n); v.n_out = n; v.n_in = n; v.KS = 1; v.K = 1;
  const uint64_t in_bytes64 = (uint64_t)n * (uint64_t)c * sizeof(T), w_bytes64 = (uint64_t)pl.total * 16;
  LGS_REQUIRE(in_bytes64 < 0xfffff000ull, "lgs_clip_loss_forward: feature tensor of 4 GiB or more");
  ClipEpi ce = ce_in;
  ce.n_anchor = na;
  const T *f = reinterpret_cast<const T *>(feat);
  const dim3 grid((unsigned)(v.n_pad / pl.tm), 1);
  const char *const here = __PRETTY_FUNCTION__;
  const int rc = with_gather_kernel<T, 1>(GatherInstance{-ncb, 0, false, false, false}, [&](auto k, const char *site) {
    LGS_GATHER_LAUNCH(k, site, here, grid, dim3(k.threads), 0, s, v, f, c, nc, reinterpret_cast<const u32x4 *>(wp), nb_total, ncp, nbp,
                      (T *)nullptr, na, (const float *)nullptr, sim, (const float *)nullptr, (unsigned)in_bytes64, (unsigned)w_bytes64,
                      (int64_t)0, ce, BnEpi(), nc, c);
    return 0;
  });
  LGS_HIP(hipGetLastError());
  return rc;
}

// ---- one kernel instance per tensor dtype: f(Inst<storage type, multiplying instance>)
template <typename T, typename TK = T> struct Inst { using S = T; using M = TK; };
template <typename F>
auto with_instance(int dtype, F &&f) {
  if (dtype == LGS_BF16) return f(Inst<bf16_t>());
  if (tune(T_FP32_SPLIT) != 0) return f(Inst<float, f32s_t>());
  return f(Inst<float>());
}
inline bool known_dtype(int dtype) { return dtype == LGS_F32 || dtype == LGS_BF16; }

// the view op 0 (forward) / 1 (dgrad) walks, and its plan
inline const View &op_view(const lgs_kmap *km, int op, int transposed) { return (op == 1) == (transposed != 0) ? km->fwd : km->bwd; }
inline ConvPlan plan_of(const View &v, int K, int g_real, int o_real, int dtype, ConvEpi epi) {
  return with_instance(dtype, [&](auto i) { return conv_plan<typename decltype(i)::S, typename decltype(i)::M>(v, K, g_real, o_real, epi); });
}

// one forward / dgrad call: op 1 gathers grad_out [*, cout] and reads the weights transposed (3^3: mirrored)
inline int conv_call(lgs_kmap *km, int op, int transposed, const void *in, int cin, const float *weight, int cout, const float *bias,
                     void *out, int dtype, void *workspace, const BnEpi *bn, void *packed, int pack_mode, int in_ld, void *stream) {
  LGS_REQUIRE(!transposed || traits_of(km).transposed_ok, "transposed 3x3x3 convolution is not part of the model family");
  LGS_REQUIRE(known_dtype(dtype), "sparse conv: unknown dtype");
  const View v = op_view(km, op, transposed);   // (with its own mirror flag: set on the bwd side of a shared 3^3 stride-1 table only)
  hipStream_t s = (hipStream_t)stream;
  if (kmap_wait(km, s)) return 1;
  return with_instance(dtype, [&](auto i) {
    return conv_gather_op<typename decltype(i)::S, typename decltype(i)::M>(v, in, op == 0 ? cin : cout, weight, km->K, cin, cout, op,
                                                                           op == 0 ? cout : cin, bias, out, workspace, s, bn, packed, pack_mode, in_ld);
  });
}

}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_conv_workspace_bytes(const lgs_kmap *km, int cin, int cout, int dtype, int op) {
  if (!km) return -1;
  // the maps of an empty batch: no launch plan to size (the planners divide by range and lane counts); the entry points return
  // before they touch the workspace
  if (km->fwd.n_pad == 0 && km->bwd.n_pad == 0) return 256;
  if (op == 2) return lgs::wgrad_workspace_bytes(km, cin, cout, dtype);
  // either view (op 0 / 1 run on fwd or bwd by `transposed`), with and without the epilogue that keeps a 1x1 layer off the
  // pointwise kernels
  int64_t bytes = 0;
  for (const View *v : {&km->fwd, &km->bwd})
    for (ConvEpi e : {kEpiNone, op == 0 ? kEpiBnStats : kEpiAccum}) {
      const int64_t b = plan_of(*v, km->K, op == 0 ? cin : cout, op == 0 ? cout : cin, dtype, e).bytes_total;
      if (b > bytes) bytes = b;
    }
  return bytes;
}

// rows of BatchNorm statistics the forward launch of this shape writes, 0 if it cannot produce them
int lgs_conv_bn_partial_rows(const lgs_kmap *km, int transposed, int cout, int dtype) {
  if (!km || !known_dtype(dtype)) return 0;
  return plan_of(op_view(km, 0, transposed), km->K, cout, cout, dtype, kEpiBnStats).bn_rows;   // (the input width does not matter)
}

int lgs_conv_pack_desc(const lgs_kmap *km, int op, int transposed, int cin, int cout, int dtype, lgs_pack_desc *out) {
  LGS_REQUIRE(km && out && (op == 0 || op == 1), "lgs_conv_pack_desc: bad argument");
  LGS_REQUIRE(known_dtype(dtype), "lgs_conv_pack_desc: unknown dtype");
  const int g = op == 0 ? cin : cout, o = op == 0 ? cout : cin;
  const ConvPlan pl = plan_of(op_view(km, op, transposed), km->K, g, o, dtype, op == 0 ? kEpiBnStats : kEpiAccum);
  memset(out, 0, sizeof(*out));
  if (!pl.packed_ext_ok) return 0;      // empty maps, scratch / padded-input routes pack internally
  out->K = km->K; out->cin_w = cin; out->cout_w = cout; out->transposed = op; out->mirror = op_view(km, op, transposed).mirror;
  out->g_real = g; out->o_real = o; out->ncp = pl.ncp; out->nbp = pl.nbp;
  out->dtype = (dtype == LGS_F32 && tune(T_FP32_SPLIT) != 0) ? kDtF32Split : dtype;
  out->total = pl.total;
  out->bytes = pl.total * 16;
  return 0;
}

int lgs_pack_weights_batch(const lgs_pack_desc *descs_device, int n, int64_t max_total, void *stream) {
  LGS_REQUIRE(descs_device && n > 0 && max_total > 0, "lgs_pack_weights_batch: bad argument");
  dim3 grid((unsigned)((max_total + 255) / 256), (unsigned)n);
  LGS_KLAUNCH(k_pack_weights_batch, grid, 256, 0, (hipStream_t)stream, descs_device);
  LGS_HIP(hipGetLastError());
  return 0;
}

int lgs_conv_forward(lgs_kmap *km, int transposed, const void *in, int cin, const float *weight, int cout,
                     const float *bias, void *out, int dtype, void *workspace, float *bn_partial, const float *bn_pivot,
                     void *packed, int pack_mode, int in_row_stride, void *stream) {
  LGS_REQUIRE(km && weight && workspace, "lgs_conv_forward: null argument");
  BnEpi bn;
  bn.partial = bn_partial; bn.pivot = bn_pivot;
  LGS_REQUIRE(!bn_partial || lgs_conv_bn_partial_rows(km, transposed, cout, dtype) > 0,
              "lgs_conv_forward: this launch shape produces no BatchNorm statistics (see lgs_conv_bn_partial_rows)");
  return conv_call(km, 0, transposed, in, cin, weight, cout, bias, out, dtype, workspace, bn_partial ? &bn : nullptr, packed, pack_mode,
                   in_row_stride, stream);
}

int lgs_conv_dgrad(lgs_kmap *km, int transposed, const void *grad_out, int cout, const float *weight, int cin,
                   void *grad_in, int dtype, void *workspace, void *packed, int pack_mode, void *stream) {
  LGS_REQUIRE(km && weight && workspace, "lgs_conv_dgrad: null argument");
  return conv_call(km, 1, transposed, grad_out, cin, weight, cout, nullptr, grad_in, dtype, workspace, nullptr, packed, pack_mode, 0, stream);
}

// 1 if lgs_conv_dgrad_accumulate adds inside the kernel epilogue for this launch shape (everything but the 2-D blocked wide
// kernel and input widths off the 4-channel grid)
int lgs_conv_dgrad_can_accumulate(const lgs_kmap *km, int transposed, int cin, int cout, int dtype) {
  if (!km || (transposed && !traits_of(km).transposed_ok) || !known_dtype(dtype)) return 0;
  return plan_of(op_view(km, 1, transposed), km->K, cout, cin, dtype, kEpiAccum).can_accumulate;
}

// grad_in += dgrad(grad_out): the sum autograd would form when the convolution's input also feeds a residual branch, taken
// in the epilogue (rounded exactly like "store dgrad, then add"), instead of a separate elementwise pass over [N, cin]
int lgs_conv_dgrad_accumulate(lgs_kmap *km, int transposed, const void *grad_out, int cout, const float *weight, int cin,
                              void *grad_in, int dtype, void *workspace, void *packed, int pack_mode, void *stream) {
  LGS_REQUIRE(km && weight && workspace && grad_in, "lgs_conv_dgrad_accumulate: null argument");
  LGS_REQUIRE(lgs_conv_dgrad_can_accumulate(km, transposed, cin, cout, dtype), "lgs_conv_dgrad_accumulate: this launch shape has no accumulating epilogue (ask lgs_conv_dgrad_can_accumulate first)");
  BnEpi acc; acc.accum = 1;
  return conv_call(km, 1, transposed, grad_out, cin, weight, cout, nullptr, grad_in, dtype, workspace, &acc, packed, pack_mode, 0, stream);
}

// the plan of op 0 / 1 on a synthetic map + what the public queries say for it: no HIP call, the map's tables are never read
int lgs_debug_conv_plan(const lgs_conv_plan_query *q, lgs_conv_plan_info *out) {
  LGS_REQUIRE(q && out && (q->op == 0 || q->op == 1) && known_dtype(q->dtype) && q->epilogue >= 0 && q->epilogue <= 2, "lgs_debug_conv_plan: bad argument");
  lgs_kmap km;
  LGS_REQUIRE(synthetic_kmap(q->fwd, q->bwd, q->ks, km) == nullptr, "lgs_debug_conv_plan: bad argument");
  *out = plan_of(op_view(&km, q->op, q->transposed), km.K, q->op == 0 ? q->cin : q->cout, q->op == 0 ? q->cout : q->cin, q->dtype, (ConvEpi)q->epilogue);
  out->workspace_bytes = lgs_conv_workspace_bytes(&km, q->cin, q->cout, q->dtype, q->op);
  out->q_bn_partial_rows = q->op == 0 ? lgs_conv_bn_partial_rows(&km, q->transposed, q->cout, q->dtype) : 0;
  out->q_can_accumulate = q->op == 1 ? lgs_conv_dgrad_can_accumulate(&km, q->transposed, q->cin, q->cout, q->dtype) : 0;
  return lgs_conv_pack_desc(&km, q->op, q->transposed, q->cin, q->cout, q->dtype, &out->pack_desc);
}

// the instance the k_conv_gather launch of that plan runs, as conv_gather_op hands the launch its rows: no HIP call either
int lgs_debug_conv_gather_instance(const lgs_conv_plan_query *q, int with_statistics, lgs_conv_gather_instance *out) {
  lgs_conv_plan_info info;
  if (int rc = lgs_debug_conv_plan(q, &info)) return rc;
  LGS_REQUIRE(out && info.path == kPathGather, "lgs_debug_conv_gather_instance: not a k_conv_gather launch");
  LGS_REQUIRE(!with_statistics || info.q_bn_partial_rows > 0, "lgs_debug_conv_gather_instance: this launch shape produces no BatchNorm statistics");
  const int g_real = q->op == 0 ? q->cin : q->cout;
  return with_instance(q->dtype, [&](auto i) {
    constexpr int EPL = Tr<typename decltype(i)::S>::EPL;     // (a padded input is gathered in rows of whole 16-byte pieces)
    return describe_gather<typename decltype(i)::M>(info, info.pad_input ? (g_real + EPL - 1) / EPL * EPL : g_real, with_statistics != 0, out);
  });
}

// the GPU's own count of resident workgroups per CU of a bf16 instance: scl chunks per walked slab (the tile's own slab length or
// 0: its own instance), with the statistics epilogue or without (a tile that has one instance answers for that one)
int lgs_debug_conv_gather_residency(int tile_id, int scl, int bn_stats, int *workgroups_per_cu) {
  LGS_REQUIRE(workgroups_per_cu, "lgs_debug_conv_gather_residency: null argument");
  const GatherCfg t = tile_of(tile_id, false);
  const GatherInstance g = {tile_id, scl == t.sc ? 0 : scl, false, bn_stats != 0 || !t.lean, false};
  return with_gather_kernel<bf16_t>(g, [&](auto k, const char *) {
    LGS_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(workgroups_per_cu, reinterpret_cast<const void *>(k.fn), k.threads, 0));
    return 0;
  });
}

int64_t lgs_clip_workspace_bytes(int c, int n_anchor, int dtype) {
  return align256((int64_t)n_anchor * c * 4) + clip_image_room(c, n_anchor, dtype) + 256;
}

int64_t lgs_clip_loss_workspace_bytes(int c, int n_anchor, int dtype) {
  (void)n_anchor;
  return clip_loss_image_room(c, dtype) + 256;
}

int lgs_clip_loss_forward(const void *feat, int64_t n, int c, const float *anchors, int n_anchor, const int64_t *labels,
                          const int64_t *neg, int k_neg, int64_t ignore_label, float *d_pos, float *d_neg, int64_t *pred,
                          float *inv_norm_f, float *anchors_n, float *sim, int dtype, void *workspace, void *stream) {
  LGS_REQUIRE(feat && anchors && labels && neg && d_pos && d_neg && anchors_n && workspace, "lgs_clip_loss_forward: null argument");
  ClipEpi ce;
  ce.labels = labels; ce.neg = neg; ce.k_neg = k_neg; ce.ignore = ignore_label;
  ce.d_pos = d_pos; ce.d_neg = d_neg; ce.pred = pred; ce.inv_norm = inv_norm_f;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LGS_F32) return clip_loss_forward_t<float>(feat, n, c, anchors, n_anchor, ce, anchors_n, sim, workspace, s);
  if (dtype == LGS_BF16) return clip_loss_forward_t<bf16_t>(feat, n, c, anchors, n_anchor, ce, anchors_n, sim, workspace, s);
  LGS_REQUIRE(false, "lgs_clip_loss_forward: unknown dtype");
}

int lgs_clip_similarity(const void *feat, int64_t n, int c, const float *anchors, int n_anchor, float *sim,
                        float *inv_norm_f, int dtype, void *workspace, void *stream) {
  LGS_REQUIRE(feat && anchors && sim && workspace && inv_norm_f, "lgs_clip_similarity: null argument");
  hipStream_t s = (hipStream_t)stream;
  if (dtype == LGS_F32) return clip_similarity_t<float>(feat, n, c, anchors, n_anchor, sim, inv_norm_f, workspace, s);
  if (dtype == LGS_BF16) return clip_similarity_t<bf16_t>(feat, n, c, anchors, n_anchor, sim, inv_norm_f, workspace, s);
  LGS_REQUIRE(false, "lgs_clip_similarity: unknown dtype");
}

}  // extern "C"
