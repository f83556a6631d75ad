// lgs_rows.h -- the row-streaming operators' one access layer (lgs_pool.hip, lgs_instnorm.hip, lgs_norm.hip; the
// class-score kernels and k_clip_loss_bwd of lgs_loss.hip, k_seg_metrics of lgs_metrics.hip; gfx950).
//
// Features are [rows, C] row-major, fp32 or bf16.  A lane moves V = Width<T, VEC>::V adjacent channels per access: 16 bytes
// (4 fp32 / 8 bf16) where the channel count, the row strides and the pointers allow it, one element otherwise; values are
// widened to fp32 on load and rounded once (nearest even) on store.  Device side: ldv / stv / stv_nt / ldf.  Host side: the
// alignment rule (al16, stride_ok, rows_ok), lanes per row and grids (lanes_log2, grid_for), and the two lifts from run-time
// values to template arguments (with_row_type, with_op).  lgs_classrows.h builds the class-score kernels' own lift on with_op.
// The MFMA kernels keep their own packing code.
#pragma once
#include "lgs_common.h"

#include <initializer_list>
#include <type_traits>

namespace lgs {

#if defined(__HIPCC__)
template <typename T, bool VEC = true> struct Width { static constexpr int V = VEC ? (int)(16 / sizeof(T)) : 1; };

// V adjacent channels of a row -> fp32.  V == 16 bytes' worth: one 16-byte access, p 16-byte aligned; V == 1: one element
template <int V> __device__ inline void ldv(const float *p, float *v) {
  if constexpr (V == 4) {
    const float4 a = *reinterpret_cast<const float4 *>(p);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  } else {
    v[0] = *p;
  }
}
template <int V> __device__ inline void ldv(const bf16_t *p, float *v) {
  if constexpr (V == 8) {
    const uint4 a = *reinterpret_cast<const uint4 *>(p);
    const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[2 * i] = bf16_to_f32((uint16_t)(w[i] & 0xffffu));
      v[2 * i + 1] = bf16_to_f32((uint16_t)(w[i] >> 16));
    }
  } else {
    v[0] = bf16_to_f32(*p);
  }
}
template <int V> __device__ inline void stv(float *p, const float *v) {
  if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}
template <int V> __device__ inline void stv(bf16_t *p, const float *v) {
  if constexpr (V == 8) {
    uint4 x;
    x.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
    x.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
    x.z = (uint32_t)f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
    x.w = (uint32_t)f32_to_bf16(v[6]) | ((uint32_t)f32_to_bf16(v[7]) << 16);
    *reinterpret_cast<uint4 *>(p) = x;
  } else {
    *p = f32_to_bf16(v[0]);
  }
}
// the 16-byte store as a non-temporal one (BatchNorm's three-launch apply: the output is not read again soon)
template <int V> __device__ inline void stv_nt(float *p, const float *v) {
  static_assert(V == 4, "16-byte accesses only");
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 x = {v[0], v[1], v[2], v[3]};
  __builtin_nontemporal_store(x, reinterpret_cast<f4 *>(p));
}
template <int V> __device__ inline void stv_nt(bf16_t *p, const float *v) {
  static_assert(V == 8, "16-byte accesses only");
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  u4 x;
  x.x = (uint32_t)f32_to_bf16(v[0]) | ((uint32_t)f32_to_bf16(v[1]) << 16);
  x.y = (uint32_t)f32_to_bf16(v[2]) | ((uint32_t)f32_to_bf16(v[3]) << 16);
  x.z = (uint32_t)f32_to_bf16(v[4]) | ((uint32_t)f32_to_bf16(v[5]) << 16);
  x.w = (uint32_t)f32_to_bf16(v[6]) | ((uint32_t)f32_to_bf16(v[7]) << 16);
  __builtin_nontemporal_store(x, reinterpret_cast<u4 *>(p));
}
// V consecutive floats of an fp32 row (statistics, weight, bias): V is 1, 4 or 8 and the rows are 16-byte aligned when V > 1
template <int V> __device__ inline void ldf(const float *p, float *v) {
  if constexpr (V == 1) {
    v[0] = *p;
  } else {
#pragma unroll
    for (int i = 0; i < V; i += 4) ldv<4>(p + i, v + i);
  }
}

// the element type and the access width of a call as compile-time values; its void pointers as T
template <typename E, bool VEC> struct RowType {
  using T = E;
  static constexpr bool vec = VEC;
  static const T *in(const void *p) { return reinterpret_cast<const T *>(p); }
  static T *out(void *p) { return reinterpret_cast<T *>(p); }
};
// (dtype, vec) -> f(RowType<T, VEC>()); `who` names the entry point in the refusal of an unknown dtype
template <typename F> int with_row_type(int dtype, bool vec, const char *who, F &&f) {
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, std::string(who) + ": unknown dtype");
  if (dtype == LGS_BF16) return vec ? f(RowType<bf16_t, true>()) : f(RowType<bf16_t, false>());
  return vec ? f(RowType<float, true>()) : f(RowType<float, false>());
}
#endif

// op in [0, N) -> f(std::integral_constant<int, op>()) (the callers have checked the range)
template <int N, typename F> int with_op(int op, F &&f) {
  if constexpr (N == 1) return f(std::integral_constant<int, 0>());
  else return op == N - 1 ? f(std::integral_constant<int, N - 1>()) : with_op<N - 1>(op, f);
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }
// a [rows, c] operand with row stride ld (elements), e.g. a column slice of a wider row-major buffer: every row starts 16-byte
// aligned and holds whole 16-byte groups -- what a 16-byte access per lane needs
inline bool stride_ok(const void *p, int64_t ld, int c, int dtype) { return ld >= c && ld % epl(dtype) == 0 && al16(p); }
// the same for every operand a call dereferences (contiguous operands: ld = c, so c itself must be a multiple of the width)
struct RowOperand { const void *p; int64_t ld; };
inline bool rows_ok(std::initializer_list<RowOperand> ops, int c, int dtype) {
  for (const RowOperand &o : ops)
    if (!stride_ok(o.p, o.ld, c, dtype)) return false;
  return true;
}
// lanes per row: enough 16-byte (or 1-element) accesses to cover the row once, at most a wave
inline int lanes_log2(int c, int v) {
  const int chunks = (c + v - 1) / v;
  int lg = 0;
  while ((1 << lg) < chunks && lg < 6) ++lg;
  return lg;
}
// workgroups of 256 threads for `units` rows of 2^lg lanes each, every lane group taking `per_group` rows; at least one
inline int64_t grid_for(int64_t units, int lg, int per_group = 1) {
  const int64_t threads = units << lg, per_block = 256 * (int64_t)per_group;
  return (threads + per_block - 1) / per_block > 0 ? (threads + per_block - 1) / per_block : 1;
}

}  // namespace lgs
