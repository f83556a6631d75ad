// lgs_classrows.h -- what the kernels that stream [N, C] class scores share: k_ce_fwd_bwd, k_focal_fwd_bwd (lgs_loss.hip) and
// k_seg_metrics (lgs_metrics.hip); gfx950.
//
// The access shape of all three: half a wavefront per row.  A lane holds Q 16-byte chunks (W = 4 fp32 / 8 bf16 elements) of each of R
// consecutive rows in `float v[R][Q][W]`, Q x R = 4, and a half-wave issues the loads of ALL its rows before it touches the first
// (with one 400-byte row in flight per half-wave the 1.2 M x 200 launch ran at 2.8 TB/s: 32 waves per CU x 800 bytes is not enough
// outstanding traffic; Q x R = 4 keeps the register count where one row left it).  Rows that are no multiple of 16 bytes (13
// classes; 20 in bf16) take element-wise accesses behind a kernel-uniform flag `vec`; their padding elements hold a value whose
// exponential is 0.  Per row: the maximum, the exponentials (in place) and their per-lane sum in the order q, then i, the xor
// butterfly 16, 8, 4, 2, 1 inside the half-wave, and a store loop.  The accesses are lgs_rows.h's ldv / stv.
// Shared as code: the host side -- class_shape (the class counts a half-wave holds and their refusal) and with_class_rows, the lift
// from (dtype, q, op) to (T, Q, R, OP).  The device loops are written out in each kernel: moving any of them behind a function,
// even the butterfly alone, reorders the instruction streams of most instantiations (same registers, other schedule), and a bf16
// head of 513 - 1024 classes lost a wave per SIMD with the whole tile behind one struct.  A change to the shape is made in the three
// kernels; tests/test_gpu_class_rows_bits.py holds all of them to recorded bits.
#pragma once
#include "lgs_rows.h"

namespace lgs {

constexpr int kClassChunks = 4;  // 16-byte chunks per lane per row: C <= 32 * 4 * W

#if defined(__HIPCC__)
// element type, chunks per lane and rows per half-wave of a call as compile-time values; its void pointers as T
template <typename E, int Q_, int R_> struct ClassRows {
  using T = E;
  static constexpr int Q = Q_, R = R_;
  static const T *in(const void *p) { return reinterpret_cast<const T *>(p); }
  static T *out(void *p) { return reinterpret_cast<T *>(p); }
  // workgroups of 8 half-waves for n rows
  static int64_t tiles(int64_t n) { return (n + 8 * R - 1) / (8 * R); }
};
// (dtype, q, op in [0, NOPS)) -> f(ClassRows<T, Q, R>(), std::integral_constant<int, op>()), Q x R = 4: one lambda level, so that a
// launch site inside f is named by all four; `who` names the entry point in the refusal of an unknown dtype
template <int NOPS, typename F> int with_class_rows(int dtype, int q, int op, const char *who, F &&f) {
  LGS_REQUIRE(dtype == LGS_F32 || dtype == LGS_BF16, std::string(who) + ": unknown dtype");
  return with_op<NOPS>(op, [&](auto o) {
    if (dtype == LGS_BF16) return q <= 1 ? f(ClassRows<bf16_t, 1, 4>(), o) : q == 2 ? f(ClassRows<bf16_t, 2, 2>(), o) : f(ClassRows<bf16_t, 4, 1>(), o);
    return q <= 1 ? f(ClassRows<float, 1, 4>(), o) : q == 2 ? f(ClassRows<float, 2, 2>(), o) : f(ClassRows<float, 4, 1>(), o);
  });
}
#endif

// c classes of `dtype` -> q = 16-byte chunks per lane and row; refuses what half a wavefront cannot hold
inline int class_shape(int c, int dtype, const char *who, int *q) {
  const int nchunk = (c + epl(dtype) - 1) / epl(dtype);
  LGS_REQUIRE(c >= 1 && nchunk <= 32 * kClassChunks, std::string(who) + ": more classes than one half-wave holds (512 fp32 / 1024 bf16)");
  *q = (nchunk + 31) / 32;
  return 0;
}

}  // namespace lgs
