// lgs_pool.hip -- sparse pooling, global pooling and broadcast as segmented reductions / broadcasts (gfx950).
//
// Replaces MinkowskiEngine's pooling and broadcast operators (kernel_size == stride == 2^k, global pooling, broadcast of a
// global-pooled tensor) as the reference calls them:
//   sum_pool / avg_pool / avg_unpool helpers        /root/reference/models/modules/common.py:239-300, models/resnet.py:48
//   MinkowskiPoolingTranspose(8 / 4 / 2)            /root/reference/models/resunet.py:367,388,409
//   global pooling + broadcast norms                /root/reference/downstream/insseg/lib/layers.py
//
// Every operator is a pass over a SegMap (lgs_common.h, built by lgs_manager_segment_map): the fine rows of coarse row q are
// the fine sorted positions [seg_start[q], seg_start[q+1]).  Three kernel families, each templated on the storage type:
//   k_seg_reduce   coarse-stationary: sum / avg / max (+ arg-max rows) / sum of a product, fp32 accumulation in the order of
//                  the sorted positions, each output row written once (no atomics: the result is the same on every run);
//                  segments that can be longer than kSegChunk rows go through chunk items and k_seg_combine
//   k_seg_bcast    fine-stationary: copy / divide by the segment's row count / add / multiply, or a plain row copy (concat)
//   k_seg_max_bwd  fine-stationary: dx[row][c] = (argmax[q][c] == row) ? dy[q][c] : 0
// A group of 2^lg lanes owns one row; every lane moves 16 bytes per access (8 bf16 / 4 fp32) when the channel count and
// the row strides allow it, one element otherwise (C % 8 != 0, e.g. C = 3): the accesses, that rule and the lift from
// (dtype, width, op) to template arguments are lgs_rows.h's.  Everything a call decides on the host comes from seg_plan().
#include "lgs_rows.h"

#include <climits>

namespace lgs {
namespace {

enum { R_SUM = 0, R_AVG = 1, R_MAX = 2, R_PROD = 3 };
enum { B_COPY = 0, B_SCALE = 1, B_ADD = 2, B_MUL = 3, B_COPYX = 4 };

template <int OP, int V> __device__ inline void acc_init(float *acc, int32_t *arg) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    acc[i] = OP == R_MAX ? -INFINITY : 0.f;
    arg[i] = INT_MAX;
  }
}
// max: strictly larger wins; on equal values the smaller fine row (the documented tie rule of the gradient)
template <int OP, int V> __device__ inline void acc_add(float *acc, int32_t *arg, const float *v, const float *w, int32_t row) {
#pragma unroll
  for (int i = 0; i < V; ++i) {
    if constexpr (OP == R_MAX) {
      if (v[i] > acc[i] || (v[i] == acc[i] && row < arg[i])) { acc[i] = v[i]; arg[i] = row; }
    } else if constexpr (OP == R_PROD) {
      acc[i] += v[i] * w[i];
    } else {
      acc[i] += v[i];
    }
  }
}

// one unit = one coarse row (PART = false) or one chunk item of at most kSegChunk rows (PART = true: fp32 partials)
template <typename T, bool VEC, int OP, bool PART>
__global__ __launch_bounds__(256) void k_seg_reduce(SegMap sm, const T *__restrict__ x, const T *__restrict__ x2, int64_t x_ld, int c,
                                                    int lg, int64_t units, T *__restrict__ out, int32_t *__restrict__ amax,
                                                    float *__restrict__ part, int32_t *__restrict__ part_amax) {
  constexpr int V = Width<T, VEC>::V;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t u = t >> lg;
  const int lane = (int)(t & ((1 << lg) - 1));
  if (u >= units) return;
  int32_t q, s, e;
  if constexpr (PART) {
    q = sm.item_seg[u];
    if (q < 0) return;
    s = sm.seg_start[q] + ((int32_t)u - sm.item_start[q]) * kSegChunk;
    e = min(s + kSegChunk, sm.seg_start[q + 1]);
  } else {
    q = (int32_t)u;
    s = sm.seg_start[q];
    e = sm.seg_start[q + 1];
  }
  const int32_t *fr = sm.fine_row;
  for (int col = lane * V; col < c; col += V << lg) {
    float acc[V];
    int32_t arg[V];
    acc_init<OP, V>(acc, arg);
    int32_t p = s;
    for (; p + 4 <= e; p += 4) {   // four rows in flight, accumulated in position order
      int32_t r[4];
      float v[4][V], w[4][V];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = fr ? fr[p + j] : p + j;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ldv<V>(x + (int64_t)r[j] * x_ld + col, v[j]);
        if constexpr (OP == R_PROD) ldv<V>(x2 + (int64_t)r[j] * x_ld + col, w[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc_add<OP, V>(acc, arg, v[j], w[j], r[j]);
    }
    for (; p < e; ++p) {
      const int32_t r = fr ? fr[p] : p;
      float v[V], w[V];
      ldv<V>(x + (int64_t)r * x_ld + col, v);
      if constexpr (OP == R_PROD) ldv<V>(x2 + (int64_t)r * x_ld + col, w);
      acc_add<OP, V>(acc, arg, v, w, r);
    }
    if constexpr (PART) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        part[u * c + col + i] = acc[i];
        if constexpr (OP == R_MAX) part_amax[u * c + col + i] = arg[i];
      }
    } else {
      if constexpr (OP == R_AVG) {
        const float cnt = (float)(e - s);
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = acc[i] / cnt;
      }
      stv<V>(out + (int64_t)q * c + col, acc);
      if constexpr (OP == R_MAX) {
#pragma unroll
        for (int i = 0; i < V; ++i) amax[(int64_t)q * c + col + i] = arg[i];
      }
    }
  }
}

// second pass of a two-pass reduction: segment q folds its chunk items' partials in item order
template <typename T, int OP>
__global__ __launch_bounds__(256) void k_seg_combine(SegMap sm, const float *__restrict__ part, const int32_t *__restrict__ part_amax,
                                                     int c, int lg, T *__restrict__ out, int32_t *__restrict__ amax) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t q = t >> lg;
  const int lane = (int)(t & ((1 << lg) - 1));
  if (q >= sm.n_coarse) return;
  const int32_t i0 = sm.item_start[q], i1 = sm.item_start[q + 1];
  for (int col = lane; col < c; col += 1 << lg) {
    float acc = OP == R_MAX ? -INFINITY : 0.f;
    int32_t arg = INT_MAX;
    for (int32_t i = i0; i < i1; ++i) {
      const float v = part[(int64_t)i * c + col];
      if constexpr (OP == R_MAX) {
        const int32_t a = part_amax[(int64_t)i * c + col];
        if (v > acc || (v == acc && a < arg)) { acc = v; arg = a; }
      } else {
        acc += v;
      }
    }
    if constexpr (OP == R_AVG) acc = acc / (float)(sm.seg_start[q + 1] - sm.seg_start[q]);
    stv<1>(out + q * c + col, &acc);
    if constexpr (OP == R_MAX) amax[q * c + col] = arg;
  }
}

// one unit = one fine sorted position p: out[row(p)] = f(x[row(p)], g[coarse_of[p]])
template <typename T, bool VEC, int OP>
__global__ __launch_bounds__(256) void k_seg_bcast(SegMap sm, const T *__restrict__ g, const T *__restrict__ x, int64_t x_ld, int c,
                                                   int lg, T *__restrict__ out, int64_t out_ld) {
  constexpr int V = Width<T, VEC>::V;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = t >> lg;
  const int lane = (int)(t & ((1 << lg) - 1));
  if (p >= sm.n_fine) return;
  const int64_t row = sm.fine_row ? sm.fine_row[p] : p;
  const int64_t q = sm.coarse_of[p];
  float cnt = 1.f;
  if constexpr (OP == B_SCALE) cnt = (float)(sm.seg_start[q + 1] - sm.seg_start[q]);
  for (int col = lane * V; col < c; col += V << lg) {
    float gv[V], xv[V], o[V];
    if constexpr (OP != B_COPYX) ldv<V>(g + q * c + col, gv);
    if constexpr (OP == B_ADD || OP == B_MUL || OP == B_COPYX) ldv<V>(x + row * x_ld + col, xv);
#pragma unroll
    for (int i = 0; i < V; ++i) {
      if constexpr (OP == B_COPY) o[i] = gv[i];
      else if constexpr (OP == B_SCALE) o[i] = gv[i] / cnt;
      else if constexpr (OP == B_ADD) o[i] = xv[i] + gv[i];
      else if constexpr (OP == B_MUL) o[i] = xv[i] * gv[i];
      else o[i] = xv[i];
    }
    stv<V>(out + row * out_ld + col, o);
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void k_seg_max_bwd(SegMap sm, const T *__restrict__ dy, const int32_t *__restrict__ amax, int c, int lg,
                                                     T *__restrict__ dx) {
  constexpr int V = Width<T, VEC>::V;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = t >> lg;
  const int lane = (int)(t & ((1 << lg) - 1));
  if (p >= sm.n_fine) return;
  const int32_t row = sm.fine_row ? sm.fine_row[p] : (int32_t)p;
  const int64_t q = sm.coarse_of[p];
  for (int col = lane * V; col < c; col += V << lg) {
    float d[V], o[V];
    ldv<V>(dy + q * c + col, d);
#pragma unroll
    for (int i = 0; i < V; ++i) o[i] = amax[q * c + col + i] == row ? d[i] : 0.f;
    stv<V>(dx + (int64_t)row * c + col, o);
  }
}


}  // namespace

// Everything a pooling / broadcast call decides on the host, from plain integers (no HIP call): the access width, the lanes per
// row, the grids of the family's launches and the two-pass reduction's workspace regions.  `vec_ok`: every operand the call
// dereferences passes stride_ok (rows_ok over the entry point's list).  lgs_debug_seg_plan returns it without a GPU.
using SegPlan = lgs_seg_plan_info;
enum SegFamily { kSegReduce = 0, kSegBcast = 1, kSegMaxBwd = 2 };
SegPlan seg_plan(int family, int64_t n_fine, int64_t n_coarse, int64_t n_items, bool single_pass, int c, int dtype, bool vec_ok) {
  SegPlan p = {};
  const int es = esize(dtype);
  p.vec = vec_ok && (c * es) % 16 == 0 ? 1 : 0;
  p.lanes_log2 = lanes_log2(c, p.vec ? 16 / es : 1);
  p.combine_lanes_log2 = lanes_log2(c, 1);
  if (family == kSegReduce) {
    p.reduce_grid = grid_for(single_pass ? n_coarse : n_items, p.lanes_log2);
    if (!single_pass) {   // chunk items -> fp32 partials (+ their arg-max rows), folded per segment by k_seg_combine
      p.combine_grid = grid_for(n_coarse, p.combine_lanes_log2);
      int64_t used = 0;
      p.partials = take_region(used, n_items * (int64_t)c * 4);
      p.partial_argmax = take_region(used, n_items * (int64_t)c * 4);
      p.bytes_total = used;
    }
  } else if (family == kSegBcast) {
    p.bcast_grid = grid_for(n_fine, p.lanes_log2);
  } else {
    p.max_bwd_grid = grid_for(n_fine, p.lanes_log2);
  }
  p.workspace_bytes = single_pass ? 0 : 2 * align256(n_items * (int64_t)c * 4);   // of the map and c alone: every op, both dtypes
  return p;
}

namespace {

template <typename T, bool VEC, int OP>
int reduce_t(const SegMap &sm, const SegPlan &p, const T *x, const T *x2, int64_t x_ld, int c, T *out, int32_t *amax, void *ws, hipStream_t s) {
  const unsigned g = (unsigned)p.reduce_grid;
  if (sm.single_pass()) {
    LGS_KLAUNCH((k_seg_reduce<T, VEC, OP, false>), g, 256, 0, s, sm, x, x2, x_ld, c, p.lanes_log2, sm.n_coarse, out, amax, nullptr, nullptr);
  } else {
    constexpr int COMBINE = OP == R_PROD ? R_SUM : OP;   // the partials of a sum of products are sums
    float *part = (float *)((char *)ws + p.partials.offset);
    int32_t *pam = (int32_t *)((char *)ws + p.partial_argmax.offset);
    LGS_KLAUNCH((k_seg_reduce<T, VEC, OP, true>), g, 256, 0, s, sm, x, x2, x_ld, c, p.lanes_log2, sm.n_items, out, amax, part, pam);
    LGS_KLAUNCH((k_seg_combine<T, COMBINE>), (unsigned)p.combine_grid, 256, 0, s, sm, part, pam, c, p.combine_lanes_log2, out, amax);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool VEC, int OP>
int bcast_t(const SegMap &sm, const SegPlan &p, const T *g, int c, const T *x, int64_t x_ld, T *out, int64_t out_ld, hipStream_t s) {
  LGS_KLAUNCH((k_seg_bcast<T, VEC, OP>), (unsigned)p.bcast_grid, 256, 0, s, sm, g, x, x_ld, c, p.lanes_log2, out, out_ld);
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool VEC>
int max_bwd_t(const SegMap &sm, const SegPlan &p, const T *dy, const int32_t *amax, int c, T *dx, hipStream_t s) {
  LGS_KLAUNCH((k_seg_max_bwd<T, VEC>), (unsigned)p.max_bwd_grid, 256, 0, s, sm, dy, amax, c, p.lanes_log2, dx);
  LGS_HIP(hipGetLastError());
  return 0;
}

SegPlan plan_of(int family, const SegMap &sm, int c, int dtype, bool vec_ok) {
  return seg_plan(family, sm.n_fine, sm.n_coarse, sm.n_items, sm.single_pass(), c, dtype, vec_ok);
}

}  // namespace
}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_seg_workspace_bytes(const lgs_segmap *h, int c) {
  if (!h || c <= 0) return 0;
  return plan_of(kSegReduce, h->sm, c, LGS_F32, true).workspace_bytes;
}

// Each entry point lists the operands it dereferences (pointer, row stride in elements); rows_ok over that list is the one
// rule for 16-byte accesses.  Contiguous operands carry the stride c.
int lgs_seg_reduce(lgs_segmap *h, int op, const void *x, const void *x2, int64_t x_ld, int c, void *out, int32_t *argmax,
                   int dtype, void *workspace, void *stream) {
  LGS_REQUIRE(h && c > 0 && (dtype == LGS_F32 || dtype == LGS_BF16), "lgs_seg_reduce: bad argument");
  LGS_REQUIRE(op >= R_SUM && op <= R_PROD, "lgs_seg_reduce: op must be 0 (sum), 1 (avg), 2 (max) or 3 (sum of products)");
  LGS_REQUIRE(x_ld >= c, "lgs_seg_reduce: row stride below the channel count");
  const SegMap &sm = h->sm;
  if (sm.n_coarse == 0) return 0;
  LGS_REQUIRE(x && out, "lgs_seg_reduce: null feature pointer");
  LGS_REQUIRE(op != R_MAX || argmax, "lgs_seg_reduce: max needs the argmax output");
  LGS_REQUIRE(op != R_PROD || x2, "lgs_seg_reduce: the product form needs x2");
  LGS_REQUIRE(sm.single_pass() || workspace, "lgs_seg_reduce: this map needs lgs_seg_workspace_bytes of workspace");
  hipStream_t s = (hipStream_t)stream;
  if (segmap_wait(h, s)) return 1;
  const bool vec_ok = op == R_PROD ? rows_ok({{x, x_ld}, {out, c}, {x2, x_ld}}, c, dtype) : rows_ok({{x, x_ld}, {out, c}}, c, dtype);
  const SegPlan p = plan_of(kSegReduce, sm, c, dtype, vec_ok);
  return with_row_type(dtype, p.vec, "lgs_seg_reduce", [&](auto e) {
    using E = decltype(e);
    return with_op<R_PROD + 1>(op, [&](auto o) {
      return reduce_t<typename E::T, E::vec, decltype(o)::value>(sm, p, e.in(x), e.in(x2), x_ld, c, e.out(out), argmax, workspace, s);
    });
  });
}

int lgs_seg_broadcast(lgs_segmap *h, int op, const void *g, int c, const void *x, int64_t x_ld, void *out, int64_t out_ld, int dtype,
                      void *stream) {
  LGS_REQUIRE(h && c > 0 && (dtype == LGS_F32 || dtype == LGS_BF16), "lgs_seg_broadcast: bad argument");
  LGS_REQUIRE(op >= B_COPY && op <= B_COPYX, "lgs_seg_broadcast: op must be 0 (copy), 1 (scale by 1/count), 2 (add), 3 (multiply) or 4 (copy x)");
  LGS_REQUIRE(out_ld >= c, "lgs_seg_broadcast: output row stride below the channel count");
  const bool needs_x = op == B_ADD || op == B_MUL || op == B_COPYX;
  LGS_REQUIRE(!needs_x || x_ld >= c, "lgs_seg_broadcast: row stride of x below the channel count");
  const SegMap &sm = h->sm;
  if (sm.n_fine == 0) return 0;
  LGS_REQUIRE(out && (op == B_COPYX || g) && (!needs_x || x), "lgs_seg_broadcast: null feature pointer");
  hipStream_t s = (hipStream_t)stream;
  if (segmap_wait(h, s)) return 1;
  const bool vec_ok = op == B_COPYX ? rows_ok({{out, out_ld}, {x, x_ld}}, c, dtype)
                      : needs_x     ? rows_ok({{out, out_ld}, {g, c}, {x, x_ld}}, c, dtype)
                                    : rows_ok({{out, out_ld}, {g, c}}, c, dtype);
  const SegPlan p = plan_of(kSegBcast, sm, c, dtype, vec_ok);
  return with_row_type(dtype, p.vec, "lgs_seg_broadcast", [&](auto e) {
    using E = decltype(e);
    return with_op<B_COPYX + 1>(op, [&](auto o) {
      return bcast_t<typename E::T, E::vec, decltype(o)::value>(sm, p, e.in(g), c, e.in(x), x_ld, e.out(out), out_ld, s);
    });
  });
}

int lgs_seg_max_backward(lgs_segmap *h, const void *dy, const int32_t *argmax, int c, void *dx, int dtype, void *stream) {
  LGS_REQUIRE(h && c > 0 && (dtype == LGS_F32 || dtype == LGS_BF16), "lgs_seg_max_backward: bad argument");
  const SegMap &sm = h->sm;
  if (sm.n_fine == 0) return 0;
  LGS_REQUIRE(dy && argmax && dx, "lgs_seg_max_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (segmap_wait(h, s)) return 1;
  const SegPlan p = plan_of(kSegMaxBwd, sm, c, dtype, rows_ok({{dy, c}, {dx, c}}, c, dtype));
  return with_row_type(dtype, p.vec, "lgs_seg_max_backward", [&](auto e) {
    using E = decltype(e);
    return max_bwd_t<typename E::T, E::vec>(sm, p, e.in(dy), argmax, c, e.out(dx), s);
  });
}

int lgs_segmap_size(const lgs_segmap *h, int64_t *n_fine, int64_t *n_coarse) {
  LGS_REQUIRE(h, "lgs_segmap_size: null handle");
  if (n_fine) *n_fine = h->sm.n_fine;
  if (n_coarse) *n_coarse = h->sm.n_coarse;
  return 0;
}

// the plan of a call given by plain integers: no HIP call (tests/test_seg_plan_cpu.py)
int lgs_debug_seg_plan(const lgs_seg_plan_query *q, lgs_seg_plan_info *out) {
  LGS_REQUIRE(q && out && q->c > 0 && (q->dtype == LGS_F32 || q->dtype == LGS_BF16) && q->family >= kSegReduce && q->family <= kSegMaxBwd &&
                  q->n_fine >= 0 && q->n_coarse >= 0 && q->n_items >= 0,
              "lgs_debug_seg_plan: bad argument");
  *out = seg_plan(q->family, q->n_fine, q->n_coarse, q->n_items, q->single_pass != 0, q->c, q->dtype, q->vec_ok != 0);
  return 0;
}

}  // extern "C"
