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
// the row strides allow it, one element otherwise (C % 8 != 0, e.g. C = 3).
#include "lgs_common.h"

#include <climits>

namespace lgs {
namespace {

enum { R_SUM = 0, R_AVG = 1, R_MAX = 2, R_PROD = 3 };
enum { B_COPY = 0, B_SCALE = 1, B_ADD = 2, B_MUL = 3, B_COPYX = 4 };

template <typename T, bool VEC> struct Width { static constexpr int V = VEC ? (int)(16 / sizeof(T)) : 1; };

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
      v[2 * i] = __uint_as_float(w[i] << 16);
      v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
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
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = (uint32_t)f32_to_bf16(v[2 * i]) | ((uint32_t)f32_to_bf16(v[2 * i + 1]) << 16);
    *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    *p = f32_to_bf16(v[0]);
  }
}
__device__ inline void st1(float *p, float v) { *p = v; }
__device__ inline void st1(bf16_t *p, float v) { *p = f32_to_bf16(v); }

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
    st1(out + q * c + col, acc);
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

// lanes per row: enough 16-byte (or 1-element) accesses to cover the row once, at most a wave
inline int lanes_log2(int c, int v) {
  const int chunks = (c + v - 1) / v;
  int lg = 0;
  while ((1 << lg) < chunks && lg < 6) ++lg;
  return lg;
}
inline unsigned grid_for(int64_t units, int lg) {
  const int64_t threads = units << lg;
  return (unsigned)((threads + 255) / 256 > 0 ? (threads + 255) / 256 : 1);
}
inline bool al16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

template <typename T, bool VEC>
int reduce_t(const SegMap &sm, int op, const void *xv, const void *x2v, int64_t x_ld, int c, void *outv, int32_t *amax, void *ws,
             hipStream_t s) {
  const T *x = (const T *)xv, *x2 = (const T *)x2v;
  T *out = (T *)outv;
  const int lg = lanes_log2(c, Width<T, VEC>::V);
  if (sm.single_pass()) {
    const unsigned g = grid_for(sm.n_coarse, lg);
    const int64_t u = sm.n_coarse;
    if (op == R_SUM) LGS_KLAUNCH((k_seg_reduce<T, VEC, R_SUM, false>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, nullptr, nullptr);
    else if (op == R_AVG) LGS_KLAUNCH((k_seg_reduce<T, VEC, R_AVG, false>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, nullptr, nullptr);
    else if (op == R_MAX) LGS_KLAUNCH((k_seg_reduce<T, VEC, R_MAX, false>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, nullptr, nullptr);
    else LGS_KLAUNCH((k_seg_reduce<T, VEC, R_PROD, false>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, nullptr, nullptr);
    LGS_HIP(hipGetLastError());
    return 0;
  }
  float *part = (float *)ws;
  int32_t *pam = (int32_t *)((char *)ws + align256(sm.n_items * (int64_t)c * 4));
  const unsigned g = grid_for(sm.n_items, lg);
  const int64_t u = sm.n_items;
  const int lgc = lanes_log2(c, 1);
  const unsigned gc = grid_for(sm.n_coarse, lgc);
  if (op == R_SUM) {
    LGS_KLAUNCH((k_seg_reduce<T, VEC, R_SUM, true>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, part, pam);
    LGS_KLAUNCH((k_seg_combine<T, R_SUM>), gc, 256, 0, s, sm, part, pam, c, lgc, out, amax);
  } else if (op == R_AVG) {
    LGS_KLAUNCH((k_seg_reduce<T, VEC, R_AVG, true>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, part, pam);
    LGS_KLAUNCH((k_seg_combine<T, R_AVG>), gc, 256, 0, s, sm, part, pam, c, lgc, out, amax);
  } else if (op == R_MAX) {
    LGS_KLAUNCH((k_seg_reduce<T, VEC, R_MAX, true>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, part, pam);
    LGS_KLAUNCH((k_seg_combine<T, R_MAX>), gc, 256, 0, s, sm, part, pam, c, lgc, out, amax);
  } else {
    LGS_KLAUNCH((k_seg_reduce<T, VEC, R_PROD, true>), g, 256, 0, s, sm, x, x2, x_ld, c, lg, u, out, amax, part, pam);
    LGS_KLAUNCH((k_seg_combine<T, R_SUM>), gc, 256, 0, s, sm, part, pam, c, lgc, out, amax);
  }
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool VEC>
int bcast_t(const SegMap &sm, int op, const void *gv, int c, const void *xv, int64_t x_ld, void *outv, int64_t out_ld, hipStream_t s) {
  const T *g = (const T *)gv, *x = (const T *)xv;
  T *out = (T *)outv;
  const int lg = lanes_log2(c, Width<T, VEC>::V);
  const unsigned gr = grid_for(sm.n_fine, lg);
  if (op == B_COPY) LGS_KLAUNCH((k_seg_bcast<T, VEC, B_COPY>), gr, 256, 0, s, sm, g, x, x_ld, c, lg, out, out_ld);
  else if (op == B_SCALE) LGS_KLAUNCH((k_seg_bcast<T, VEC, B_SCALE>), gr, 256, 0, s, sm, g, x, x_ld, c, lg, out, out_ld);
  else if (op == B_ADD) LGS_KLAUNCH((k_seg_bcast<T, VEC, B_ADD>), gr, 256, 0, s, sm, g, x, x_ld, c, lg, out, out_ld);
  else if (op == B_MUL) LGS_KLAUNCH((k_seg_bcast<T, VEC, B_MUL>), gr, 256, 0, s, sm, g, x, x_ld, c, lg, out, out_ld);
  else LGS_KLAUNCH((k_seg_bcast<T, VEC, B_COPYX>), gr, 256, 0, s, sm, g, x, x_ld, c, lg, out, out_ld);
  LGS_HIP(hipGetLastError());
  return 0;
}

template <typename T, bool VEC>
int max_bwd_t(const SegMap &sm, const void *dy, const int32_t *amax, int c, void *dx, hipStream_t s) {
  const int lg = lanes_log2(c, Width<T, VEC>::V);
  LGS_KLAUNCH((k_seg_max_bwd<T, VEC>), grid_for(sm.n_fine, lg), 256, 0, s, sm, (const T *)dy, amax, c, lg, (T *)dx);
  LGS_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace lgs

using namespace lgs;

extern "C" {

int64_t lgs_seg_workspace_bytes(const lgs_segmap *h, int c) {
  if (!h || c <= 0 || h->sm.single_pass()) return 0;
  return 2 * align256(h->sm.n_items * (int64_t)c * 4);
}

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
  const int es = esize(dtype), v = 16 / es;
  const bool vec = c % v == 0 && (x_ld * es) % 16 == 0 && al16(x) && al16(out) && (op != R_PROD || al16(x2));
  if (dtype == LGS_BF16)
    return vec ? reduce_t<bf16_t, true>(sm, op, x, x2, x_ld, c, out, argmax, workspace, s)
               : reduce_t<bf16_t, false>(sm, op, x, x2, x_ld, c, out, argmax, workspace, s);
  return vec ? reduce_t<float, true>(sm, op, x, x2, x_ld, c, out, argmax, workspace, s)
             : reduce_t<float, false>(sm, op, x, x2, x_ld, c, out, argmax, workspace, s);
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
  const int es = esize(dtype), v = 16 / es;
  const bool vec = c % v == 0 && (out_ld * es) % 16 == 0 && al16(out) && (op == B_COPYX || al16(g)) &&
                   (!needs_x || ((x_ld * es) % 16 == 0 && al16(x)));
  if (dtype == LGS_BF16)
    return vec ? bcast_t<bf16_t, true>(sm, op, g, c, x, x_ld, out, out_ld, s) : bcast_t<bf16_t, false>(sm, op, g, c, x, x_ld, out, out_ld, s);
  return vec ? bcast_t<float, true>(sm, op, g, c, x, x_ld, out, out_ld, s) : bcast_t<float, false>(sm, op, g, c, x, x_ld, out, out_ld, s);
}

int lgs_seg_max_backward(lgs_segmap *h, const void *dy, const int32_t *argmax, int c, void *dx, int dtype, void *stream) {
  LGS_REQUIRE(h && c > 0 && (dtype == LGS_F32 || dtype == LGS_BF16), "lgs_seg_max_backward: bad argument");
  const SegMap &sm = h->sm;
  if (sm.n_fine == 0) return 0;
  LGS_REQUIRE(dy && argmax && dx, "lgs_seg_max_backward: null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (segmap_wait(h, s)) return 1;
  const int es = esize(dtype), v = 16 / es;
  const bool vec = c % v == 0 && al16(dy) && al16(dx);
  if (dtype == LGS_BF16) return vec ? max_bwd_t<bf16_t, true>(sm, dy, argmax, c, dx, s) : max_bwd_t<bf16_t, false>(sm, dy, argmax, c, dx, s);
  return vec ? max_bwd_t<float, true>(sm, dy, argmax, c, dx, s) : max_bwd_t<float, false>(sm, dy, argmax, c, dx, s);
}

int lgs_segmap_size(const lgs_segmap *h, int64_t *n_fine, int64_t *n_coarse) {
  LGS_REQUIRE(h, "lgs_segmap_size: null handle");
  if (n_fine) *n_fine = h->sm.n_fine;
  if (n_coarse) *n_coarse = h->sm.n_coarse;
  return 0;
}

}  // extern "C"
