// The classifier head behind the token readout, and the GraphSAINT-weighted NLL loss with its metrics, fused.
// Reference: src/ampnet/module/amp_gcn.py:272-276 (final_linear_out -> log_softmax / sigmoid) and
// experiments/cora_benchmark_graphsaint.py:105-128
//     loss = (F.nll_loss(out, y, reduction='none') * node_norm)[mask].sum();  acc = (out.argmax(1) == y)[mask].mean()
// Contract: include/ampconv.h, "classifier head".  fp32 arithmetic on the vector ALU; pooled [N, D] is streamed once per
// pass in 16-byte pieces (element-wise where the base, the row stride or D do not allow it: the XOR toy's D = 3).
//
// MAPPING.  A row is walked by a group of G lanes (G = the row's pieces rounded up to a power of two, 4..64), so a
// 256-thread workgroup takes a tile of R = 256 / G rows at a time and every wave instruction reads whole rows.  The
// logits are kCT = 8 register accumulators per lane, summed over the group by an xor butterfly (every lane of the group
// ends with the same bits), and go to a [R, C] LDS scratch -- the only place an [N, C] intermediate ever lives.  W [C, D]
// and b are staged once per workgroup in LDS while the whole layout fits 64 KiB; past that (C = 64 with D >= 256) the
// kernels read W through L2 instead.
// BACKWARD.  dz of a tile is formed in the same scratch (recomputed from pooled for the loss, from dout / out for the
// plain head), dpooled = dz W is written row by row, and dW = dz^T pooled is accumulated in registers: lane (slot, g)
// owns piece g of kCT classes for the rows of its slot.  Workgroups write their partial [C, D + 1] (column D: db) to a
// workspace in a fixed slot order and a second kernel adds the partials in workgroup order: no floating-point atomics,
// the same bits on every launch.  More than kCT classes or more than G pieces per row take further passes over the rows.
// METRICS.  Per-mask loss sums are 64-bit fixed point (AMPCONV_HEAD_LOSS_SHIFT), counts are integers; both are added
// with integer atomics into a per-call scratch, which a one-wave kernel then adds to the caller's running buffer and
// turns into the fp32 loss: order-independent, so bitwise reproducible.
// dispatch, make_geom (with its LDS byte count) and grid_of are mirrored and pinned by tests/test_gpu_head_kernels.py.
#include <type_traits>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kCT = 8;                          // classes per register chunk
constexpr int kMaxBlocks = 1024;                // 256 CUs x 4 workgroups; also the depth of the second reduction stage
constexpr size_t kLdsBytes = 64 * 1024;
constexpr int kSlots = AMPCONV_HEAD_METRICS_SLOTS;
typedef unsigned long long u64;

template <typename T, int NP>
struct alignas(sizeof(T) * NP) Vec {
  T e[NP];
};

struct Geom {
  int64_t N, stride, tiles;                     // rows, elements between rows of pooled, row tiles
  int D, C, P, G, R;                            // P pieces per row, G lanes per row, R rows per tile
  int w_floats, red_floats;                     // LDS floats of W (0: read from global) and of the slot reduction
};

struct Lds {
  float *W, *b, *z, *red;
};
__device__ __forceinline__ Lds carve(float *base, const Geom &q) {
  Lds l;
  l.W = base;
  l.b = l.W + q.w_floats;
  l.z = l.b + ((q.C + 3) & ~3);
  l.red = l.z + ((q.R * q.C + 3) & ~3);
  return l;
}

template <bool WLDS>
__device__ __forceinline__ const float *stage_params(const Lds &l, const float *W, const float *b, const Geom &q) {
  if constexpr (WLDS)
    for (int i = threadIdx.x; i < q.C * q.D; i += kThreads) l.W[i] = W[i];
  if (b)
    for (int i = threadIdx.x; i < q.C; i += kThreads) l.b[i] = b[i];
  __syncthreads();
  return WLDS ? l.W : W;
}

template <int NP>
__device__ __forceinline__ void load_w(const float *w, float (&o)[NP]) {
  if constexpr (NP == 1) {
    o[0] = w[0];
  } else {
#pragma unroll
    for (int k = 0; k < NP / 4; ++k) {
      const float4 v = *reinterpret_cast<const float4 *>(w + 4 * k);
      o[4 * k] = v.x, o[4 * k + 1] = v.y, o[4 * k + 2] = v.z, o[4 * k + 3] = v.w;
    }
  }
}
template <typename T, int NP>
__device__ __forceinline__ void load_x(const T *row, int p, float (&x)[NP]) {
  const Vec<T, NP> v = *reinterpret_cast<const Vec<T, NP> *>(row + (int64_t)p * NP);
#pragma unroll
  for (int j = 0; j < NP; ++j) x[j] = (float)v.e[j];
}
__device__ __forceinline__ float group_sum(float x, int G) {
  for (int o = G >> 1; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// z[c] = b[c] + pooled[n, :] . W[c, :] for the row of this lane's slot (row == nullptr: no row, nothing written).
// The shuffles are outside every divergent branch.  The caller synchronises before z is read.
template <typename T, int NP>
__device__ __forceinline__ void row_logits(const T *row, const float *Wp, const float *bias, float *z, const Geom &q,
                                           int g) {
  for (int c0 = 0; c0 < q.C; c0 += kCT) {
    float acc[kCT];
#pragma unroll
    for (int k = 0; k < kCT; ++k) acc[k] = 0.f;
    if (row)
      for (int p = g; p < q.P; p += q.G) {
        float x[NP];
        load_x<T, NP>(row, p, x);
#pragma unroll
        for (int k = 0; k < kCT; ++k)
          if (c0 + k < q.C) {
            float w[NP];
            load_w<NP>(Wp + (int64_t)(c0 + k) * q.D + p * NP, w);
#pragma unroll
            for (int j = 0; j < NP; ++j) acc[k] = fmaf(x[j], w[j], acc[k]);
          }
      }
#pragma unroll
    for (int k = 0; k < kCT; ++k) acc[k] = group_sum(acc[k], q.G);
    if (row && g == 0) {
#pragma unroll
      for (int k = 0; k < kCT; ++k)
        if (c0 + k < q.C) z[c0 + k] = acc[k] + bias[c0 + k];
    }
  }
}

// log-sum-exp of one row of logits, the row maximum subtracted first
__device__ __forceinline__ float row_lse(const float *z, int C) {
  float m = z[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
  float s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(z[c] - m);
  return m + logf(s);
}

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T, int NP, bool WLDS>
__global__ __launch_bounds__(kThreads) void head_fwd_kernel(const T *__restrict__ X, const float *__restrict__ W,
                                                            const float *__restrict__ b, Geom q, int kind,
                                                            float *__restrict__ out) {
  extern __shared__ float4 smem[];
  const Lds l = carve(reinterpret_cast<float *>(smem), q);
  const float *Wp = stage_params<WLDS>(l, W, b, q);
  const int g = threadIdx.x & (q.G - 1), slot = threadIdx.x / q.G;
  float *z = l.z + slot * q.C;
  for (int64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const int64_t n = tile * q.R + slot;
    const bool valid = n < q.N;
    row_logits<T, NP>(valid ? X + n * q.stride : nullptr, Wp, l.b, z, q, g);
    __syncthreads();
    if (valid) {
      if (kind == AMPCONV_HEAD_LOG_SOFTMAX) {
        const float lse = row_lse(z, q.C);
        for (int c = g; c < q.C; c += q.G) out[n * q.C + c] = z[c] - lse;
      } else {
        for (int c = g; c < q.C; c += q.G) out[n * q.C + c] = 1.f / (1.f + expf(-z[c]));
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// selection of a row by mask m (masks == nullptr: one all-true mask)
__device__ __forceinline__ bool selected(const uint8_t *masks, int m, int64_t N, int64_t n) {
  return masks ? masks[(int64_t)m * N + n] != 0 : true;
}

template <typename T, int NP, bool WLDS>
__global__ __launch_bounds__(kThreads) void head_nll_fwd_kernel(const T *__restrict__ X, const float *__restrict__ W,
                                                                const float *__restrict__ b, Geom q,
                                                                const int64_t *__restrict__ Y,
                                                                const float *__restrict__ wn,
                                                                const uint8_t *__restrict__ masks, int M,
                                                                float *__restrict__ logp, u64 *__restrict__ scratch) {
  extern __shared__ float4 smem[];
  const Lds l = carve(reinterpret_cast<float *>(smem), q);
  const float *Wp = stage_params<WLDS>(l, W, b, q);
  const int g = threadIdx.x & (q.G - 1), slot = threadIdx.x / q.G;
  float *z = l.z + slot * q.C;
  long long acc[kSlots];
#pragma unroll
  for (int i = 0; i < kSlots; ++i) acc[i] = 0;
  for (int64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const int64_t n = tile * q.R + slot;
    const bool valid = n < q.N;
    row_logits<T, NP>(valid ? X + n * q.stride : nullptr, Wp, l.b, z, q, g);
    __syncthreads();
    if (valid) {
      const float lse = row_lse(z, q.C);
      if (logp)
        for (int c = g; c < q.C; c += q.G) logp[n * q.C + c] = z[c] - lse;
      if (g == 0) {
        const int64_t y = Y[n];
        bool any = false;
#pragma unroll
        for (int m = 0; m < AMPCONV_HEAD_MAX_MASKS; ++m) any |= m < M && selected(masks, m, q.N, n);
        if (y == AMPCONV_HEAD_IGNORE_INDEX || !any) {
          // not selected: nothing is counted
        } else if (y < 0 || y >= q.C) {
          acc[kSlots - 1] += 1;                               // a bad label: never used as an index
        } else {
          int best = 0;
          float zb = z[0];
          for (int c = 1; c < q.C; ++c)
            if (z[c] > zb) zb = z[c], best = c;               // ties: the lowest class
          const float term = (wn ? wn[n] : 1.f) * (lse - z[y]);
          const long long fixed = __double2ll_rn((double)term * (double)(1ull << AMPCONV_HEAD_LOSS_SHIFT));
          const long long hit = best == (int)y;
#pragma unroll
          for (int m = 0; m < AMPCONV_HEAD_MAX_MASKS; ++m)
            if (m < M && selected(masks, m, q.N, n)) acc[3 * m] += fixed, acc[3 * m + 1] += 1, acc[3 * m + 2] += hit;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < kSlots; ++i) {
    const long long v = wave_sum_i64(acc[i]);
    if ((threadIdx.x & 63) == 0 && v != 0) atomicAdd(scratch + i, (u64)v);
  }
}

// the call's sums -> the running buffer and the fp32 loss of the gradient mask
__global__ void head_nll_finish_kernel(const u64 *__restrict__ scratch, u64 *__restrict__ metrics, int grad_mask,
                                       float *__restrict__ loss) {
  const int i = threadIdx.x;
  if (metrics && i < kSlots) metrics[i] += scratch[i];
  if (loss && i == 0)
    *loss = (float)((double)(long long)scratch[3 * grad_mask] / (double)(1ull << AMPCONV_HEAD_LOSS_SHIFT));
}

// ---- backward --------------------------------------------------------------------------------------------------------
struct BwdArgs {
  int mode;                                     // AMPCONV_HEAD_LOG_SOFTMAX / _SIGMOID: from dout and out; 2: the loss
  const float *dout, *out;                      // mode 0 / 1
  const float *b;                               // mode 2
  const int64_t *Y;
  const float *wn;
  const uint8_t *mask;                          // row grad_mask of masks, or nullptr
  const float *gscale;                          // upstream gradient, on the device
};

template <typename T, int NP, bool WLDS>
__global__ __launch_bounds__(kThreads) void head_bwd_kernel(const T *__restrict__ X, const float *__restrict__ W,
                                                            Geom q, BwdArgs a, T *__restrict__ dX,
                                                            float *__restrict__ partial) {
  extern __shared__ float4 smem[];
  const Lds l = carve(reinterpret_cast<float *>(smem), q);
  const float *Wp = stage_params<WLDS>(l, W, a.mode == 2 ? a.b : nullptr, q);
  const int g = threadIdx.x & (q.G - 1), slot = threadIdx.x / q.G;
  float *z = l.z + slot * q.C;
  const float gs = a.mode == 2 ? *a.gscale : 0.f;
  float *mine = partial + (int64_t)blockIdx.x * q.C * (q.D + 1);
  for (int c0 = 0; c0 < q.C; c0 += kCT)
    for (int p0 = 0; p0 < q.P; p0 += q.G) {
      const bool first = c0 == 0 && p0 == 0;      // the pass that writes dpooled
      const int p = p0 + g;
      float acc[kCT][NP], accb[kCT];
#pragma unroll
      for (int k = 0; k < kCT; ++k) {
        accb[k] = 0.f;
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[k][j] = 0.f;
      }
      for (int64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
        const int64_t n = tile * q.R + slot;
        const bool valid = n < q.N;
        const T *row = valid ? X + n * q.stride : nullptr;
        bool live = valid;                        // the row has a gradient
        if (a.mode == 2) {
          int64_t y = -1;
          float coef = 0.f;
          if (valid) {
            y = a.Y[n];
            if (y >= 0 && y < q.C && (a.mask ? a.mask[n] != 0 : true)) coef = gs * (a.wn ? a.wn[n] : 1.f);
          }
          live = coef != 0.f;
          row_logits<T, NP>(live ? row : nullptr, Wp, l.b, z, q, g);
          __syncthreads();
          float lse = 0.f;
          if (live) lse = row_lse(z, q.C);
          __syncthreads();
          if (live)
            for (int c = g; c < q.C; c += q.G) z[c] = coef * (expf(z[c] - lse) - (c == (int)y ? 1.f : 0.f));
        } else {
          float s = 0.f;
          if (valid && a.mode == AMPCONV_HEAD_LOG_SOFTMAX)
            for (int c = g; c < q.C; c += q.G) s += a.dout[n * q.C + c];
          s = group_sum(s, q.G);
          if (valid)
            for (int c = g; c < q.C; c += q.G) {
              const float d = a.dout[n * q.C + c], o = a.out[n * q.C + c];
              z[c] = a.mode == AMPCONV_HEAD_LOG_SOFTMAX ? d - expf(o) * s : d * o * (1.f - o);
            }
        }
        __syncthreads();
        if (first && valid && dX) {
          T *drow = dX + n * q.D;
          for (int pp = g; pp < q.P; pp += q.G) {
            float o[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) o[j] = 0.f;
            if (live)
              for (int c = 0; c < q.C; ++c) {
                float w[NP];
                load_w<NP>(Wp + (int64_t)c * q.D + pp * NP, w);
                const float dz = z[c];
#pragma unroll
                for (int j = 0; j < NP; ++j) o[j] = fmaf(dz, w[j], o[j]);
              }
            Vec<T, NP> v;
#pragma unroll
            for (int j = 0; j < NP; ++j) v.e[j] = (T)o[j];
            *reinterpret_cast<Vec<T, NP> *>(drow + (int64_t)pp * NP) = v;
          }
        }
        if (live && p < q.P) {
          float x[NP];
          load_x<T, NP>(row, p, x);
#pragma unroll
          for (int k = 0; k < kCT; ++k)
            if (c0 + k < q.C) {
              const float dz = z[c0 + k];
#pragma unroll
              for (int j = 0; j < NP; ++j) acc[k][j] = fmaf(dz, x[j], acc[k][j]);
              if (p == 0) accb[k] += dz;
            }
        }
        __syncthreads();
      }
      // the slots of the workgroup, added in slot order
      for (int r = 1; r < q.R; ++r) {
        if (slot == r) {
#pragma unroll
          for (int k = 0; k < kCT; ++k) {
#pragma unroll
            for (int j = 0; j < NP; ++j) l.red[(g * kCT + k) * NP + j] = acc[k][j];
            if (g == 0) l.red[q.G * kCT * NP + k] = accb[k];
          }
        }
        __syncthreads();
        if (slot == 0) {
#pragma unroll
          for (int k = 0; k < kCT; ++k) {
#pragma unroll
            for (int j = 0; j < NP; ++j) acc[k][j] += l.red[(g * kCT + k) * NP + j];
            if (g == 0) accb[k] += l.red[q.G * kCT * NP + k];
          }
        }
        __syncthreads();
      }
      if (slot == 0) {
#pragma unroll
        for (int k = 0; k < kCT; ++k)
          if (c0 + k < q.C) {
            float *dst = mine + (int64_t)(c0 + k) * (q.D + 1);
            if (p < q.P) {
#pragma unroll
              for (int j = 0; j < NP; ++j) dst[p * NP + j] = acc[k][j];
            }
            if (p == 0) dst[q.D] = accb[k];
          }
      }
    }
}

// dW[c, d] / db[c] = the workgroups' partials added in workgroup order (four independent loads in flight)
__global__ __launch_bounds__(kThreads) void head_reduce_kernel(const float *__restrict__ partial, int blocks, int C,
                                                               int D, float *__restrict__ dW, float *__restrict__ db) {
  const int64_t per = (int64_t)C * (D + 1);
  const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (e >= per) return;
  float s = 0.f;
  int i = 0;
  for (; i + 4 <= blocks; i += 4) {
    const float v0 = partial[(int64_t)i * per + e], v1 = partial[(int64_t)(i + 1) * per + e],
                v2 = partial[(int64_t)(i + 2) * per + e], v3 = partial[(int64_t)(i + 3) * per + e];
    s = (((s + v0) + v1) + v2) + v3;
  }
  for (; i < blocks; ++i) s += partial[(int64_t)i * per + e];
  const int c = (int)(e / (D + 1)), d = (int)(e - (int64_t)c * (D + 1));
  if (d < D) dW[(int64_t)c * D + d] = s;
  else db[c] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

inline int64_t row_tiles_bound(int64_t N) { return (N + 3) / 4; }          // R >= 4 rows per tile whatever the path
inline int64_t blocks_bound(int64_t N) {
  const int64_t t = row_tiles_bound(N);
  return t < kMaxBlocks ? t : kMaxBlocks;
}

inline bool dims_ok(int64_t N, int D, int C, int64_t stride) {
  return N >= 0 && D >= 1 && C >= 1 && C <= AMPCONV_HEAD_MAX_CLASSES && stride >= D &&
         (N == 0 || stride <= INT64_MAX / N) && N <= INT64_MAX / ((int64_t)D > C ? D : C);
}

inline Geom make_geom(int64_t N, int D, int C, int64_t stride, int NP, bool bwd, bool &wlds) {
  Geom q{};
  q.N = N, q.stride = stride, q.D = D, q.C = C;
  q.P = D / NP;
  int G = 4;
  while (G < q.P && G < 64) G <<= 1;
  q.G = G, q.R = kThreads / G;
  q.tiles = (N + q.R - 1) / q.R;
  q.red_floats = bwd ? G * kCT * NP + kCT : 0;
  const size_t rest = (size_t)(((C + 3) & ~3) + ((q.R * C + 3) & ~3) + q.red_floats) * sizeof(float);
  const size_t w_floats = ((size_t)C * D + 3) & ~(size_t)3;
  wlds = rest + w_floats * sizeof(float) <= kLdsBytes;
  q.w_floats = wlds ? (int)w_floats : 0;
  return q;
}
inline size_t lds_bytes(const Geom &q) {
  return (size_t)(q.w_floats + ((q.C + 3) & ~3) + ((q.R * q.C + 3) & ~3) + q.red_floats) * sizeof(float);
}
inline unsigned grid_of(const Geom &q) { return (unsigned)(q.tiles < kMaxBlocks ? q.tiles : kMaxBlocks); }

// f(T{}, integral_constant<int, NP>{}, integral_constant<bool, WLDS>{}) for the storage, the access width and the home
// of W of a call.  vec: every row of every streamed tensor starts on a 16-byte boundary and holds whole pieces.
template <typename F>
int dispatch(int dtype, int64_t N, int D, int C, int64_t stride, bool ptrs_aligned, bool bwd, const F &f) {
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  auto go = [&](auto t, auto np) -> int {
    using T = decltype(t);
    constexpr int NP = decltype(np)::value;
    bool wlds;
    const Geom q = make_geom(N, D, C, stride, NP, bwd, wlds);
    return wlds ? f(t, np, std::true_type{}, q) : f(t, np, std::false_type{}, q);
  };
  auto by_type = [&](auto t) -> int {
    using T = decltype(t);
    constexpr int NPV = 16 / (int)sizeof(T);
    const bool vec = ptrs_aligned && D % NPV == 0 && stride % NPV == 0;
    return vec ? go(t, std::integral_constant<int, NPV>{}) : go(t, std::integral_constant<int, 1>{});
  };
  return dtype == AMPCONV_BF16 ? by_type(__bf16{}) : by_type(float{});
}

int reduce_partials(const float *ws, int blocks, int C, int D, float *dW, float *db, hipStream_t s) {
  const int64_t per = (int64_t)C * (D + 1);
  head_reduce_kernel<<<(unsigned)((per + kThreads - 1) / kThreads), kThreads, 0, s>>>(ws, blocks, C, D, dW, db);
  return ampconv_launch_status();
}

int run_bwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, int C, const BwdArgs &a, void *dpooled,
            float *dW, float *db, void *ws, size_t ws_bytes, int dtype, hipStream_t s) {
  if (!dims_ok(N, D, C, stride)) return AMPCONV_E_BADARG;
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  if (!W || !dW || !db) return AMPCONV_E_BADARG;
  if (N == 0) return reduce_partials(nullptr, 0, C, D, dW, db, s);
  if (!pooled || !ws) return AMPCONV_E_BADARG;
  if (ws_bytes < ampconv_head_workspace_bytes(N, D, C)) return AMPCONV_E_WORKSPACE;
  const bool al = aligned16(pooled) && aligned16(W) && (!dpooled || aligned16(dpooled));
  int blocks = 0;
  const int rc = dispatch(dtype, N, D, C, stride, al, true, [&](auto t, auto np, auto wl, const Geom &q) -> int {
    using T = decltype(t);
    blocks = (int)grid_of(q);
    head_bwd_kernel<T, decltype(np)::value, decltype(wl)::value><<<grid_of(q), kThreads, lds_bytes(q), s>>>(
        (const T *)pooled, W, q, a, (T *)dpooled, (float *)ws);
    return ampconv_launch_status();
  });
  if (rc) return rc;
  return reduce_partials((const float *)ws, blocks, C, D, dW, db, s);
}

}  // namespace

extern "C" size_t ampconv_head_workspace_bytes(int64_t N, int D, int C) {
  if (N <= 0 || D < 1 || C < 1) return 0;
  return (size_t)blocks_bound(N) * (size_t)C * (size_t)(D + 1) * sizeof(float);
}

extern "C" int ampconv_head_fwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, const float *b,
                                int C, int kind, float *out, int dtype, void *stream) {
  if (!dims_ok(N, D, C, stride)) return AMPCONV_E_BADARG;
  if (kind != AMPCONV_HEAD_LOG_SOFTMAX && kind != AMPCONV_HEAD_SIGMOID) return AMPCONV_E_BADARG;
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  if (N == 0) return AMPCONV_OK;
  if (!pooled || !W || !b || !out) return AMPCONV_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  return dispatch(dtype, N, D, C, stride, aligned16(pooled) && aligned16(W), false,
                  [&](auto t, auto np, auto wl, const Geom &q) -> int {
                    using T = decltype(t);
                    head_fwd_kernel<T, decltype(np)::value, decltype(wl)::value>
                        <<<grid_of(q), kThreads, lds_bytes(q), s>>>((const T *)pooled, W, b, q, kind, out);
                    return ampconv_launch_status();
                  });
}

extern "C" int ampconv_head_bwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, int C, int kind,
                                const float *dout, const float *out, void *dpooled, float *dW, float *db,
                                void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  if (kind != AMPCONV_HEAD_LOG_SOFTMAX && kind != AMPCONV_HEAD_SIGMOID) return AMPCONV_E_BADARG;
  if (N > 0 && (!dout || !out)) return AMPCONV_E_BADARG;
  BwdArgs a{};
  a.mode = kind, a.dout = dout, a.out = out;
  return run_bwd(pooled, N, D, stride, W, C, a, dpooled, dW, db, workspace, workspace_bytes, dtype,
                 (hipStream_t)stream);
}

extern "C" int ampconv_head_nll_fwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W,
                                    const float *b, int C, const int64_t *y, const float *w, const uint8_t *masks,
                                    int M, int grad_mask, float *logp, int64_t *metrics, int64_t *scratch,
                                    float *loss, int dtype, void *stream) {
  if (!dims_ok(N, D, C, stride)) return AMPCONV_E_BADARG;
  if (M < 1 || M > AMPCONV_HEAD_MAX_MASKS || grad_mask < 0 || grad_mask >= M) return AMPCONV_E_BADARG;
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  if (!scratch || (N > 0 && (!pooled || !W || !b || !y))) return AMPCONV_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemsetAsync(scratch, 0, kSlots * sizeof(int64_t), s); e != hipSuccess) return (int)e;
  if (N > 0) {
    const int rc = dispatch(dtype, N, D, C, stride, aligned16(pooled) && aligned16(W), false,
                            [&](auto t, auto np, auto wl, const Geom &q) -> int {
                              using T = decltype(t);
                              head_nll_fwd_kernel<T, decltype(np)::value, decltype(wl)::value>
                                  <<<grid_of(q), kThreads, lds_bytes(q), s>>>((const T *)pooled, W, b, q, y, w, masks,
                                                                             M, logp, (u64 *)scratch);
                              return ampconv_launch_status();
                            });
    if (rc) return rc;
  }
  head_nll_finish_kernel<<<1, 64, 0, s>>>((const u64 *)scratch, (u64 *)metrics, grad_mask, loss);
  return ampconv_launch_status();
}

extern "C" int ampconv_head_nll_bwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W,
                                    const float *b, int C, const int64_t *y, const float *w, const uint8_t *masks,
                                    int M, int grad_mask, const float *g, void *dpooled, float *dW, float *db,
                                    void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  if (M < 1 || M > AMPCONV_HEAD_MAX_MASKS || grad_mask < 0 || grad_mask >= M) return AMPCONV_E_BADARG;
  if (N > 0 && (!b || !y || !g)) return AMPCONV_E_BADARG;
  BwdArgs a{};
  a.mode = 2, a.b = b, a.Y = y, a.wn = w, a.gscale = g;
  a.mask = masks && N >= 0 ? masks + (int64_t)grad_mask * N : nullptr;
  return run_bwd(pooled, N, D, stride, W, C, a, dpooled, dW, db, workspace, workspace_bytes, dtype,
                 (hipStream_t)stream);
}
