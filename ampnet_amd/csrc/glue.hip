// The glue around the AMPConv layers of the reference's models: activation + dropout between the layers and
// activation + dropout + token pooling after the last one, each as ONE pass over [N, L*D] with the dropout mask
// regenerated from (seed, element index) instead of stored.
// Reference: src/ampnet/module/amp_gcn.py:239-276
//   :252      x = self.drop1(x)                                  act_dropout, identity
//   :256-257  x = F.relu(x); x = self.drop2(x)                   act_dropout, ReLU
//   :264-271  F.relu -> drop3 -> reshape [N, L, D] -> mean(dim=1) / [:, 0]     pool
// and amp_net_classifier_Rahul.py:45-57, the same with F.elu.
// All four operations stream their tensors once: 16 bytes per lane, a wave's lanes on consecutive 16-byte pieces,
// four loads in flight per lane and stream, no LDS.  Bases that are not 16-byte aligned and rows that are no multiple
// of 16 bytes (the XOR toy: L = 2, D = 3) take the element-wise kernels at the end of each section.
// The launch arithmetic (vec / scalar, capped_blocks, pool_grid) is mirrored and pinned by tests/test_gpu_glue_kernels.py.
#include "site_common.h"

namespace {

constexpr int kUnroll = 4;                      // 16-byte loads in flight per lane and input stream
constexpr int kMaxBlocks = 2048;                // grid-stride beyond 256 CUs x 8 workgroups

// ---- activation + dropout, element-wise ----------------------------------------------------------------------------
template <typename T, int ACT>
__device__ __forceinline__ Piece<T> act_dropout_piece(const Piece<T> &x, uint32_t keep, float scale) {
  Piece<T> y;
#pragma unroll
  for (int k = 0; k < Piece<T>::N; ++k) y.e[k] = (T)((keep >> k) & 1 ? act_value<ACT>((float)x.e[k]) * scale : 0.f);
  return y;
}
template <typename T, int ACT>
__device__ __forceinline__ Piece<T> act_dropout_grad_piece(const Piece<T> &dy, const Piece<T> &y, uint32_t keep,
                                                           float scale, float inv_scale) {
  Piece<T> dx;
#pragma unroll
  for (int k = 0; k < Piece<T>::N; ++k) {
    const float slope = ACT == AMPCONV_ACT_IDENTITY ? 1.f : act_slope_of_value<ACT>((float)y.e[k] * inv_scale);
    dx.e[k] = (T)((keep >> k) & 1 ? (float)dy.e[k] * scale * slope : 0.f);
  }
  return dx;
}

// a workgroup takes tiles of kUnroll x 256 consecutive pieces: every wave instruction covers 1 KiB
template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_dropout_fwd_vec(const T *__restrict__ X, int64_t pieces, uint64_t seed,
                                                           uint32_t thr, float scale, T *__restrict__ Y) {
  constexpr int NP = Piece<T>::N;
  const Piece<T> *x = reinterpret_cast<const Piece<T> *>(X);
  Piece<T> *y = reinterpret_cast<Piece<T> *>(Y);
  const int64_t tile = 256 * kUnroll, step = (int64_t)gridDim.x * tile;
  for (int64_t base = (int64_t)blockIdx.x * tile; base < pieces; base += step) {
    const int64_t q0 = base + threadIdx.x;
    if (base + tile <= pieces) {
      Piece<T> v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = x[q0 + u * 256];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t q = q0 + u * 256;
        y[q] = act_dropout_piece<T, ACT>(v[u], keep_bits<NP>(seed, thr, (uint64_t)q * (NP / 4)), scale);
      }
    } else {
      for (int64_t q = q0; q < pieces; q += 256)
        y[q] = act_dropout_piece<T, ACT>(x[q], keep_bits<NP>(seed, thr, (uint64_t)q * (NP / 4)), scale);
    }
  }
}

// Yv (the saved output) is not read for the identity
template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_dropout_bwd_vec(const T *__restrict__ dY, const T *__restrict__ Yv,
                                                           int64_t pieces, uint64_t seed, uint32_t thr, float scale,
                                                           T *__restrict__ dX) {
  constexpr int NP = Piece<T>::N;
  constexpr bool kNeedY = ACT != AMPCONV_ACT_IDENTITY;
  const Piece<T> *dy = reinterpret_cast<const Piece<T> *>(dY);
  const Piece<T> *y = reinterpret_cast<const Piece<T> *>(Yv);
  Piece<T> *dx = reinterpret_cast<Piece<T> *>(dX);
  const float inv_scale = 1.f / scale;
  const int64_t tile = 256 * kUnroll, step = (int64_t)gridDim.x * tile;
  for (int64_t base = (int64_t)blockIdx.x * tile; base < pieces; base += step) {
    const int64_t q0 = base + threadIdx.x;
    if (base + tile <= pieces) {
      Piece<T> g[kUnroll], v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        g[u] = dy[q0 + u * 256];
        if constexpr (kNeedY) v[u] = y[q0 + u * 256];
        else v[u] = g[u];
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int64_t q = q0 + u * 256;
        dx[q] = act_dropout_grad_piece<T, ACT>(g[u], v[u], keep_bits<NP>(seed, thr, (uint64_t)q * (NP / 4)), scale,
                                               inv_scale);
      }
    } else {
      for (int64_t q = q0; q < pieces; q += 256) {
        const Piece<T> g = dy[q];
        dx[q] = act_dropout_grad_piece<T, ACT>(g, kNeedY ? y[q] : g, keep_bits<NP>(seed, thr, (uint64_t)q * (NP / 4)),
                                               scale, inv_scale);
      }
    }
  }
}

template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_dropout_fwd_scalar(const T *__restrict__ X, int64_t n, uint64_t seed,
                                                              uint32_t thr, float scale, T *__restrict__ Y) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step)
    Y[i] = (T)(keep_one(seed, thr, (uint64_t)i) ? act_value<ACT>((float)X[i]) * scale : 0.f);
}
template <typename T, int ACT>
__global__ __launch_bounds__(256) void act_dropout_bwd_scalar(const T *__restrict__ dY, const T *__restrict__ Yv,
                                                              int64_t n, uint64_t seed, uint32_t thr, float scale,
                                                              T *__restrict__ dX) {
  const float inv_scale = 1.f / scale;
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    float slope = 1.f;
    if constexpr (ACT != AMPCONV_ACT_IDENTITY) slope = act_slope_of_value<ACT>((float)Yv[i] * inv_scale);
    dX[i] = (T)(keep_one(seed, thr, (uint64_t)i) ? (float)dY[i] * scale * slope : 0.f);
  }
}

// ---- activation + dropout + token pooling --------------------------------------------------------------------------
// One lane per (node, 16-byte column piece), consecutive lanes on consecutive pieces -- every lane of a wave works
// whatever the row length (D = 100 fp32 is 25 pieces: a wave spans 2.56 nodes) -- and walks the node's tokens in
// ascending order, kUnroll rows in flight: one fp32 chain per column, no atomics, the same bits on every launch.
// `tokens` = L for the token mean, 1 for token-0 pooling (inv = 1 / L resp. 1); P = 16-byte pieces per token row.
template <typename T, int ACT>
__global__ __launch_bounds__(256) void pool_fwd_vec(const T *__restrict__ X, int64_t units, int L, int P, int tokens,
                                                    float inv, uint64_t seed, uint32_t thr, float scale,
                                                    T *__restrict__ pooled) {
  constexpr int NP = Piece<T>::N;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= units) return;
  const int64_t n = t / P;
  const int p = (int)(t - n * P);
  const int64_t q0 = n * L * P + p;                   // piece index of (n, token 0, p) in the flat tensor
  const Piece<T> *x = reinterpret_cast<const Piece<T> *>(X);
  float acc[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) acc[k] = 0.f;
  int l = 0;
  for (; l + kUnroll <= tokens; l += kUnroll) {
    Piece<T> v[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) v[u] = x[q0 + (int64_t)(l + u) * P];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t keep = keep_bits<NP>(seed, thr, (uint64_t)(q0 + (int64_t)(l + u) * P) * (NP / 4));
#pragma unroll
      for (int k = 0; k < NP; ++k) acc[k] += (keep >> k) & 1 ? act_value<ACT>((float)v[u].e[k]) * scale : 0.f;
    }
  }
  for (; l < tokens; ++l) {
    const Piece<T> v = x[q0 + (int64_t)l * P];
    const uint32_t keep = keep_bits<NP>(seed, thr, (uint64_t)(q0 + (int64_t)l * P) * (NP / 4));
#pragma unroll
    for (int k = 0; k < NP; ++k) acc[k] += (keep >> k) & 1 ? act_value<ACT>((float)v.e[k]) * scale : 0.f;
  }
  Piece<T> out;
#pragma unroll
  for (int k = 0; k < NP; ++k) out.e[k] = (T)(acc[k] * inv);
  reinterpret_cast<Piece<T> *>(pooled)[t] = out;
}

// dx[n, l, :] = act'(x) keep scale dpooled[n, :] / L for l < tokens, exact zeros for the rows behind (token-0 pooling)
template <typename T, int ACT>
__global__ __launch_bounds__(256) void pool_bwd_vec(const T *__restrict__ X, const T *__restrict__ dpooled,
                                                    int64_t units, int L, int P, int tokens, float inv, uint64_t seed,
                                                    uint32_t thr, float scale, T *__restrict__ dX) {
  constexpr int NP = Piece<T>::N;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= units) return;
  const int64_t n = t / P;
  const int p = (int)(t - n * P);
  const int64_t q0 = n * L * P + p;
  const Piece<T> *x = reinterpret_cast<const Piece<T> *>(X);
  Piece<T> *dx = reinterpret_cast<Piece<T> *>(dX);
  const Piece<T> gp = reinterpret_cast<const Piece<T> *>(dpooled)[t];
  float g[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) g[k] = (float)gp.e[k] * inv * scale;
  auto grad = [&](const Piece<T> &v, int64_t q) {
    const uint32_t keep = keep_bits<NP>(seed, thr, (uint64_t)q * (NP / 4));
    Piece<T> d;
#pragma unroll
    for (int k = 0; k < NP; ++k) d.e[k] = (T)((keep >> k) & 1 ? g[k] * act_slope_of_input<ACT>((float)v.e[k]) : 0.f);
    return d;
  };
  int l = 0;
  if constexpr (ACT == AMPCONV_ACT_IDENTITY) {          // x is not read: the slope is 1
    Piece<T> none;
#pragma unroll
    for (int k = 0; k < NP; ++k) none.e[k] = (T)0.f;
    for (; l < tokens; ++l) dx[q0 + (int64_t)l * P] = grad(none, q0 + (int64_t)l * P);
  } else {
    for (; l + kUnroll <= tokens; l += kUnroll) {
      Piece<T> v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) v[u] = x[q0 + (int64_t)(l + u) * P];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) dx[q0 + (int64_t)(l + u) * P] = grad(v[u], q0 + (int64_t)(l + u) * P);
    }
    for (; l < tokens; ++l) dx[q0 + (int64_t)l * P] = grad(x[q0 + (int64_t)l * P], q0 + (int64_t)l * P);
  }
  Piece<T> zero;
#pragma unroll
  for (int k = 0; k < NP; ++k) zero.e[k] = (T)0.f;
  for (; l < L; ++l) dx[q0 + (int64_t)l * P] = zero;
}

// one lane per (node, channel)
template <typename T, int ACT>
__global__ __launch_bounds__(256) void pool_fwd_scalar(const T *__restrict__ X, int64_t units, int L, int D, int tokens,
                                                       float inv, uint64_t seed, uint32_t thr, float scale,
                                                       T *__restrict__ pooled) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= units) return;
  const int64_t n = t / D;
  const int64_t i0 = n * L * D + (t - n * D);
  float acc = 0.f;
  for (int l = 0; l < tokens; ++l) {
    const int64_t i = i0 + (int64_t)l * D;
    acc += keep_one(seed, thr, (uint64_t)i) ? act_value<ACT>((float)X[i]) * scale : 0.f;
  }
  pooled[t] = (T)(acc * inv);
}
template <typename T, int ACT>
__global__ __launch_bounds__(256) void pool_bwd_scalar(const T *__restrict__ X, const T *__restrict__ dpooled,
                                                       int64_t units, int L, int D, int tokens, float inv,
                                                       uint64_t seed, uint32_t thr, float scale, T *__restrict__ dX) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= units) return;
  const int64_t n = t / D;
  const int64_t i0 = n * L * D + (t - n * D);
  const float g = (float)dpooled[t] * inv * scale;
  int l = 0;
  for (; l < tokens; ++l) {
    const int64_t i = i0 + (int64_t)l * D;
    float slope = 1.f;
    if constexpr (ACT != AMPCONV_ACT_IDENTITY) slope = act_slope_of_input<ACT>((float)X[i]);
    dX[i] = (T)(keep_one(seed, thr, (uint64_t)i) ? g * slope : 0.f);
  }
  for (; l < L; ++l) dX[i0 + (int64_t)l * D] = (T)0.f;
}

inline unsigned capped_blocks(int64_t work_items, int64_t per_block) {
  const int64_t b = (work_items + per_block - 1) / per_block;
  return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}

}  // namespace

extern "C" int ampconv_act_dropout_fwd(const void *x, int64_t n, int act, uint64_t seed, uint32_t threshold,
                                       float scale, void *y, int dtype, void *stream) {
  if (n < 0 || !mask_args_ok(threshold, scale)) return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T = decltype(t);
    constexpr int ACT = decltype(a)::value, NP = Piece<T>::N;
    if (n == 0) return AMPCONV_OK;
    if (!x || !y) return AMPCONV_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(x) && aligned16(y) && n % NP == 0)
      act_dropout_fwd_vec<T, ACT><<<capped_blocks(n / NP, 256 * kUnroll), 256, 0, s>>>((const T *)x, n / NP, seed,
                                                                                       threshold, scale, (T *)y);
    else
      act_dropout_fwd_scalar<T, ACT><<<capped_blocks(n, 256), 256, 0, s>>>((const T *)x, n, seed, threshold, scale,
                                                                           (T *)y);
    return ampconv_launch_status();
  });
}

extern "C" int ampconv_act_dropout_bwd(const void *dy, const void *y, int64_t n, int act, uint64_t seed,
                                       uint32_t threshold, float scale, void *dx, int dtype, void *stream) {
  if (n < 0 || !mask_args_ok(threshold, scale)) return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T = decltype(t);
    constexpr int ACT = decltype(a)::value, NP = Piece<T>::N;
    if (n == 0) return AMPCONV_OK;
    const bool need_y = ACT != AMPCONV_ACT_IDENTITY;
    if (!dy || !dx || (need_y && !y)) return AMPCONV_E_BADARG;
    hipStream_t s = (hipStream_t)stream;
    if (aligned16(dy) && aligned16(dx) && (!need_y || aligned16(y)) && n % NP == 0)
      act_dropout_bwd_vec<T, ACT><<<capped_blocks(n / NP, 256 * kUnroll), 256, 0, s>>>(
          (const T *)dy, (const T *)y, n / NP, seed, threshold, scale, (T *)dx);
    else
      act_dropout_bwd_scalar<T, ACT><<<capped_blocks(n, 256), 256, 0, s>>>((const T *)dy, (const T *)y, n, seed,
                                                                           threshold, scale, (T *)dx);
    return ampconv_launch_status();
  });
}

namespace {
// work items and the launch grid of the pooling kernels; false: does not fit a launch
inline bool pool_grid(int64_t N, int per_node, int64_t &units, unsigned &blocks) {
  units = N * per_node;
  const int64_t b = (units + 255) / 256;
  blocks = (unsigned)b;
  return b <= INT32_MAX;
}
inline bool pool_args_ok(int64_t N, int L, int D, int pooling, uint32_t thr, float scale) {
  return N >= 0 && L > 0 && D > 0 && (pooling == AMPCONV_POOL_MEAN || pooling == AMPCONV_POOL_TOKEN0) &&
         mask_args_ok(thr, scale) && N <= INT64_MAX / ((int64_t)L * D);
}
}  // namespace

extern "C" int ampconv_pool_fwd(const void *x, int64_t N, int L, int D, int act, int pooling, uint64_t seed,
                                uint32_t threshold, float scale, void *pooled, int dtype, void *stream) {
  if (!pool_args_ok(N, L, D, pooling, threshold, scale)) return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T = decltype(t);
    constexpr int ACT = decltype(a)::value, NP = Piece<T>::N;
    if (N == 0) return AMPCONV_OK;
    if (!x || !pooled) return AMPCONV_E_BADARG;
    const int tokens = pooling == AMPCONV_POOL_TOKEN0 ? 1 : L;
    const float inv = 1.f / (float)tokens;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = aligned16(x) && aligned16(pooled) && D % NP == 0;
    int64_t units;
    unsigned blocks;
    if (!pool_grid(N, vec ? D / NP : D, units, blocks)) return AMPCONV_E_BADARG;
    if (vec)
      pool_fwd_vec<T, ACT><<<blocks, 256, 0, s>>>((const T *)x, units, L, D / NP, tokens, inv, seed, threshold, scale,
                                                  (T *)pooled);
    else
      pool_fwd_scalar<T, ACT><<<blocks, 256, 0, s>>>((const T *)x, units, L, D, tokens, inv, seed, threshold, scale,
                                                     (T *)pooled);
    return ampconv_launch_status();
  });
}

extern "C" int ampconv_pool_bwd(const void *x, const void *dpooled, int64_t N, int L, int D, int act, int pooling,
                                uint64_t seed, uint32_t threshold, float scale, void *dx, int dtype, void *stream) {
  if (!pool_args_ok(N, L, D, pooling, threshold, scale)) return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T = decltype(t);
    constexpr int ACT = decltype(a)::value, NP = Piece<T>::N;
    if (N == 0) return AMPCONV_OK;
    const bool need_x = ACT != AMPCONV_ACT_IDENTITY;
    if (!dpooled || !dx || (need_x && !x)) return AMPCONV_E_BADARG;
    const int tokens = pooling == AMPCONV_POOL_TOKEN0 ? 1 : L;
    const float inv = 1.f / (float)tokens;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = (!need_x || aligned16(x)) && aligned16(dpooled) && aligned16(dx) && D % NP == 0;
    int64_t units;
    unsigned blocks;
    if (!pool_grid(N, vec ? D / NP : D, units, blocks)) return AMPCONV_E_BADARG;
    if (vec)
      pool_bwd_vec<T, ACT><<<blocks, 256, 0, s>>>((const T *)x, (const T *)dpooled, units, L, D / NP, tokens, inv, seed,
                                                  threshold, scale, (T *)dx);
    else
      pool_bwd_scalar<T, ACT><<<blocks, 256, 0, s>>>((const T *)x, (const T *)dpooled, units, L, D, tokens, inv, seed,
                                                     threshold, scale, (T *)dx);
    return ampconv_launch_status();
  });
}
