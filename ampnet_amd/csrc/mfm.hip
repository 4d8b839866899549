// Masked feature modelling: the featuriser's build with the token masking fused in, the gradient of the mask token, and
// the value decoder with its mean-squared loss over the masked tokens, one pass per direction.
// Reference: every model class carries the masked-autoencoder parameter (src/ampnet/module/gcn_one_layer.py:43-54,
// commented out in amp_gcn.py:60), gcn_classifier.py:138-151 replaces whole token vectors by it in a Python loop over
// nodes x features, and experiments/predictive_ssl_AMPNet.py stops at `criterion = None`.
// Contract: include/ampconv.h, "MASKED FEATURE MODELLING".  fp32 arithmetic on the vector ALU.
//
// MAPPING (norm.hip's rows, head.hip's tiles).  A token row is walked by a group of G lanes (G = the row's pieces rounded
// up to a power of two, 4..64): lane g takes pieces g, g + G, ...  A 256-thread workgroup takes a tile of R = 256 / G
// consecutive tokens at a time and strides over the tiles by the grid.  A group whose token is not masked issues no load:
// at rate 0.15 the loss kernels touch 15 % of h.  Pieces are 16 bytes (bf16: 8 bytes where only those fit, D = 100),
// single elements where the bases or D do not allow it.
// SUMS OVER TOKENS (dw, db, dmask_token).  A lane keeps the fp32 sums of its piece over the tokens of its slot, in tile
// order; the R slots of the workgroup are added in slot order through LDS into the workgroup's row of the workspace;
// mfm_fold_kernel adds the rows in workgroup order.  More than G pieces per row take further passes over the tokens.  The
// grid is a function of the shape alone: the same bits on every launch, no floating-point atomics.
// THE LOSS.  Squared residuals in 64-bit fixed point and the count, per-lane integer sums, a butterfly over the wave, one
// integer atomic per wave into the call's `state`; a one-wave kernel then adds state to the running buffer and writes the
// fp32 loss.  The backward pass reads the count and the upstream gradient from the device.
#include <type_traits>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;                // 256 CUs x 4 workgroups; also the depth of the second reduction stage
constexpr int kMaxNP = 8;                       // elements of the widest piece (16 bytes of bf16)
typedef unsigned long long u64;

template <typename T, int NP>
struct alignas(sizeof(T) * NP) Vec {
  T e[NP];
};

struct Geom {
  int64_t T, tiles;                             // tokens, token tiles
  int D, c0, P, G, R;                           // row width, first column and pieces of the part that is read, lanes per
};                                              // row, rows per tile

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
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the build -------------------------------------------------------------------------------------------------------
// one element per lane; the expressions of build_tokens_kernel (featurizer.hip), so that unmasked tokens have its bits
template <typename T>
__global__ __launch_bounds__(kThreads) void mfm_build_kernel(const float *__restrict__ x, const float *__restrict__ mean,
                                                             const float *__restrict__ inv_std,
                                                             const int32_t *__restrict__ idx,
                                                             const float *__restrict__ table,
                                                             const float *__restrict__ token, Geom q, int F, int L,
                                                             uint64_t seed, uint32_t thr, int mode,
                                                             const uint8_t *__restrict__ masked_in, T *__restrict__ out,
                                                             uint8_t *__restrict__ masked, float *__restrict__ target) {
  const int g = threadIdx.x & (q.G - 1), slot = threadIdx.x / q.G;
  const int De = q.D - 1;
  for (int64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const int64_t t = tile * q.R + slot;
    if (t >= q.T) continue;
    const int f = idx[t];
    const int64_t n = t / L;
    const int l = (int)(t - n * L);
    T *o = out + t * q.D;
    if (f < 0) {
      for (int c = g; c <= De; c += q.G) o[c] = (T)0.f;
      if (g == 0) masked[t] = 0, target[t] = 0.f;
      continue;
    }
    const bool m = masked_in ? masked_in[t] != 0 : (uint32_t)(draw(seed, (uint64_t)n, (uint64_t)l) >> 48) < thr;
    const float z = (x[n * (int64_t)F + f] - mean[f]) * inv_std[f];
    if (m && mode == AMPCONV_MFM_TOKEN) {
      for (int c = g; c <= De; c += q.G) o[c] = (T)token[c];
    } else {
      for (int c = g; c < De; c += q.G) o[c] = (T)table[(int64_t)f * De + c];
      if (g == 0) o[De] = (T)(m ? token[De] : z);
    }
    if (g == 0) masked[t] = m ? 1 : 0, target[t] = z;
  }
}

// ---- decoder and loss, forward ---------------------------------------------------------------------------------------
template <typename T, int NP>
__global__ __launch_bounds__(kThreads) void mfm_loss_fwd_kernel(const T *__restrict__ H, const uint8_t *__restrict__ masked,
                                                                const float *__restrict__ target,
                                                                const float *__restrict__ w, const float *__restrict__ b,
                                                                Geom q, float *__restrict__ resid,
                                                                u64 *__restrict__ state) {
  const int g = threadIdx.x & (q.G - 1), slot = threadIdx.x / q.G;
  const float bias = *b;
  long long sq = 0, cnt = 0;
  for (int64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
    const int64_t t = tile * q.R + slot;
    const bool valid = t < q.T;
    const bool live = valid && masked[t] != 0;
    float acc = 0.f;
    if (live) {
      const T *row = H + t * q.D;
      for (int p = g; p < q.P; p += q.G) {
        float xv[NP], wv[NP];
        load_x<T, NP>(row, p, xv);
        load_w<NP>(w + (int64_t)p * NP, wv);
#pragma unroll
        for (int j = 0; j < NP; ++j) acc = fmaf(xv[j], wv[j], acc);
      }
    }
    acc = group_sum(acc, q.G);                    // outside every divergent branch
    if (valid && g == 0) {
      float r = 0.f;
      if (live) {
        r = (acc + bias) - target[t];
        sq += __double2ll_rn((double)r * (double)r * (double)(1ull << AMPCONV_MFM_LOSS_SHIFT));
        cnt += 1;
      }
      resid[t] = r;
    }
  }
  sq = wave_sum_i64(sq);
  cnt = wave_sum_i64(cnt);
  if ((threadIdx.x & 63) == 0 && cnt != 0) {
    atomicAdd(state, (u64)sq);
    atomicAdd(state + 1, (u64)cnt);
  }
}

// the call's sums -> the running buffer and the fp32 loss
__global__ void mfm_loss_finish_kernel(const long long *__restrict__ state, long long *__restrict__ sums,
                                       float *__restrict__ loss) {
  const int i = threadIdx.x;
  if (sums && i < 2) sums[i] += state[i];
  if (i == 0) {
    const long long n = state[1] > 1 ? state[1] : 1;
    *loss = (float)((double)state[0] / (double)(1ull << AMPCONV_MFM_LOSS_SHIFT) / (double)n);
  }
}

// ---- sums over the masked tokens: loss backward (LOSS) and the mask token's gradient -------------------------------------
// LOSS:  coef[t] = c resid[t]; dX[t, :] = coef w (first pass, every token: zeros for the others); the workgroup's row is
//        [sum coef X[t, :], sum coef] (D + 1 floats).
// !LOSS: coef = 1 (fmaf(1, x, acc) is the plain sum); the row is the sum of X[t, c0 : c0 + P NP] (P NP floats).
template <typename T, int NP, bool LOSS>
__global__ __launch_bounds__(kThreads) void mfm_colsum_kernel(const T *__restrict__ X, const uint8_t *__restrict__ masked,
                                                              const float *__restrict__ resid,
                                                              const float *__restrict__ w,
                                                              const long long *__restrict__ state,
                                                              const float *__restrict__ gscale, Geom q, T *__restrict__ dX,
                                                              float *__restrict__ partial) {
  __shared__ float red[kThreads * kMaxNP + kThreads / 4];
  const int g = threadIdx.x & (q.G - 1), slot = threadIdx.x / q.G;
  const int width = q.P * NP;                     // columns that are summed
  const int per = LOSS ? q.D + 1 : width;
  float *redb = red + kThreads * NP;
  float c = 1.f;
  if constexpr (LOSS) {
    const long long n = state[1] > 1 ? state[1] : 1;
    c = 2.f * *gscale / (float)n;
  }
  float *mine = partial + (int64_t)blockIdx.x * per;
  for (int p0 = 0; p0 < q.P; p0 += q.G) {
    const bool first = p0 == 0;
    const int p = p0 + g;
    float acc[NP], accb = 0.f;
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = 0.f;
    for (int64_t tile = blockIdx.x; tile < q.tiles; tile += gridDim.x) {
      const int64_t t = tile * q.R + slot;
      const bool valid = t < q.T;
      const bool live = valid && masked[t] != 0;
      float coef = 1.f;
      if constexpr (LOSS) {
        coef = live ? c * resid[t] : 0.f;
        if (first && valid && dX) {
          T *drow = dX + t * q.D;
          for (int pp = g; pp < q.P; pp += q.G) {
            Vec<T, NP> v;
            if (live) {
              float wv[NP];
              load_w<NP>(w + (int64_t)pp * NP, wv);
#pragma unroll
              for (int j = 0; j < NP; ++j) v.e[j] = (T)(coef * wv[j]);
            } else {
#pragma unroll
              for (int j = 0; j < NP; ++j) v.e[j] = (T)0.f;
            }
            *reinterpret_cast<Vec<T, NP> *>(drow + (int64_t)pp * NP) = v;
          }
        }
        if (live && first && g == 0) accb += coef;
      }
      if (live && p < q.P) {
        float xv[NP];
        load_x<T, NP>(X + t * q.D + q.c0, p, xv);
#pragma unroll
        for (int j = 0; j < NP; ++j) acc[j] = fmaf(coef, xv[j], acc[j]);
      }
    }
    // the slots of the workgroup, added in slot order
#pragma unroll
    for (int j = 0; j < NP; ++j) red[(slot * q.G + g) * NP + j] = acc[j];
    if (LOSS && first && g == 0) redb[slot] = accb;
    __syncthreads();
    for (int e = threadIdx.x; e < q.G * NP; e += kThreads) {
      float s = 0.f;
      for (int r = 0; r < q.R; ++r) s += red[r * q.G * NP + e];
      if (p0 + e / NP < q.P) mine[p0 * NP + e] = s;
    }
    if (LOSS && first && threadIdx.x == 0) {
      float s = 0.f;
      for (int r = 0; r < q.R; ++r) s += redb[r];
      mine[q.D] = s;
    }
    __syncthreads();
  }
}

// out_a[e] (e < na) / out_b[e - na]: 0 for e < zero_below, else the workgroups' rows added in workgroup order (four
// independent loads in flight); row element e - zero_below.  blocks == 0 writes zeros.
__global__ __launch_bounds__(kThreads) void mfm_fold_kernel(const float *__restrict__ partial, int blocks, int per, int n,
                                                            int zero_below, float *__restrict__ out_a, int na,
                                                            float *__restrict__ out_b) {
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  if (e >= zero_below) {
    const float *col = partial + (e - zero_below);
    int i = 0;
    for (; i + 4 <= blocks; i += 4) {
      const float v0 = col[(int64_t)i * per], v1 = col[(int64_t)(i + 1) * per], v2 = col[(int64_t)(i + 2) * per],
                  v3 = col[(int64_t)(i + 3) * per];
      s = (((s + v0) + v1) + v2) + v3;
    }
    for (; i < blocks; ++i) s += col[(int64_t)i * per];
  }
  if (e < na) out_a[e] = s;
  else out_b[e - na] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------
inline unsigned misalign(const void *p) { return (unsigned)((uintptr_t)p & 15); }

inline bool dims_ok(int64_t N, int L, int D) {
  return N >= 0 && L >= 1 && D >= 1 && (N == 0 || (N <= INT64_MAX / L && N * L <= INT64_MAX / D));
}
inline bool dtype_ok(int dtype) { return dtype == AMPCONV_F32 || dtype == AMPCONV_BF16; }

inline Geom make_geom(int64_t T, int D, int c0, int width, int NP) {
  Geom q{};
  q.T = T, q.D = D, q.c0 = c0;
  q.P = width / NP;
  int G = 4;
  while (G < q.P && G < 64) G <<= 1;
  q.G = G, q.R = kThreads / G;
  q.tiles = (T + q.R - 1) / q.R;
  return q;
}
inline unsigned grid_of(const Geom &q) { return (unsigned)(q.tiles < kMaxBlocks ? q.tiles : kMaxBlocks); }
inline int64_t blocks_bound(int64_t T) {          // R >= 4 tokens per tile whatever the path
  const int64_t t = (T + 3) / 4;
  return t < kMaxBlocks ? t : kMaxBlocks;
}

// f(T{}, integral_constant<int, NP>{}) for the storage and the piece of a call.  bad: the OR of the low four address bits
// of every streamed tensor; force_scalar: w is not 16-byte aligned (its pieces are read as float4), or one column is read
template <typename F>
int dispatch(int dtype, int D, unsigned bad, bool force_scalar, const F &f) {
  if (dtype == AMPCONV_BF16) {
    if (!force_scalar && bad == 0 && D % 8 == 0) return f(__bf16{}, std::integral_constant<int, 8>{});
    if (!force_scalar && (bad & 7) == 0 && D % 4 == 0) return f(__bf16{}, std::integral_constant<int, 4>{});
    return f(__bf16{}, std::integral_constant<int, 1>{});
  }
  if (!force_scalar && bad == 0 && D % 4 == 0) return f(float{}, std::integral_constant<int, 4>{});
  return f(float{}, std::integral_constant<int, 1>{});
}

int fold(const float *ws, int blocks, int per, int n, int zero_below, float *out_a, int na, float *out_b, hipStream_t s) {
  mfm_fold_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(ws, blocks, per, n, zero_below, out_a, na,
                                                                                out_b);
  return ampconv_launch_status();
}

}  // namespace

extern "C" size_t ampconv_mfm_workspace_bytes(int64_t N, int L, int D) {
  if (N <= 0 || !dims_ok(N, L, D)) return 0;
  return (size_t)blocks_bound(N * L) * (size_t)(D + 1) * sizeof(float);
}

extern "C" int ampconv_mfm_build(const float *x, const float *mean, const float *inv_std, const int32_t *idx,
                                 const float *table, int64_t N, int F, int L, int De, const float *mask_token,
                                 uint64_t seed, uint32_t threshold, int mode, const uint8_t *masked_in, void *out,
                                 uint8_t *masked, float *target, int dtype, void *stream) {
  if (De < 0 || De == INT32_MAX || F < 1 || !dims_ok(N, L, De + 1) || (N > 0 && N > INT64_MAX / F)) return AMPCONV_E_BADARG;
  if (threshold > 65536u || (mode != AMPCONV_MFM_TOKEN && mode != AMPCONV_MFM_VALUE)) return AMPCONV_E_BADARG;
  if (!dtype_ok(dtype)) return AMPCONV_E_DTYPE;
  if (N == 0) return AMPCONV_OK;
  if (!x || !mean || !inv_std || !idx || !mask_token || !out || !masked || !target || (De > 0 && !table))
    return AMPCONV_E_BADARG;
  const Geom q = make_geom(N * L, De + 1, 0, De + 1, 1);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == AMPCONV_BF16)
    mfm_build_kernel<<<grid_of(q), kThreads, 0, s>>>(x, mean, inv_std, idx, table, mask_token, q, F, L, seed, threshold,
                                                     mode, masked_in, (__bf16 *)out, masked, target);
  else
    mfm_build_kernel<<<grid_of(q), kThreads, 0, s>>>(x, mean, inv_std, idx, table, mask_token, q, F, L, seed, threshold,
                                                     mode, masked_in, (float *)out, masked, target);
  return ampconv_launch_status();
}

extern "C" int ampconv_mfm_token_grad(const void *dout, const uint8_t *masked, int64_t N, int L, int De, int mode,
                                      float *dmask_token, void *workspace, size_t workspace_bytes, int dtype,
                                      void *stream) {
  if (De < 0 || De == INT32_MAX || !dims_ok(N, L, De + 1)) return AMPCONV_E_BADARG;
  if (mode != AMPCONV_MFM_TOKEN && mode != AMPCONV_MFM_VALUE) return AMPCONV_E_BADARG;
  if (!dtype_ok(dtype)) return AMPCONV_E_DTYPE;
  if (!dmask_token) return AMPCONV_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int D = De + 1;
  if (N == 0) return fold(nullptr, 0, 1, D, 0, dmask_token, D, nullptr, s);
  if (!dout || !masked) return AMPCONV_E_BADARG;
  if (!workspace || workspace_bytes < ampconv_mfm_workspace_bytes(N, L, D)) return AMPCONV_E_WORKSPACE;
  const bool value = mode == AMPCONV_MFM_VALUE;     // one column, element-wise
  const int c0 = value ? De : 0, width = value ? 1 : D;
  return dispatch(dtype, D, misalign(dout), value, [&](auto t, auto np) -> int {
    using T = decltype(t);
    constexpr int NP = decltype(np)::value;
    const Geom q = make_geom(N * L, D, c0, width, NP);
    mfm_colsum_kernel<T, NP, false><<<grid_of(q), kThreads, 0, s>>>((const T *)dout, masked, nullptr, nullptr, nullptr,
                                                                    nullptr, q, nullptr, (float *)workspace);
    if (int rc = ampconv_launch_status()) return rc;
    return fold((const float *)workspace, (int)grid_of(q), width, D, c0, dmask_token, D, nullptr, s);
  });
}

extern "C" int ampconv_mfm_loss_fwd(const void *h, const uint8_t *masked, const float *target, const float *w,
                                    const float *b, int64_t N, int L, int D, float *resid, int64_t *sums, int64_t *state,
                                    float *loss, int dtype, void *stream) {
  if (!dims_ok(N, L, D)) return AMPCONV_E_BADARG;
  if (!dtype_ok(dtype)) return AMPCONV_E_DTYPE;
  if (!state || !loss || (N > 0 && (!h || !masked || !target || !w || !b || !resid))) return AMPCONV_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (hipError_t e = hipMemsetAsync(state, 0, 2 * sizeof(int64_t), s); e != hipSuccess) return (int)e;
  if (N > 0) {
    const int rc = dispatch(dtype, D, misalign(h), misalign(w) != 0, [&](auto t, auto np) -> int {
      using T = decltype(t);
      constexpr int NP = decltype(np)::value;
      const Geom q = make_geom(N * L, D, 0, D, NP);
      mfm_loss_fwd_kernel<T, NP><<<grid_of(q), kThreads, 0, s>>>((const T *)h, masked, target, w, b, q, resid,
                                                                 (u64 *)state);
      return ampconv_launch_status();
    });
    if (rc) return rc;
  }
  mfm_loss_finish_kernel<<<1, 64, 0, s>>>((const long long *)state, (long long *)sums, loss);
  return ampconv_launch_status();
}

extern "C" int ampconv_mfm_loss_bwd(const void *h, const uint8_t *masked, const float *resid, const float *w,
                                    const int64_t *state, const float *g, int64_t N, int L, int D, void *dh, float *dw,
                                    float *db, void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  if (!dims_ok(N, L, D)) return AMPCONV_E_BADARG;
  if (!dtype_ok(dtype)) return AMPCONV_E_DTYPE;
  if (!dw || !db) return AMPCONV_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) return fold(nullptr, 0, 1, D + 1, 0, dw, D, db, s);
  if (!h || !masked || !resid || !w || !state || !g) return AMPCONV_E_BADARG;
  if (!workspace || workspace_bytes < ampconv_mfm_workspace_bytes(N, L, D)) return AMPCONV_E_WORKSPACE;
  const unsigned bad = misalign(h) | (dh ? misalign(dh) : 0u);
  return dispatch(dtype, D, bad, misalign(w) != 0, [&](auto t, auto np) -> int {
    using T = decltype(t);
    constexpr int NP = decltype(np)::value;
    const Geom q = make_geom(N * L, D, 0, D, NP);
    mfm_colsum_kernel<T, NP, true><<<grid_of(q), kThreads, 0, s>>>((const T *)h, masked, resid, w,
                                                                   (const long long *)state, g, q, (T *)dh,
                                                                   (float *)workspace);
    if (int rc = ampconv_launch_status()) return rc;
    return fold((const float *)workspace, (int)grid_of(q), D + 1, D + 1, 0, dw, D, db, s);
  });
}
