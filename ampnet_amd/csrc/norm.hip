// Per-token LayerNorm sites around the AMPConv layers: LayerNorm(D) -> activation -> dropout, and the same followed by
// the token pooling, each as ONE pass over [N, L*D] per direction (include/ampconv.h, "per-token LayerNorm sites").
// Reference: experiments/cora_overfit_one_subgraph.py:46-107
//   :91-94   x = self.conv1(x, edge_index); reshape [N, L, D] -> self.norm1 -> F.relu -> reshape back
//   :103-107 the last layer's output -> mean over the tokens -> Linear -> log_softmax
// A token row is owned by a GROUP of G lanes of one wave: G = the smallest power of two in 4..64 that covers the row's P
// 16-byte pieces, lane j on pieces j, j + G, ... (K = ceil(P / G) <= 4 of them: D <= 1024).  The row is read once and
// stays in registers; lanes behind the row (D = 100 fp32: 25 pieces in a 32-lane group) are masked, not padded.  Both
// row sums of a direction are xor butterflies inside the group.  A group keeps kInFlight 16-byte loads per lane and
// stream in flight: U = kInFlight / K consecutive tokens per step.  Rows that no 16-byte piece divides and unaligned
// bases run the same kernels on one-element pieces, a wave per token.
// dgamma, dbeta: per-lane register sums over the group's tokens, a butterfly over the groups of a wave, the 4 waves of
// a workgroup in wave order through LDS into the workgroup's [2, D] slot, then norm_reduce_slots: no atomics.
// row_shape, tokens_per_step and grid_of are mirrored and pinned by tests/test_gpu_norm_kernels.py.
#include "site_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;                // grid-stride beyond 256 CUs x 8 workgroups; also the number of slots
constexpr int kInFlight = 4;                    // 16-byte loads in flight per lane and input stream
constexpr int kMaxD = AMPCONV_NORM_MAX_D;
constexpr int kScalarK = kMaxD / 64;            // one-element pieces of a 64-lane group
constexpr int kRuns = 16, kCols = 32;           // norm_reduce_slots: runs of slots x columns per workgroup

template <typename T>
struct Elem {                                   // the "piece" of the element-wise path
  static constexpr int N = 1;
  T e[1];
};

struct Mask {
  uint64_t seed;
  uint32_t thr;
  float scale;
};

// bit e = element e of piece q (flat piece index in the logical [N, L*D] tensor) is kept
template <int NP>
__device__ __forceinline__ uint32_t keep_of(const Mask &m, int64_t q) {
  if constexpr (NP == 1) return keep_one(m.seed, m.thr, (uint64_t)q);
  else return keep_bits<NP>(m.seed, m.thr, (uint64_t)q * (NP / 4));
}

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a lane's share of a token row: which pieces, and gamma / beta of their channels
template <typename PT, int K>
struct Lane {
  static constexpr int NP = PT::N;
  int j, G, P;
  float D;
  float g[K][NP], b[K][NP];
  __device__ __forceinline__ Lane(int G_, int P_, int D_, const float *gamma, const float *beta)
      : j(threadIdx.x & (G_ - 1)), G(G_), P(P_), D((float)D_) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < NP; ++e) {
        const bool there = gamma && has(k);
        g[k][e] = there ? gamma[piece(k) * NP + e] : 1.f;
        b[k][e] = there ? beta[piece(k) * NP + e] : 0.f;
      }
  }
  __device__ __forceinline__ int piece(int k) const { return k * G + j; }
  __device__ __forceinline__ bool has(int k) const { return piece(k) < P; }
  __device__ __forceinline__ void load(const PT *row, PT (&r)[K]) const {
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (has(k)) r[k] = row[piece(k)];
  }
  __device__ __forceinline__ void store(PT *row, const float (&v)[K][NP]) const {
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (has(k)) {
        PT o;
#pragma unroll
        for (int e = 0; e < NP; ++e) o.e[e] = (std::remove_all_extents_t<decltype(PT::e)>)v[k][e];
        row[piece(k)] = o;
      }
  }
};

// one token forward: r = the lane's pieces of the row, q0 = flat piece index of the row's piece 0.
// y = keep ? act(z) scale : 0 (zeros on masked lanes); returns (mu, rstd), the same bits on every lane of the group.
template <typename PT, int ACT, int K>
__device__ __forceinline__ float2 token_fwd(const PT (&r)[K], const Lane<PT, K> &ln, float eps, const Mask &m, int64_t q0,
                                            float (&y)[K][PT::N]) {
  constexpr int NP = PT::N;
  float v[K][NP], s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < NP; ++e) s += v[k][e] = ln.has(k) ? (float)r[k].e[e] : 0.f;
  const float mu = group_sum(s, ln.G) / ln.D;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      v[k][e] = ln.has(k) ? v[k][e] - mu : 0.f;
      ss += v[k][e] * v[k][e];
    }
  const float rstd = 1.f / sqrtf(group_sum(ss, ln.G) / ln.D + eps);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t keep = ln.has(k) ? keep_of<NP>(m, q0 + ln.piece(k)) : 0u;
#pragma unroll
    for (int e = 0; e < NP; ++e)
      y[k][e] = (keep >> e) & 1 ? act_value<ACT>(v[k][e] * rstd * ln.g[k][e] + ln.b[k][e]) * m.scale : 0.f;
  }
  return make_float2(mu, rstd);
}

// one token backward: dy = the lane's share of the upstream gradient as floats; adds the token to ag (dgamma), ab (dbeta)
template <typename PT, int ACT, int K>
__device__ __forceinline__ void token_bwd(const PT (&r)[K], const float (&dy)[K][PT::N], const Lane<PT, K> &ln, float2 st,
                                          const Mask &m, int64_t q0, float (&dx)[K][PT::N], float (&ag)[K][PT::N],
                                          float (&ab)[K][PT::N]) {
  constexpr int NP = PT::N;
  float xhat[K][NP], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint32_t keep = ln.has(k) ? keep_of<NP>(m, q0 + ln.piece(k)) : 0u;
#pragma unroll
    for (int e = 0; e < NP; ++e) {
      xhat[k][e] = ln.has(k) ? ((float)r[k].e[e] - st.x) * st.y : 0.f;
      const float z = xhat[k][e] * ln.g[k][e] + ln.b[k][e];
      const float dz = (keep >> e) & 1 ? m.scale * act_slope_of_input<ACT>(z) * dy[k][e] : 0.f;
      ag[k][e] += dz * xhat[k][e];
      ab[k][e] += dz;
      dx[k][e] = dz * ln.g[k][e];                       // dxhat
      s1 += dx[k][e];
      s2 += dx[k][e] * xhat[k][e];
    }
  }
  s1 = group_sum(s1, ln.G) / ln.D;
  s2 = group_sum(s2, ln.G) / ln.D;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < NP; ++e) dx[k][e] = st.y * (dx[k][e] - s1 - xhat[k][e] * s2);
}

// the workgroup's sums over its tokens into its [2, D] slot: groups of a wave by butterfly, waves in wave order
template <typename PT, int K>
__device__ __forceinline__ void write_slot(float (&ag)[K][PT::N], float (&ab)[K][PT::N], const Lane<PT, K> &ln, int D,
                                           float *slot) {
  constexpr int NP = PT::N;
  __shared__ float red[2 * kMaxD];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int e = 0; e < NP; ++e)
      for (int o = ln.G; o < 64; o <<= 1) {
        ag[k][e] += __shfl_xor(ag[k][e], o, 64);
        ab[k][e] += __shfl_xor(ab[k][e], o, 64);
      }
  const int wave = threadIdx.x >> 6;
  for (int w = 0; w < kThreads / 64; ++w) {
    if (wave == w && (threadIdx.x & 63) < ln.G) {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (ln.has(k))
#pragma unroll
          for (int e = 0; e < NP; ++e) {
            const int c = ln.piece(k) * NP + e;
            red[c] = w ? red[c] + ag[k][e] : ag[k][e];
            red[D + c] = w ? red[D + c] + ab[k][e] : ab[k][e];
          }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 2 * D; i += kThreads) slot[i] = red[i];
}

template <int K>
constexpr int tokens_per_step() { return K >= kInFlight ? 1 : kInFlight / K; }

// ---- LayerNorm + activation + dropout ------------------------------------------------------------------------------
// group tb of the grid takes tokens tb U .. tb U + U - 1, then strides by the grid's groups
template <typename PT, int ACT, int K>
__global__ __launch_bounds__(kThreads) void norm_fwd_rows(const PT *__restrict__ X, int64_t T, int P, int D, int G,
                                                          const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float eps, Mask m,
                                                          PT *__restrict__ Y, float2 *__restrict__ stats) {
  constexpr int U = tokens_per_step<K>();
  const Lane<PT, K> ln(G, P, D, gamma, beta);
  const int per_block = kThreads / G;
  const int64_t groups = (int64_t)gridDim.x * per_block;
  for (int64_t tb = (int64_t)blockIdx.x * per_block + threadIdx.x / G; tb * U < T; tb += groups) {
    PT r[U][K];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tb * U + u < T) ln.load(X + (tb * U + u) * P, r[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = tb * U + u;
      if (t < T) {
        float y[K][PT::N];
        const float2 st = token_fwd<PT, ACT, K>(r[u], ln, eps, m, t * P, y);
        ln.store(Y + t * P, y);
        if (ln.j == 0) stats[t] = st;
      }
    }
  }
}

// slots == nullptr: dgamma, dbeta are not wanted
template <typename PT, int ACT, int K>
__global__ __launch_bounds__(kThreads) void norm_bwd_rows(const PT *__restrict__ X, const PT *__restrict__ dY,
                                                          const float2 *__restrict__ stats, int64_t T, int P, int D,
                                                          int G, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, Mask m, PT *__restrict__ dX,
                                                          float *__restrict__ slots) {
  constexpr int U = tokens_per_step<K>(), NP = PT::N;
  const Lane<PT, K> ln(G, P, D, gamma, beta);
  const int per_block = kThreads / G;
  const int64_t groups = (int64_t)gridDim.x * per_block;
  float ag[K][NP] = {}, ab[K][NP] = {};
  for (int64_t tb = (int64_t)blockIdx.x * per_block + threadIdx.x / G; tb * U < T; tb += groups) {
    PT r[U][K], d[U][K];
    float2 st[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (tb * U + u < T) {
        ln.load(X + (tb * U + u) * P, r[u]);
        ln.load(dY + (tb * U + u) * P, d[u]);
        st[u] = stats[tb * U + u];
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t t = tb * U + u;
      if (t < T) {
        float dy[K][NP], dx[K][NP];
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
          for (int e = 0; e < NP; ++e) dy[k][e] = ln.has(k) ? (float)d[u][k].e[e] : 0.f;
        token_bwd<PT, ACT, K>(r[u], dy, ln, st[u], m, t * P, dx, ag, ab);
        ln.store(dX + t * P, dx);
      }
    }
  }
  if (slots) write_slot<PT, K>(ag, ab, ln, D, slots + (int64_t)blockIdx.x * 2 * D);
}

// ---- LayerNorm + activation + dropout + token pooling --------------------------------------------------------------
// a group owns a node and walks its tokens in ascending order, U rows in flight: one fp32 chain per pooled channel.
// `tokens` = L for the token mean, 1 for token-0 pooling (inv = 1 / L resp. 1); stats is [N, tokens].
template <typename PT, int ACT, int K>
__global__ __launch_bounds__(kThreads) void norm_pool_fwd_rows(const PT *__restrict__ X, int64_t N, int L, int tokens,
                                                               float inv, int P, int D, int G,
                                                               const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, float eps, Mask m,
                                                               PT *__restrict__ pooled, float2 *__restrict__ stats) {
  constexpr int U = tokens_per_step<K>(), NP = PT::N;
  const Lane<PT, K> ln(G, P, D, gamma, beta);
  const int per_block = kThreads / G;
  const int64_t groups = (int64_t)gridDim.x * per_block;
  for (int64_t n = (int64_t)blockIdx.x * per_block + threadIdx.x / G; n < N; n += groups) {
    const int64_t q0 = n * L * P;                         // flat piece index of (n, token 0, piece 0)
    float acc[K][NP] = {};
    for (int l0 = 0; l0 < tokens; l0 += U) {
      PT r[U][K];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (l0 + u < tokens) ln.load(X + q0 + (int64_t)(l0 + u) * P, r[u]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (l0 + u < tokens) {
          float y[K][NP];
          const float2 st = token_fwd<PT, ACT, K>(r[u], ln, eps, m, q0 + (int64_t)(l0 + u) * P, y);
          if (ln.j == 0) stats[n * tokens + l0 + u] = st;
#pragma unroll
          for (int k = 0; k < K; ++k)
#pragma unroll
            for (int e = 0; e < NP; ++e) acc[k][e] += y[k][e];
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < NP; ++e) acc[k][e] *= inv;
    ln.store(pooled + n * P, acc);
  }
}

template <typename PT, int ACT, int K>
__global__ __launch_bounds__(kThreads) void norm_pool_bwd_rows(const PT *__restrict__ X, const PT *__restrict__ dpooled,
                                                               const float2 *__restrict__ stats, int64_t N, int L,
                                                               int tokens, float inv, int P, int D, int G,
                                                               const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, Mask m,
                                                               PT *__restrict__ dX, float *__restrict__ slots) {
  constexpr int U = tokens_per_step<K>(), NP = PT::N;
  const Lane<PT, K> ln(G, P, D, gamma, beta);
  const int per_block = kThreads / G;
  const int64_t groups = (int64_t)gridDim.x * per_block;
  float ag[K][NP] = {}, ab[K][NP] = {};
  for (int64_t n = (int64_t)blockIdx.x * per_block + threadIdx.x / G; n < N; n += groups) {
    const int64_t q0 = n * L * P;
    PT gp[K];
    ln.load(dpooled + n * P, gp);
    float dy[K][NP], zero[K][NP] = {};
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int e = 0; e < NP; ++e) dy[k][e] = ln.has(k) ? (float)gp[k].e[e] * inv : 0.f;
    for (int l0 = 0; l0 < tokens; l0 += U) {
      PT r[U][K];
      float2 st[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (l0 + u < tokens) {
          ln.load(X + q0 + (int64_t)(l0 + u) * P, r[u]);
          st[u] = stats[n * tokens + l0 + u];
        }
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (l0 + u < tokens) {
          float dx[K][NP];
          token_bwd<PT, ACT, K>(r[u], dy, ln, st[u], m, q0 + (int64_t)(l0 + u) * P, dx, ag, ab);
          ln.store(dX + q0 + (int64_t)(l0 + u) * P, dx);
        }
    }
    for (int l = tokens; l < L; ++l) ln.store(dX + q0 + (int64_t)l * P, zero);      // token-0 pooling: the rows behind
  }
  if (slots) write_slot<PT, K>(ag, ab, ln, D, slots + (int64_t)blockIdx.x * 2 * D);
}

// dgamma[c] = sum of slot[b][0][c], dbeta[c] = sum of slot[b][1][c] over the `blocks` slots in ascending b: kRuns
// consecutive runs of slots, each an ascending chain, then the run sums in ascending order.  blocks == 0 writes zeros.
__global__ __launch_bounds__(kRuns *kCols) void norm_reduce_slots(const float *__restrict__ slots, int blocks, int D,
                                                                   float *__restrict__ dgamma,
                                                                   float *__restrict__ dbeta) {
  __shared__ float part[kRuns][kCols];
  const int col = threadIdx.x % kCols, run = threadIdx.x / kCols;
  const int i = blockIdx.x * kCols + col;                 // index into [2, D]
  const int per = (blocks + kRuns - 1) / kRuns;
  const int b0 = run * per, b1 = b0 + per < blocks ? b0 + per : blocks;
  float s = 0.f;
  if (i < 2 * D) {
#pragma unroll 8
    for (int b = b0; b < b1; ++b) s += slots[(int64_t)b * 2 * D + i];
  }
  part[run][col] = s;
  __syncthreads();
  if (run == 0 && i < 2 * D) {
    float t = 0.f;
    for (int r = 0; r < kRuns; ++r) t += part[r][col];
    if (i < D) dgamma[i] = t;
    else dbeta[i - D] = t;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
struct RowShape {
  int P, G, K;                                            // pieces per row, lanes per group, pieces per lane
};
// vec: rows of 16-byte pieces; else one-element pieces, a wave per token
inline RowShape row_shape(bool vec, int D, int NP) {
  if (!vec) return {D, 64, kScalarK};
  const int P = D / NP;
  int G = 4;
  while (G < 64 && G < P) G <<= 1;
  return {P, G, (P + G - 1) / G};
}
inline unsigned grid_of(int64_t units, int G) {
  const int64_t b = (units + kThreads / G - 1) / (kThreads / G);
  return (unsigned)(b < kMaxBlocks ? b : kMaxBlocks);
}

// f(piece type, integral_constant<int, K>, RowShape) for the row shape of a call
template <typename T, typename F>
int with_row_shape(bool vec, int D, const F &f) {
  const RowShape rs = row_shape(vec, D, Piece<T>::N);
  if (!vec) return f(Elem<T>{}, std::integral_constant<int, kScalarK>{}, rs);
  if (rs.K == 1) return f(Piece<T>{}, std::integral_constant<int, 1>{}, rs);
  if (rs.K == 2) return f(Piece<T>{}, std::integral_constant<int, 2>{}, rs);
  if constexpr (sizeof(T) == 4) {                         // 1024 bf16 channels are 128 pieces: K <= 2
    if (rs.K == 3) return f(Piece<T>{}, std::integral_constant<int, 3>{}, rs);
    if (rs.K == 4) return f(Piece<T>{}, std::integral_constant<int, 4>{}, rs);
  }
  return AMPCONV_E_BADARG;
}

inline bool norm_args_ok(int64_t T, int D, const float *gamma, const float *beta, uint32_t thr, float scale) {
  return T >= 0 && D >= 1 && D <= kMaxD && T <= INT64_MAX / D && (gamma == nullptr) == (beta == nullptr) &&
         mask_args_ok(thr, scale);
}
inline bool grads_ok(const float *gamma, const float *dgamma, const float *dbeta) {
  return (dgamma == nullptr) == (dbeta == nullptr) && (gamma || !dgamma);
}
inline bool pooling_ok(int pooling) { return pooling == AMPCONV_POOL_MEAN || pooling == AMPCONV_POOL_TOKEN0; }

int reduce_slots(const float *slots, int blocks, int D, float *dgamma, float *dbeta, hipStream_t s) {
  norm_reduce_slots<<<(2 * D + kCols - 1) / kCols, kRuns * kCols, 0, s>>>(slots, blocks, D, dgamma, dbeta);
  return ampconv_launch_status();
}

}  // namespace

extern "C" size_t ampconv_norm_workspace_bytes(int64_t T, int D) {
  if (T <= 0 || D < 1 || D > kMaxD) return 0;
  return (size_t)(T < kMaxBlocks ? T : kMaxBlocks) * 2 * D * sizeof(float);       // a slot per workgroup: <= T of them
}

extern "C" int ampconv_norm_fwd(const void *x, int64_t T, int D, const float *gamma, const float *beta, float eps,
                                int act, uint64_t seed, uint32_t threshold, float scale, void *y, float *stats,
                                int dtype, void *stream) {
  if (!norm_args_ok(T, D, gamma, beta, threshold, scale) || !(eps > 0.f)) return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T_ = decltype(t);
    constexpr int ACT = decltype(a)::value;
    if (T == 0) return AMPCONV_OK;
    if (!x || !y || !stats) return AMPCONV_E_BADARG;
    const bool vec = aligned16(x) && aligned16(y) && D % Piece<T_>::N == 0;
    return with_row_shape<T_>(vec, D, [&](auto piece, auto k, RowShape rs) -> int {
      using PT = decltype(piece);
      constexpr int K = decltype(k)::value;
      const int64_t steps = (T + tokens_per_step<K>() - 1) / tokens_per_step<K>();
      norm_fwd_rows<PT, ACT, K><<<grid_of(steps, rs.G), kThreads, 0, (hipStream_t)stream>>>(
          (const PT *)x, T, rs.P, D, rs.G, gamma, beta, eps, Mask{seed, threshold, scale}, (PT *)y, (float2 *)stats);
      return ampconv_launch_status();
    });
  });
}

extern "C" int ampconv_norm_bwd(const void *x, const void *dy, const float *stats, int64_t T, int D, const float *gamma,
                                const float *beta, int act, uint64_t seed, uint32_t threshold, float scale, void *dx,
                                float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, int dtype,
                                void *stream) {
  if (!norm_args_ok(T, D, gamma, beta, threshold, scale) || !grads_ok(gamma, dgamma, dbeta)) return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T_ = decltype(t);
    constexpr int ACT = decltype(a)::value;
    hipStream_t s = (hipStream_t)stream;
    if (T == 0) return dgamma ? reduce_slots(nullptr, 0, D, dgamma, dbeta, s) : AMPCONV_OK;
    if (!x || !dy || !stats || !dx) return AMPCONV_E_BADARG;
    if (dgamma && (!workspace || workspace_bytes < ampconv_norm_workspace_bytes(T, D))) return AMPCONV_E_WORKSPACE;
    const bool vec = aligned16(x) && aligned16(dy) && aligned16(dx) && D % Piece<T_>::N == 0;
    return with_row_shape<T_>(vec, D, [&](auto piece, auto k, RowShape rs) -> int {
      using PT = decltype(piece);
      constexpr int K = decltype(k)::value;
      const int64_t steps = (T + tokens_per_step<K>() - 1) / tokens_per_step<K>();
      const unsigned blocks = grid_of(steps, rs.G);
      norm_bwd_rows<PT, ACT, K><<<blocks, kThreads, 0, s>>>((const PT *)x, (const PT *)dy, (const float2 *)stats, T, rs.P,
                                                            D, rs.G, gamma, beta, Mask{seed, threshold, scale}, (PT *)dx,
                                                            dgamma ? (float *)workspace : nullptr);
      if (int rc = ampconv_launch_status()) return rc;
      return dgamma ? reduce_slots((const float *)workspace, (int)blocks, D, dgamma, dbeta, s) : AMPCONV_OK;
    });
  });
}

extern "C" int ampconv_norm_pool_fwd(const void *x, int64_t N, int L, int D, const float *gamma, const float *beta,
                                     float eps, int act, int pooling, uint64_t seed, uint32_t threshold, float scale,
                                     void *pooled, float *stats, int dtype, void *stream) {
  if (N < 0 || L < 1 || N > INT64_MAX / L || !norm_args_ok(N * L, D, gamma, beta, threshold, scale) || !(eps > 0.f) ||
      !pooling_ok(pooling))
    return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T_ = decltype(t);
    constexpr int ACT = decltype(a)::value;
    if (N == 0) return AMPCONV_OK;
    if (!x || !pooled || !stats) return AMPCONV_E_BADARG;
    const int tokens = pooling == AMPCONV_POOL_TOKEN0 ? 1 : L;
    const bool vec = aligned16(x) && aligned16(pooled) && D % Piece<T_>::N == 0;
    return with_row_shape<T_>(vec, D, [&](auto piece, auto k, RowShape rs) -> int {
      using PT = decltype(piece);
      constexpr int K = decltype(k)::value;
      norm_pool_fwd_rows<PT, ACT, K><<<grid_of(N, rs.G), kThreads, 0, (hipStream_t)stream>>>(
          (const PT *)x, N, L, tokens, 1.f / (float)tokens, rs.P, D, rs.G, gamma, beta, eps,
          Mask{seed, threshold, scale}, (PT *)pooled, (float2 *)stats);
      return ampconv_launch_status();
    });
  });
}

extern "C" int ampconv_norm_pool_bwd(const void *x, const void *dpooled, const float *stats, int64_t N, int L, int D,
                                     const float *gamma, const float *beta, int act, int pooling, uint64_t seed,
                                     uint32_t threshold, float scale, void *dx, float *dgamma, float *dbeta,
                                     void *workspace, size_t workspace_bytes, int dtype, void *stream) {
  if (N < 0 || L < 1 || N > INT64_MAX / L || !norm_args_ok(N * L, D, gamma, beta, threshold, scale) ||
      !grads_ok(gamma, dgamma, dbeta) || !pooling_ok(pooling))
    return AMPCONV_E_BADARG;
  return with_type_and_act(dtype, act, [&](auto t, auto a) -> int {
    using T_ = decltype(t);
    constexpr int ACT = decltype(a)::value;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) return dgamma ? reduce_slots(nullptr, 0, D, dgamma, dbeta, s) : AMPCONV_OK;
    if (!x || !dpooled || !stats || !dx) return AMPCONV_E_BADARG;
    if (dgamma && (!workspace || workspace_bytes < ampconv_norm_workspace_bytes(N * L, D))) return AMPCONV_E_WORKSPACE;
    const int tokens = pooling == AMPCONV_POOL_TOKEN0 ? 1 : L;
    const bool vec = aligned16(x) && aligned16(dpooled) && aligned16(dx) && D % Piece<T_>::N == 0;
    return with_row_shape<T_>(vec, D, [&](auto piece, auto k, RowShape rs) -> int {
      using PT = decltype(piece);
      constexpr int K = decltype(k)::value;
      const unsigned blocks = grid_of(N, rs.G);
      norm_pool_bwd_rows<PT, ACT, K><<<blocks, kThreads, 0, s>>>(
          (const PT *)x, (const PT *)dpooled, (const float2 *)stats, N, L, tokens, 1.f / (float)tokens, rs.P, D, rs.G,
          gamma, beta, Mask{seed, threshold, scale}, (PT *)dx, dgamma ? (float *)workspace : nullptr);
      if (int rc = ampconv_launch_status()) return rc;
      return dgamma ? reduce_slots((const float *)workspace, (int)blocks, D, dgamma, dbeta, s) : AMPCONV_OK;
    });
  });
}
