// t-SNE of node embeddings and features (include/ampconv.h, "t-SNE"): the perplexity search, the exact repulsive term
// and the gains / momentum step of scikit-learn's TSNE(method='barnes_hut') at angle = 0, two output dimensions.
// The neighbour search (ampnet_amd.knn), the symmetrisation of the affinities (a library sort) and the schedule are
// the Python side's (ampnet_amd/tsne.py).
//
// Affinities.  One wave per row, lane l holds the distances l, l + 64, l + 128, l + 192 (K <= 256) in fp64 registers;
// the search is scikit-learn's _binary_search_perplexity statement by statement in fp64, the two sums per step by a
// butterfly (every lane ends with the same bits, so the branch is wave-uniform).
//
// Repulsion.  The chunked N-body pass of layout_common.h with three planes: x, y and the row's share of Z.  Per pair:
// two subtractions, two FMAs for 1 + d^2, v_rcp_f32, one addition, one product, two FMAs.  j = i is excluded by index, in
// the one chunk that holds the workgroup's own points (a workgroup-uniform choice of loop); everywhere else the loop has
// no compare.  Z: per row in fp64, 256 rows by a fixed tree, the workgroups' sums by one workgroup in a fixed order.
//
// Step.  One wave per row of the CSR of P with layout_common.h's long-row scheme at AMPCONV_TSNE_PART: lane l takes the
// entries l, l + 64, ... of a row or a part in fp32 (part_sum), tsne_parts_kernel stores the sums of the parts that start
// in a window as [2 sides][4], and the row's wave adds its parts in order in fp64.  The lane-0 tail is scikit-learn's
// _gradient_descent for the row's two coordinates.
#include "layout_common.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int kMaxK = AMPCONV_TSNE_MAX_K;
constexpr int kRun = AMPCONV_TSNE_RUN;
constexpr int kTile = AMPCONV_TSNE_TILE;
constexpr int kChunk0 = AMPCONV_TSNE_CHUNK;
constexpr int kPart = AMPCONV_TSNE_PART;
constexpr int kQ = kTile / 256;              // query points per lane
static_assert(kMaxK == 256 && kChunk0 % kRun == 0 && kTile % 256 == 0, "lane maps of this file");

// ------------------------------------------------------------------------------------------------------ affinities
__global__ __launch_bounds__(256) void tsne_affinity_kernel(const float *__restrict__ dist2, int64_t N, int K, int64_t ldd,
                                                            double log_perplexity, float *__restrict__ P,
                                                            double *__restrict__ beta_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;                                              // wave-uniform
  double d[4], p[4];
  bool on[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    on[t] = lane + 64 * t < K;
    d[t] = on[t] ? (double)dist2[row * ldd + lane + 64 * t] : 0.0;
    p[t] = 0.0;
  }
  const double kTol = (double)1e-5f, kEps = (double)1e-8f;           // scikit-learn keeps both as C floats
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, at = 1.0;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      p[t] = on[t] ? exp(-d[t] * beta) : 0.0;
      s += p[t];
    }
    s = wave_sum_f64(s);
    if (s == 0.0) s = kEps;
    double sd = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      p[t] /= s;
      sd += d[t] * p[t];
    }
    sd = wave_sum_f64(sd);
    const double diff = (log(s) + beta * sd) - log_perplexity;
    at = beta;
    if (fabs(diff) <= kTol) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (on[t]) {
      float f = (float)p[t];                                         // positive in fp64 stays positive: a pair of P exists
      if (p[t] > 0.0 && __float_as_uint(f) == 0u) f = __uint_as_float(1u);      // or not by that (include/ampconv.h)
      P[row * K + lane + 64 * t] = f;
    }
  if (lane == 0) beta_out[row] = at;
}

// ------------------------------------------------------------------------------------------------------- repulsion
template <bool SELF>
__device__ __forceinline__ void repulsion_run(const float2 *__restrict__ y, int j0, int j1, const float (&xi)[kQ],
                                              const float (&yi)[kQ], const int (&qi)[kQ], float (&ax)[kQ], float (&ay)[kQ],
                                              float (&aq)[kQ]) {
#pragma unroll 8
  for (int j = j0; j < j1; ++j) {                                    // j is workgroup-uniform: scalar loads, eight keys each
    const float2 k = y[j];
#pragma unroll
    for (int t = 0; t < kQ; ++t) {
      const float dx = xi[t] - k.x, dy = yi[t] - k.y;
      float q = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
      if (SELF && j == qi[t]) q = 0.f;
      aq[t] += q;
      const float q2 = q * q;
      ax[t] = fmaf(q2, dx, ax[t]);
      ay[t] = fmaf(q2, dy, ay[t]);
    }
  }
}

__global__ __launch_bounds__(256) void tsne_repulsion_kernel(const float2 *__restrict__ y, int N, int chunk,
                                                             double *__restrict__ part) {
  const int q0 = blockIdx.x * kTile, c = blockIdx.y;
  const int k0 = c * chunk, k1 = min(k0 + chunk, N);
  float xi[kQ], yi[kQ];
  int qi[kQ];
  double sx[kQ], sy[kQ], sq[kQ];
#pragma unroll
  for (int t = 0; t < kQ; ++t) {
    qi[t] = q0 + 256 * t + (int)threadIdx.x;
    const float2 v = y[min(qi[t], N - 1)];
    xi[t] = v.x; yi[t] = v.y;
    sx[t] = sy[t] = sq[t] = 0.0;
  }
  const bool own = k0 < q0 + kTile && q0 < k1;                       // this chunk holds some of the workgroup's points
  for (int r0 = k0; r0 < k1; r0 += kRun) {
    const int r1 = min(r0 + kRun, k1);
    float ax[kQ], ay[kQ], aq[kQ];
#pragma unroll
    for (int t = 0; t < kQ; ++t) ax[t] = ay[t] = aq[t] = 0.f;
    if (own) repulsion_run<true>(y, r0, r1, xi, yi, qi, ax, ay, aq);
    else repulsion_run<false>(y, r0, r1, xi, yi, qi, ax, ay, aq);
#pragma unroll
    for (int t = 0; t < kQ; ++t) {
      sx[t] += (double)ax[t]; sy[t] += (double)ay[t]; sq[t] += (double)aq[t];
    }
  }
  double *o = part + (int64_t)c * 3 * N;
#pragma unroll
  for (int t = 0; t < kQ; ++t)
    if (qi[t] < N) {
      o[qi[t]] = sx[t];
      o[(int64_t)N + qi[t]] = sy[t];
      o[2 * (int64_t)N + qi[t]] = sq[t];
    }
}

__global__ __launch_bounds__(256) void tsne_repulsion_fold_kernel(const double *__restrict__ part, int chunks, int N,
                                                                  float2 *__restrict__ neg_f, double *__restrict__ zpart) {
  __shared__ double s[256];
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  double f[3] = {0.0, 0.0, 0.0};
  if (i < N) {
    fold_chunks<3>(part, chunks, N, i, f);
    neg_f[i] = make_float2((float)f[0], (float)f[1]);
  }
  const double z = block_sum_f64(f[2], s);
  if (threadIdx.x == 0) zpart[blockIdx.x] = z;
}

// ------------------------------------------------------------------------------------------------------------ step
struct StepArgs {
  const float2 *y;
  float2 *y_out, *update, *gains;
  CsrRows rows;
  const float *val;
  const float2 *neg;
  const double *Z;
  float exag, mom, lr, min_gain;
  int err;
  float *parts;                      // [2 windows][4]: x, y, error of the parts that start in a window
  double *rowerr;                    // [2][N]: the rows' error terms, the rows' squared gradient norms
};

// entries [b, e) of a row at yi, e - b <= AMPCONV_TSNE_PART, by one wave; every lane returns the sums
__device__ __forceinline__ void part_sum(const StepArgs &a, float2 yi, int64_t b, int64_t e, double Z, int lane, float &sx,
                                         float &sy, float &kl) {
  sx = sy = kl = 0.f;
  for (int64_t p = b + lane; p < e; p += 64) {
    const float2 yj = a.y[a.rows.col(p)];
    const float pv = a.exag * a.val[p];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float q = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
    const float w = pv * q;
    sx = fmaf(w, dx, sx);
    sy = fmaf(w, dy, sy);
    if (a.err) {
      const float qn = (float)((double)q / Z);
      kl += pv * logf(fmaxf(pv, FLT_MIN) / fmaxf(qn, FLT_MIN));
    }
  }
  sx = wave_sum(sx); sy = wave_sum(sy); kl = wave_sum(kl);
}

__global__ __launch_bounds__(256) void tsne_parts_kernel(const StepArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const double Z = fmax(*a.Z, DBL_EPSILON);
  for_window_parts(a.rows, kPart, w, [&](int64_t r, int64_t, int64_t, int64_t ps, int64_t pe, int side) {
    float sx, sy, kl;
    part_sum(a, a.y[r], ps, pe, Z, lane, sx, sy, kl);
    if (lane == 0) {
      float *o = a.parts + (2 * w + side) * 4;
      o[0] = sx; o[1] = sy; o[2] = kl;
    }
  });
}

__global__ __launch_bounds__(256) void tsne_step_kernel(const StepArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= a.rows.N) return;                                         // wave-uniform
  int64_t beg, end;
  a.rows.span(i, beg, end);
  const float2 yi = a.y[i];
  const double Z = fmax(*a.Z, DBL_EPSILON);
  double px, py, pk;
  if (end - beg <= kPart) {
    float sx, sy, kl;
    part_sum(a, yi, beg, end, Z, lane, sx, sy, kl);
    px = (double)sx; py = (double)sy; pk = (double)kl;
  } else {
    px = py = pk = 0.0;
    for (int64_t ps = beg; ps < end; ps += kPart) {                  // the row's parts in order, in fp64
      const int64_t w = ps / kPart;
      const float *o = a.parts + (2 * w + (beg <= w * kPart ? 0 : 1)) * 4;
      px += (double)o[0]; py += (double)o[1]; pk += (double)o[2];
    }
  }
  if (lane != 0) return;
  const float2 neg = a.neg[i], up = a.update[i], ga = a.gains[i];
  const float pos[2] = {(float)px, (float)py}, ng[2] = {neg.x, neg.y}, u[2] = {up.x, up.y}, g0[2] = {ga.x, ga.y};
  const float yv[2] = {yi.x, yi.y};
  float un[2], gn[2], yo[2], gg[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float grad = 4.f * (float)((double)pos[c] - (double)ng[c] / Z);
    float gain = u[c] * grad < 0.f ? g0[c] + 0.2f : g0[c] * 0.8f;
    gain = fmaxf(gain, a.min_gain);
    gg[c] = grad * gain;
    const float m = a.mom * u[c], l = a.lr * gg[c];
    un[c] = m - l;
    gn[c] = gain;
    yo[c] = yv[c] + un[c];
  }
  a.gains[i] = make_float2(gn[0], gn[1]);
  a.update[i] = make_float2(un[0], un[1]);
  a.y_out[i] = make_float2(yo[0], yo[1]);
  if (a.err) {
    a.rowerr[i] = pk;
    a.rowerr[a.rows.N + i] = (double)gg[0] * (double)gg[0] + (double)gg[1] * (double)gg[1];
  }
}

int64_t windows(int64_t nnz) { return window_count(nnz, kPart); }

}  // namespace

extern "C" int ampconv_tsne_affinities(const float *dist2, int64_t N, int K, int64_t ldd, float perplexity, float *P,
                                       double *beta, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!dist2 || !P || !beta || N < 1 || N > AMPCONV_TSNE_MAX_N || K < 1 || K > kMaxK || ldd < K || !(perplexity > 0.f))
    return AMPCONV_E_BADARG;
  tsne_affinity_kernel<<<dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream>>>(dist2, N, K, ldd, std::log((double)perplexity),
                                                                                P, beta);
  return ampconv_launch_status();
}

extern "C" size_t ampconv_tsne_repulsion_workspace_bytes(int64_t N) {
  if (N < 1 || N > AMPCONV_TSNE_MAX_N) return 0;
  return pad256((size_t)nbody_chunk_count(N, kChunk0) * 3 * (size_t)N * sizeof(double)) + pad256((size_t)((N + 255) / 256) * sizeof(double));
}

extern "C" int ampconv_tsne_repulsion(const float *y, int64_t N, float *neg_f, double *Z, void *workspace,
                                      size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(y) || !aligned8(neg_f) || !aligned8(Z) || N < 1 || N > AMPCONV_TSNE_MAX_N) return AMPCONV_E_BADARG;
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < ampconv_tsne_repulsion_workspace_bytes(N))
    return AMPCONV_E_WORKSPACE;
  const int chunk = nbody_chunk_keys(N, kChunk0), chunks = nbody_chunk_count(N, kChunk0);
  const int blocks = (int)((N + 255) / 256);
  double *part = (double *)workspace;
  double *zpart = (double *)((char *)workspace + pad256((size_t)chunks * 3 * (size_t)N * sizeof(double)));
  tsne_repulsion_kernel<<<dim3((unsigned)((N + kTile - 1) / kTile), (unsigned)chunks), dim3(256), 0, stream>>>(
      (const float2 *)y, (int)N, chunk, part);
  if (int rc = ampconv_launch_status()) return rc;
  tsne_repulsion_fold_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(part, chunks, (int)N, (float2 *)neg_f, zpart);
  if (int rc = ampconv_launch_status()) return rc;
  sum_rows_kernel<<<dim3(1), dim3(256), 0, stream>>>(zpart, blocks, Z);
  return ampconv_launch_status();
}

extern "C" size_t ampconv_tsne_step_workspace_bytes(int64_t N, int64_t nnz) {
  if (N < 1 || N > AMPCONV_TSNE_MAX_N || nnz < 0) return 0;
  return pad256((size_t)(2 * windows(nnz) * 4 + 4) * sizeof(float)) + pad256((size_t)2 * (size_t)N * sizeof(double));
}

extern "C" int ampconv_tsne_step(const float *y_in, float *y_out, float *update, float *gains, int64_t N,
                                 const int64_t *indptr, const int64_t *indices, const float *val, int64_t nnz,
                                 const float *neg_f, const double *Z, float exaggeration, float momentum,
                                 float learning_rate, float min_gain, double *error, void *workspace,
                                 size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(y_in) || !aligned8(y_out) || !aligned8(update) || !aligned8(gains) || !aligned8(neg_f) || !aligned8(Z) ||
      !aligned8(indptr) || y_in == y_out || N < 1 || N > AMPCONV_TSNE_MAX_N || nnz < 0 || (error && (uintptr_t)error % 8))
    return AMPCONV_E_BADARG;
  if (nnz > 0 && (!aligned8(indices) || !val)) return AMPCONV_E_BADARG;
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < ampconv_tsne_step_workspace_bytes(N, nnz))
    return AMPCONV_E_WORKSPACE;
  StepArgs a = {};
  a.y = (const float2 *)y_in; a.y_out = (float2 *)y_out; a.update = (float2 *)update; a.gains = (float2 *)gains;
  a.rows = {indptr, indices, N, nnz}; a.val = val;
  a.neg = (const float2 *)neg_f; a.Z = Z;
  a.exag = exaggeration; a.mom = momentum; a.lr = learning_rate; a.min_gain = min_gain;
  a.err = error != nullptr;
  a.parts = (float *)workspace;
  a.rowerr = (double *)((char *)workspace + pad256((size_t)(2 * windows(nnz) * 4 + 4) * sizeof(float)));
  if (nnz > kPart) {                                                 // no row is longer than a part otherwise
    tsne_parts_kernel<<<dim3((unsigned)((windows(nnz) + 3) / 4)), dim3(256), 0, stream>>>(a);
    if (int rc = ampconv_launch_status()) return rc;
  }
  tsne_step_kernel<<<dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream>>>(a);
  if (int rc = ampconv_launch_status()) return rc;
  if (error) {
    sum_rows_kernel<<<dim3(2), dim3(256), 0, stream>>>(a.rowerr, N, error);
    return ampconv_launch_status();
  }
  return AMPCONV_OK;
}
