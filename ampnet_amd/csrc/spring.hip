// Force-directed graph layout (include/ampconv.h, "Spring layout"): the Fruchterman-Reingold iteration of networkx's
// spring_layout -- the all-pairs repulsion, the attraction over the CSR of the graph, the temperature schedule and the
// stopping rule, with the state of the schedule on the device.  The adjacency (a library sort), the start's extent and
// the final rescaling are the Python side's (ampnet_amd/spring.py).
//
// Repulsion.  The chunked N-body pass of layout_common.h with dim planes.  Per pair and dim = 2: two subtractions, a
// product and an FMA for d^2, a max, v_rcp_f32, two FMAs -- all but the max and the reciprocal packed over two query
// points, five instructions per pair; k^2 is applied by the step after the sums, so the pair carries no other factor.
// j = i needs no compare: its difference is exactly 0 and 0 / 1e-4 adds nothing.
//
// Step.  layout_common.h's grouped gather with its long-row scheme; an entry adds max(|d|, 0.01) w d (SpringEntry).
// The lane-0 tail is the displacement, its length with networkx's floor, the move and the row's share of sum delta^2.
// spring_finish_kernel (one workgroup) adds the rows' shares in a fixed order and moves the state: t, ran, done.  A
// launch sequence entered with done != 0 copies y_in to y_out and leaves everything else as it is.
#include "layout_common.h"

#include <cmath>

namespace {

constexpr int kRun = AMPCONV_SPRING_RUN;
constexpr int kTile = AMPCONV_SPRING_TILE;
constexpr int kChunk0 = AMPCONV_SPRING_CHUNK;
constexpr int kQ = kTile / 256;              // query points per lane
constexpr float kMinDist = 0.01f, kMinDist2 = 1e-4f;     // networkx's clip of the distance, and its square
static_assert(kChunk0 % kRun == 0 && kTile % 512 == 0 && AMPCONV_SPRING_PART % kGroup == 0 && kGroup == AMPCONV_WAVE,
              "lane maps of this file");
static_assert(sizeof(ampconv_spring_state) == 32, "the state is four 8-byte words");

typedef ampconv_spring_state State;

// ----------------------------------------------------------------------------------------------------------- start
__global__ __launch_bounds__(256) void spring_start_kernel(float *__restrict__ y, int64_t N, int dim, uint64_t seed) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= N * dim) return;
  const uint64_t i = (uint64_t)(e / dim), c = (uint64_t)(e % dim);
  const uint64_t r = draw(seed, i, c);
  y[e] = (float)(r >> 40) * 0x1p-24f;                                // 24 bits: exact in fp32, [0, 1)
}

// ------------------------------------------------------------------------------------------------------- repulsion
// Two query points ride in the two halves of a packed fp32 register pair (v_pk_add_f32, v_pk_mul_f32, v_pk_fma_f32); the
// clamp and the reciprocal have no packed form.  p and a are [coordinate][pair of query points].  The values are those
// of the scalar statements of the header: d^2 = fma(d_c, d_c, ...) over the coordinates in order, from d_0 d_0.
typedef float float2v __attribute__((ext_vector_type(2)));

template <int D>
__device__ __forceinline__ void repulsion_run(const float *__restrict__ y, int j0, int j1, const float2v (&p)[D][kQ / 2],
                                              float2v (&a)[D][kQ / 2]) {
#pragma unroll 8
  for (int j = j0; j < j1; ++j) {                                    // j is workgroup-uniform: scalar loads, eight keys each
    float k[D];
    load_point<D>(y, D, j, k);
#pragma unroll
    for (int h = 0; h < kQ / 2; ++h) {
      float2v d[D], d2;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        d[c] = p[c][h] - k[c];
        d2 = c == 0 ? d[c] * d[c] : __builtin_elementwise_fma(d[c], d[c], d2);
      }
      float2v q;
      q.x = __builtin_amdgcn_rcpf(fmaxf(d2.x, kMinDist2));
      q.y = __builtin_amdgcn_rcpf(fmaxf(d2.y, kMinDist2));
#pragma unroll
      for (int c = 0; c < D; ++c) a[c][h] = __builtin_elementwise_fma(q, d[c], a[c][h]);
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void spring_repulsion_kernel(const float *__restrict__ y, int N, int chunk,
                                                               const State *__restrict__ state, double *__restrict__ part) {
  if (state && state->done) return;                                  // grid-uniform
  const int q0 = blockIdx.x * kTile, c = blockIdx.y;
  const int k0 = c * chunk, k1 = min(k0 + chunk, N);
  float2v p[D][kQ / 2];
  int qi[kQ];
  double s[D][kQ];
#pragma unroll
  for (int t = 0; t < kQ; ++t) {
    qi[t] = q0 + 256 * t + (int)threadIdx.x;
    float v[D];
    load_point<D>(y, D, min(qi[t], N - 1), v);
#pragma unroll
    for (int cc = 0; cc < D; ++cc) {
      p[cc][t / 2][t % 2] = v[cc];
      s[cc][t] = 0.0;
    }
  }
  for (int r0 = k0; r0 < k1; r0 += kRun) {
    const int r1 = min(r0 + kRun, k1);
    float2v a[D][kQ / 2];
#pragma unroll
    for (int cc = 0; cc < D; ++cc)
#pragma unroll
      for (int h = 0; h < kQ / 2; ++h) a[cc][h] = 0.f;
    repulsion_run<D>(y, r0, r1, p, a);
#pragma unroll
    for (int cc = 0; cc < D; ++cc)
#pragma unroll
      for (int t = 0; t < kQ; ++t) s[cc][t] += (double)a[cc][t / 2][t % 2];
  }
  double *o = part + (int64_t)c * D * N;
#pragma unroll
  for (int t = 0; t < kQ; ++t)
    if (qi[t] < N) {
#pragma unroll
      for (int cc = 0; cc < D; ++cc) o[(int64_t)cc * N + qi[t]] = s[cc][t];
    }
}

template <int D>
__global__ __launch_bounds__(256) void spring_repulsion_fold_kernel(const double *__restrict__ part, int chunks, int N,
                                                                    const State *__restrict__ state, double *__restrict__ rep) {
  if (state && state->done) return;                                  // grid-uniform
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= N) return;
  double s[D];
  fold_chunks<D>(part, chunks, N, i, s);
#pragma unroll
  for (int c = 0; c < D; ++c) rep[(int64_t)i * D + c] = s[c];
}

template <int D>
int launch_repulsion(const float *y, int64_t N, double *rep, const State *state, void *workspace, hipStream_t stream) {
  const int chunk = nbody_chunk_keys(N, kChunk0), chunks = nbody_chunk_count(N, kChunk0);
  double *part = (double *)workspace;
  spring_repulsion_kernel<D><<<dim3((unsigned)((N + kTile - 1) / kTile), (unsigned)chunks), dim3(256), 0, stream>>>(
      y, (int)N, chunk, state, part);
  if (int rc = ampconv_launch_status()) return rc;
  spring_repulsion_fold_kernel<D><<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream>>>(part, chunks, (int)N, state, rep);
  return ampconv_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ step
struct StepArgs {
  const float *y;
  float *y_out;
  CsrRows rows;
  const float *val;
  const uint8_t *fixed;
  const double *rep;
  double k, threshold;
  State *state;
  int64_t part;
  float *groups;                     // [nnz / 64 + N + 1][dim]: the group sums of the rows longer than a part
  double *rowsq;                     // [N]: the rows' sum of delta^2
};

// entry e of the row at yi: max(|d|, 0.01) w d
struct SpringEntry {
  const StepArgs &A;

  template <int D>
  __device__ __forceinline__ void operator()(const float (&yi)[D], int64_t e, float (&s)[D]) const {
    float yj[D], d[D];
    load_point<D>(A.y, D, A.rows.col(e), yj);
    const float dist = fmaxf(__fsqrt_rn(difference<D>(yi, yj, d)), kMinDist);
    const float w = A.val ? A.val[e] * dist : dist;
#pragma unroll
    for (int c = 0; c < D; ++c) s[c] = fmaf(w, d[c], s[c]);
  }
};

template <int D>
__global__ __launch_bounds__(256) void spring_parts_kernel(const StepArgs A) {
  if (A.state->done) return;                                         // grid-uniform
  gather_parts<D>(A.rows, A.y, D, A.part, A.groups, SpringEntry{A});
}

template <int D>
__global__ __launch_bounds__(256) void spring_step_kernel(const StepArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= A.rows.N) return;                                         // wave-uniform
  float yi[D];
  load_point<D>(A.y, D, i, yi);
  if (A.state->done) {                                               // grid-uniform: the latch
    if (lane < D) A.y_out[i * D + lane] = A.y[i * D + lane];
    return;
  }
  const double acc = gather_row<D>(A.rows, A.y, D, A.part, A.groups, i, lane, SpringEntry{A});    // lane c: coordinate c
  double att[D];
#pragma unroll
  for (int c = 0; c < D; ++c) att[c] = __shfl(acc, c, 64);
  if (lane != 0) return;
  const double t = A.state->t, k2 = A.k * A.k;
  double disp[D], l2 = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    disp[c] = k2 * A.rep[i * D + c] - att[c] / A.k;
    l2 += disp[c] * disp[c];
  }
  double len = sqrt(l2);
  if (len < 0.01) len = 0.1;
  const double scale = t / len;
  const bool still = A.fixed && A.fixed[i];
  double sq = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const float delta = still ? 0.f : (float)(disp[c] * scale);
    A.y_out[i * D + c] = yi[c] + delta;
    sq += (double)delta * (double)delta;
  }
  A.rowsq[i] = sq;
}

// the rows' shares by lane t adding t, t + 256, ... in order, the tree of a 256-lane workgroup, then the state
__global__ __launch_bounds__(256) void spring_finish_kernel(const double *__restrict__ rowsq, int64_t N, double threshold,
                                                            State *state) {
  __shared__ double s[256];
  if (state->done) return;                                           // every lane reads it before lane 0 writes (below the tree)
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) v += rowsq[i];
  v = block_sum_f64(v, s);
  if (threadIdx.x == 0) {
    state->t -= state->dt;
    state->ran += 1;
    state->done = sqrt(v) / (double)N < threshold ? 1 : 0;
  }
}

template <int D>
int launch_step(const StepArgs &A, hipStream_t stream) {
  if (A.rows.nnz > A.part) {                                         // no row is longer than a part otherwise
    const int64_t windows = window_count(A.rows.nnz, A.part);
    spring_parts_kernel<D><<<dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, stream>>>(A);
    if (int rc = ampconv_launch_status()) return rc;
  }
  spring_step_kernel<D><<<dim3((unsigned)((A.rows.N + 3) / 4)), dim3(256), 0, stream>>>(A);
  if (int rc = ampconv_launch_status()) return rc;
  spring_finish_kernel<<<dim3(1), dim3(256), 0, stream>>>(A.rowsq, A.rows.N, A.threshold, A.state);
  return ampconv_launch_status();
}

bool shape_ok(int64_t N, int dim) { return N >= 1 && N <= AMPCONV_SPRING_MAX_N && (dim == 2 || dim == 3); }

}  // namespace

extern "C" int ampconv_spring_start(float *y, int64_t N, int dim, uint64_t seed, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(y) || !shape_ok(N, dim)) return AMPCONV_E_BADARG;
  spring_start_kernel<<<dim3((unsigned)((N * dim + 255) / 256)), dim3(256), 0, stream>>>(y, N, dim, seed);
  return ampconv_launch_status();
}

extern "C" size_t ampconv_spring_repulsion_workspace_bytes(int64_t N, int dim) {
  if (!shape_ok(N, dim)) return 0;
  return pad256((size_t)nbody_chunk_count(N, kChunk0) * (size_t)dim * (size_t)N * sizeof(double));
}

extern "C" int ampconv_spring_repulsion(const float *y, int64_t N, int dim, double *rep, const ampconv_spring_state *state,
                                        void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(y) || !aligned8(rep) || !shape_ok(N, dim) || (state && (uintptr_t)state % 8)) return AMPCONV_E_BADARG;
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < ampconv_spring_repulsion_workspace_bytes(N, dim))
    return AMPCONV_E_WORKSPACE;
  return dim == 2 ? launch_repulsion<2>(y, N, rep, state, workspace, stream) : launch_repulsion<3>(y, N, rep, state, workspace, stream);
}

extern "C" size_t ampconv_spring_step_workspace_bytes(int64_t N, int64_t nnz, int dim) {
  if (!shape_ok(N, dim) || nnz < 0) return 0;
  return groups_bytes(N, nnz, dim) + pad256((size_t)N * sizeof(double));
}

extern "C" int ampconv_spring_step_split(const float *y_in, float *y_out, int64_t N, int dim, const int64_t *indptr,
                                         const int64_t *indices, const float *val, int64_t nnz, const uint8_t *fixed,
                                         const double *rep, double k, double threshold, ampconv_spring_state *state, int part,
                                         void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(y_in) || !aligned8(y_out) || y_in == y_out || !aligned8(indptr) || !aligned8(rep) || !aligned8(state) ||
      !shape_ok(N, dim) || nnz < 0 || !(k > 0.0) || !std::isfinite(k) || part < kGroup || part > (1 << 24) || part % kGroup)
    return AMPCONV_E_BADARG;
  if (nnz > 0 && (!aligned8(indices) || (val && !aligned4(val)))) return AMPCONV_E_BADARG;
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < ampconv_spring_step_workspace_bytes(N, nnz, dim))
    return AMPCONV_E_WORKSPACE;
  StepArgs A = {};
  A.y = y_in; A.y_out = y_out; A.rows = {indptr, indices, N, nnz}; A.val = val; A.fixed = fixed;
  A.rep = rep; A.k = k; A.threshold = threshold; A.state = state; A.part = part;
  A.groups = (float *)workspace;
  A.rowsq = (double *)((char *)workspace + groups_bytes(N, nnz, dim));
  return dim == 2 ? launch_step<2>(A, stream) : launch_step<3>(A, stream);
}

extern "C" int ampconv_spring_step(const float *y_in, float *y_out, int64_t N, int dim, const int64_t *indptr,
                                   const int64_t *indices, const float *val, int64_t nnz, const uint8_t *fixed,
                                   const double *rep, double k, double threshold, ampconv_spring_state *state, void *workspace,
                                   size_t workspace_bytes, void *stream_) {
  return ampconv_spring_step_split(y_in, y_out, N, dim, indptr, indices, val, nnz, fixed, rep, k, threshold, state,
                                   AMPCONV_SPRING_PART, workspace, workspace_bytes, stream_);
}
