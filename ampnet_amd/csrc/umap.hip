// UMAP of node embeddings and features (include/ampconv.h, "UMAP"): the smooth-kNN calibration with the memberships and
// one synchronous epoch of the layout optimiser.  The neighbour search (ampnet_amd.tsne.nearest), the fuzzy union (a
// library sort), the curve fit and the schedule are the Python side's (ampnet_amd/umap.py).
//
// Memberships.  One wave per row as tsne_affinity_kernel: lane l holds the distances l, l + 64, l + 128, l + 192
// (k <= 256) in fp64 registers, the search for sigma is the header's statement by statement, its sum a butterfly (every
// lane ends with the same bits, so the branch is wave-uniform).  The mean of all M k distances that floors sigma where
// rho = 0 comes from two launches in front: the rows' fp64 sums (the same butterfly), then one workgroup over them.
//
// Epoch.  Gather only: row j walks its own CSR row and nothing is scattered (the mirrored entry of the symmetric graph
// has the same firing history and, with positions frozen for the epoch, the same move: include/ampconv.h).  The walk
// is layout_common.h's grouped gather with its long-row scheme; what is this file's is the entry (UmapEntry): its
// attraction, then its negative samples, added in that order in fp32, and its schedule state, which is read and written
// by exactly one lane of one launch.
#include "layout_common.h"

#include <cmath>

namespace {

constexpr int kMaxK = AMPCONV_UMAP_MAX_K;
static_assert(kMaxK == 256 && AMPCONV_UMAP_PART % kGroup == 0 && kGroup == AMPCONV_WAVE, "lane maps of this file");

// ----------------------------------------------------------------------------------------------------- memberships
__global__ __launch_bounds__(256) void umap_rowsum_kernel(const float *__restrict__ dist, int64_t M, int K, int64_t ldd,
                                                          double *__restrict__ rowsum) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                              // wave-uniform
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (lane + 64 * t < K) s += (double)dist[row * ldd + lane + 64 * t];
  s = wave_sum_f64(s);
  if (lane == 0) rowsum[row] = s;
}

__global__ __launch_bounds__(256) void umap_membership_kernel(const int64_t *__restrict__ idx, int64_t ldi,
                                                              const float *__restrict__ dist, int64_t ldd, int64_t M, int K,
                                                              double target, const double *__restrict__ total,
                                                              float *__restrict__ memb, double *__restrict__ sigma_out,
                                                              double *__restrict__ rho_out) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;                                              // wave-uniform
  double d[4];
  bool on[4];
  double sum = 0.0, lowest = INFINITY;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    on[t] = lane + 64 * t < K;
    d[t] = on[t] ? (double)dist[row * ldd + lane + 64 * t] : 0.0;
    sum += d[t];
    if (on[t] && d[t] > 0.0) lowest = fmin(lowest, d[t]);
  }
  sum = wave_sum_f64(sum);
  lowest = wave_min_f64(lowest);
  const double rho = lowest == INFINITY ? 0.0 : lowest;
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int round = 0; round < 64; ++round) {
    double ps = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (on[t] && lane + 64 * t >= 1) {                             // column 0, the sample itself, takes no part
        const double x = d[t] - rho;
        ps += x > 0.0 ? exp(-(x / mid)) : 1.0;
      }
    ps = wave_sum_f64(ps);
    if (fabs(ps - target) < 1e-5) break;
    if (ps > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  const double mean = rho > 0.0 ? sum / (double)K : *total / ((double)M * (double)K);
  const double sigma = fmax(mid, 1e-3 * mean);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (on[t]) {
      const double x = d[t] - rho;
      double v = (x <= 0.0 || sigma == 0.0) ? 1.0 : exp(-(x / sigma));
      if (idx[row * ldi + lane + 64 * t] == row) v = 0.0;
      memb[row * K + lane + 64 * t] = (float)v;
    }
  if (lane == 0) {
    sigma_out[row] = sigma;
    rho_out[row] = rho;
  }
}

// ----------------------------------------------------------------------------------------------------------- epoch
// the two coefficients of the header: d2^b = exp2(b log2(d2)) in fp32, one division each
__device__ __forceinline__ float attract_coeff(float d2, float a, float b) {
  if (!(d2 > 0.f)) return 0.f;
  const float pw = exp2f(b * log2f(d2));
  return (-2.f * a * b * pw) / (d2 * fmaf(a, pw, 1.f));
}
__device__ __forceinline__ float repel_coeff(float d2, float a, float b, float gamma) {
  if (!(d2 > 0.f)) return 0.f;
  const float pw = exp2f(b * log2f(d2));
  return (2.f * gamma * b) / ((0.001f + d2) * fmaf(a, pw, 1.f));
}
__device__ __forceinline__ float clip4(float x) { return fminf(fmaxf(x, -4.f), 4.f); }
// a value the compiler has to materialise: keeps a product out of an FMA with the addition that follows it (the
// schedule state is held to the model bit for bit, and the model rounds the product)
__device__ __forceinline__ float rounded(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

__global__ __launch_bounds__(256) void umap_coeff_kernel(const float *__restrict__ d2, int64_t n, float a, float b, float gamma,
                                                         float *__restrict__ att, float *__restrict__ rep) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  att[i] = attract_coeff(d2[i], a, b);
  rep[i] = repel_coeff(d2[i], a, b, gamma);
}

struct EpochArgs {
  const float *y;
  float *y_out;
  CsrRows rows;
  int dim;
  const float *eps;
  float *next, *nextneg;
  int32_t *drawn;
  float a, b, gamma, alpha, n;
  uint64_t seed;
  int64_t part;
  float *groups;                     // [nnz / 64 + M + 1][dim]: the group sums of the rows longer than a part
};

// entry e of the row at yi: what it adds to the row this epoch (s += ...), and its schedule state moved on
struct UmapEntry {
  const EpochArgs &A;

  template <int D>
  __device__ __forceinline__ void operator()(const float (&yi)[D], int64_t e, float (&s)[D]) const {
    const float eps = A.eps[e], nx = A.next[e];
    if (!(nx <= A.n)) return;
    float yo[D], d[D];
    load_point<D>(A.y, A.dim, A.rows.col(e), yo);
    const float ca = attract_coeff(difference<D>(yi, yo, d), A.a, A.b);
#pragma unroll
    for (int c = 0; c < D; ++c) s[c] = fmaf(2.f * clip4(ca * d[c]), A.alpha, s[c]);
    A.next[e] = nx + eps;
    const float epn = eps / 5.f, nn = A.nextneg[e];
    int m = (int)((A.n - nn) / epn);
    m = m < 0 ? 0 : (m > AMPCONV_UMAP_MAX_NEGATIVES ? AMPCONV_UMAP_MAX_NEGATIVES : m);
    const int32_t dr = A.drawn[e];
    for (int p = 0; p < m; ++p) {
      const uint64_t r = draw(A.seed, (uint64_t)e, (uint64_t)(int64_t)(dr + p));
      load_point<D>(A.y, A.dim, (int64_t)(r % (uint64_t)A.rows.N), yo);
      const float cr = repel_coeff(difference<D>(yi, yo, d), A.a, A.b, A.gamma);
#pragma unroll
      for (int c = 0; c < D; ++c) s[c] = fmaf(clip4(cr * d[c]), A.alpha, s[c]);
    }
    A.drawn[e] = dr + m;
    A.nextneg[e] = nn + rounded((float)m * epn);
  }
};

template <int D>
__global__ __launch_bounds__(256) void umap_parts_kernel(const EpochArgs A) {
  gather_parts<D>(A.rows, A.y, A.dim, A.part, A.groups, UmapEntry{A});
}

template <int D>
__global__ __launch_bounds__(256) void umap_epoch_kernel(const EpochArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= A.rows.N) return;                                         // wave-uniform
  const double acc = gather_row<D>(A.rows, A.y, A.dim, A.part, A.groups, i, lane, UmapEntry{A});   // lane c: coordinate c
  if (lane < A.dim) A.y_out[i * A.dim + lane] = (float)((double)A.y[i * A.dim + lane] + acc);
}

template <int D>
int launch_epoch(const EpochArgs &A, hipStream_t stream) {
  if (A.rows.nnz > A.part) {                                         // no row is longer than a part otherwise
    const int64_t windows = window_count(A.rows.nnz, A.part);
    umap_parts_kernel<D><<<dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, stream>>>(A);
    if (int rc = ampconv_launch_status()) return rc;
  }
  umap_epoch_kernel<D><<<dim3((unsigned)((A.rows.N + 3) / 4)), dim3(256), 0, stream>>>(A);
  return ampconv_launch_status();
}

}  // namespace

extern "C" size_t ampconv_umap_memberships_workspace_bytes(int64_t M) {
  if (M < 2 || M > AMPCONV_UMAP_MAX_M) return 0;
  return pad256((size_t)(M + 1) * sizeof(double));
}

extern "C" int ampconv_umap_memberships(const int64_t *idx, int64_t ldi, const float *dist, int64_t ldd, int64_t M, int k,
                                        float *memb, double *sigma, double *rho, void *workspace, size_t workspace_bytes,
                                        void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(idx) || !aligned4(dist) || !aligned4(memb) || !aligned8(sigma) || !aligned8(rho) || M < 2 ||
      M > AMPCONV_UMAP_MAX_M || k < 2 || k > kMaxK || k > M || ldi < k || ldd < k)
    return AMPCONV_E_BADARG;
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < ampconv_umap_memberships_workspace_bytes(M))
    return AMPCONV_E_WORKSPACE;
  double *rowsum = (double *)workspace, *total = rowsum + M;
  const dim3 grid((unsigned)((M + 3) / 4));
  umap_rowsum_kernel<<<grid, dim3(256), 0, stream>>>(dist, M, k, ldd, rowsum);
  if (int rc = ampconv_launch_status()) return rc;
  sum_rows_kernel<<<dim3(1), dim3(256), 0, stream>>>(rowsum, M, total);
  if (int rc = ampconv_launch_status()) return rc;
  umap_membership_kernel<<<grid, dim3(256), 0, stream>>>(idx, ldi, dist, ldd, M, k, std::log2((double)k), total, memb, sigma, rho);
  return ampconv_launch_status();
}

extern "C" int ampconv_umap_coefficients(const float *d2, int64_t n, float a, float b, float gamma, float *attract,
                                         float *repel, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned4(d2) || !aligned4(attract) || !aligned4(repel) || n < 1 || n > ((int64_t)1 << 31)) return AMPCONV_E_BADARG;
  umap_coeff_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(d2, n, a, b, gamma, attract, repel);
  return ampconv_launch_status();
}

extern "C" size_t ampconv_umap_epoch_workspace_bytes(int64_t M, int64_t nnz, int dim) {
  if (M < 1 || M > AMPCONV_UMAP_MAX_M || nnz < 0 || dim < 2 || dim > AMPCONV_UMAP_MAX_DIM) return 0;
  return groups_bytes(M, nnz, dim);
}

extern "C" int ampconv_umap_epoch_split(const float *y_in, float *y_out, int64_t M, int dim, const int64_t *indptr,
                                        const int64_t *indices, int64_t nnz, const float *eps, float *next, float *nextneg,
                                        int32_t *drawn, float a, float b, float gamma, float alpha, int epoch, uint64_t seed,
                                        int part, void *workspace, size_t workspace_bytes, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!aligned8(y_in) || !aligned8(y_out) || y_in == y_out || !aligned8(indptr) || M < 1 || M > AMPCONV_UMAP_MAX_M ||
      dim < 2 || dim > AMPCONV_UMAP_MAX_DIM || nnz < 0 || epoch < 0 || epoch > (1 << 24) || part < kGroup ||
      part > (1 << 24) || part % kGroup)
    return AMPCONV_E_BADARG;
  if (nnz > 0 && (!aligned8(indices) || !aligned4(eps) || !aligned4(next) || !aligned4(nextneg) || !aligned4(drawn)))
    return AMPCONV_E_BADARG;
  if (!workspace || (uintptr_t)workspace % 8 || workspace_bytes < ampconv_umap_epoch_workspace_bytes(M, nnz, dim))
    return AMPCONV_E_WORKSPACE;
  EpochArgs A = {};
  A.y = y_in; A.y_out = y_out; A.rows = {indptr, indices, M, nnz}; A.dim = dim;
  A.eps = eps; A.next = next; A.nextneg = nextneg; A.drawn = drawn;
  A.a = a; A.b = b; A.gamma = gamma; A.alpha = alpha; A.n = (float)epoch; A.seed = seed;
  A.part = part; A.groups = (float *)workspace;
  if (dim == 2) return launch_epoch<2>(A, stream);
  if (dim <= 4) return launch_epoch<4>(A, stream);
  if (dim <= 8) return launch_epoch<8>(A, stream);
  if (dim <= 16) return launch_epoch<16>(A, stream);
  return launch_epoch<32>(A, stream);
}

extern "C" int ampconv_umap_epoch(const float *y_in, float *y_out, int64_t M, int dim, const int64_t *indptr,
                                  const int64_t *indices, int64_t nnz, const float *eps, float *next, float *nextneg,
                                  int32_t *drawn, float a, float b, float gamma, float alpha, int epoch, uint64_t seed,
                                  void *workspace, size_t workspace_bytes, void *stream_) {
  return ampconv_umap_epoch_split(y_in, y_out, M, dim, indptr, indices, nnz, eps, next, nextneg, drawn, a, b, gamma, alpha,
                                  epoch, seed, AMPCONV_UMAP_PART, workspace, workspace_bytes, stream_);
}
