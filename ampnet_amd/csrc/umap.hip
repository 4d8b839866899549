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
// has the same firing history and, with positions frozen for the epoch, the same move: include/ampconv.h).  One wave
// per row; a row is cut into GROUPS of 64 entries counted from its start, lane l of the wave takes entry l of the group:
// its attraction, then its negative samples, added in that order in fp32; a butterfly adds the lanes; the row's groups
// are added in order in fp64.  A row longer than `part` entries is cut into parts of that length from its start (a
// multiple of 64, so a part is whole groups); umap_parts_kernel walks them -- one wave per window of `part` positions
// of the entry array, tsne_parts_kernel's scheme: at most two parts start in a window -- and stores every GROUP's sum;
// the row's wave then adds the stored groups in the same order.  The part length therefore only decides who computes a
// group, never what is added to what: the bits do not depend on it.  Every entry's schedule state is read and written by
// exactly one lane of one launch.
#include "common.h"

#include <cmath>

namespace {

constexpr int kMaxK = AMPCONV_UMAP_MAX_K;
constexpr int kGroup = 64;
static_assert(kMaxK == 256 && AMPCONV_UMAP_PART % kGroup == 0 && kGroup == AMPCONV_WAVE, "lane maps of this file");

inline size_t pad256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ double wave_min_f64(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o, 64));
  return x;
}

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

// out[0] = the sum of in[0 .. n): lane t adds the elements t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void umap_sum_kernel(const double *__restrict__ in, int64_t n, double *__restrict__ out) {
  __shared__ double s[256];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) v += in[i];
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s[0];
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
  int64_t M, nnz;
  int dim;
  const int64_t *indptr, *indices;
  const float *eps;
  float *next, *nextneg;
  int32_t *drawn;
  float a, b, gamma, alpha, n;
  uint64_t seed;
  int64_t part;
  float *groups;                     // [nnz / 64 + M + 1][dim]: the group sums of the rows longer than a part
};

__device__ __forceinline__ int64_t clamp_pos(int64_t p, int64_t n) { return p < 0 ? 0 : (p > n ? n : p); }

// the largest row r with indptr[r] <= p: the row that holds entry p
__device__ __forceinline__ int64_t row_of(const EpochArgs &A, int64_t p) {
  int64_t lo = 0, hi = A.M - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (A.indptr[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// where the sum of group g of a row that starts at entry `beg` lies: rows r' < r hold at most beg / 64 + r groups
__device__ __forceinline__ int64_t group_slot(int64_t beg, int64_t r, int64_t g) { return beg / kGroup + r + g; }

template <int D>
__device__ __forceinline__ void load_point(const EpochArgs &A, int64_t j, float (&v)[D]) {
  if constexpr (D == 2) {
    const float2 t = reinterpret_cast<const float2 *>(A.y)[j];
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = c < A.dim ? A.y[j * A.dim + c] : 0.f;
  }
}

// d = yi - yo per coordinate; returns |d|^2 by FMAs over the coordinates in order
template <int D>
__device__ __forceinline__ float difference(const float (&yi)[D], const float (&yo)[D], float (&d)[D]) {
  float d2 = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    d[c] = yi[c] - yo[c];
    d2 = fmaf(d[c], d[c], d2);
  }
  return d2;
}

// entry e of the row at yi: what it adds to the row this epoch (s += ...), and its schedule state moved on
template <int D>
__device__ __forceinline__ void entry_terms(const EpochArgs &A, const float (&yi)[D], int64_t e, float (&s)[D]) {
  const float eps = A.eps[e], nx = A.next[e];
  if (!(nx <= A.n)) return;
  float yo[D], d[D];
  int64_t j = A.indices[e];
  j = j < 0 ? 0 : (j >= A.M ? A.M - 1 : j);                          // clamped, never followed out of the array
  load_point<D>(A, j, yo);
  const float ca = attract_coeff(difference<D>(yi, yo, d), A.a, A.b);
#pragma unroll
  for (int c = 0; c < D; ++c) s[c] = fmaf(2.f * clip4(ca * d[c]), A.alpha, s[c]);
  A.next[e] = nx + eps;
  const float epn = eps / 5.f, nn = A.nextneg[e];
  int m = (int)((A.n - nn) / epn);
  m = m < 0 ? 0 : (m > AMPCONV_UMAP_MAX_NEGATIVES ? AMPCONV_UMAP_MAX_NEGATIVES : m);
  const int32_t dr = A.drawn[e];
  for (int p = 0; p < m; ++p) {
    const uint64_t r = splitmix64(A.seed ^ splitmix64((uint64_t)e * 0x100000001B3ull + (uint64_t)(int64_t)(dr + p)));
    load_point<D>(A, (int64_t)(r % (uint64_t)A.M), yo);
    const float cr = repel_coeff(difference<D>(yi, yo, d), A.a, A.b, A.gamma);
#pragma unroll
    for (int c = 0; c < D; ++c) s[c] = fmaf(clip4(cr * d[c]), A.alpha, s[c]);
  }
  A.drawn[e] = dr + m;
  A.nextneg[e] = nn + rounded((float)m * epn);
}

// the group of 64 entries at g0 of a row that ends at `end`: every lane returns the sums
template <int D>
__device__ __forceinline__ void group_sum(const EpochArgs &A, const float (&yi)[D], int64_t g0, int64_t end, int lane,
                                          float (&s)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) s[c] = 0.f;
  if (g0 + lane < end) entry_terms<D>(A, yi, g0 + lane, s);
#pragma unroll
  for (int c = 0; c < D; ++c) s[c] = wave_sum(s[c]);
}

template <int D>
__global__ __launch_bounds__(256) void umap_parts_kernel(const EpochArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t p0 = w * A.part;
  if (p0 >= A.nnz) return;                                           // wave-uniform
  const int64_t pl = min(p0 + A.part, A.nnz) - 1;
  const int64_t ra = row_of(A, p0), rb = row_of(A, pl);
  for (int side = 0; side < 2; ++side) {
    if (side == 1 && rb == ra) break;
    const int64_t r = side ? rb : ra;
    const int64_t beg = clamp_pos(A.indptr[r], A.nnz), end = clamp_pos(A.indptr[r + 1], A.nnz);
    if (end - beg <= A.part) continue;
    int64_t ps = beg;                                                // side 1: the row starts inside the window
    if (side == 0) {
      ps = beg + (p0 - beg + A.part - 1) / A.part * A.part;          // the first part of row ra that starts at or after p0
      if (ps > pl || ps >= end || ps < p0) continue;
    } else if (beg <= p0 || beg > pl) {
      continue;
    }
    float yi[D], s[D];
    load_point<D>(A, r, yi);
    const int64_t pe = min(ps + A.part, end);
    for (int64_t g0 = ps; g0 < pe; g0 += kGroup) {
      group_sum<D>(A, yi, g0, pe, lane, s);
      float *o = A.groups + group_slot(beg, r, (g0 - beg) / kGroup) * A.dim;
#pragma unroll
      for (int c = 0; c < D; ++c)
        if (lane == c && c < A.dim) o[c] = s[c];
    }
  }
}

template <int D>
__global__ __launch_bounds__(256) void umap_epoch_kernel(const EpochArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= A.M) return;                                              // wave-uniform
  const int64_t beg = clamp_pos(A.indptr[i], A.nnz), end = max(beg, clamp_pos(A.indptr[i + 1], A.nnz));
  double acc = 0.0;                                                  // lane c: coordinate c
  if (end - beg <= A.part) {
    float yi[D], s[D];
    load_point<D>(A, i, yi);
    for (int64_t g0 = beg; g0 < end; g0 += kGroup) {
      group_sum<D>(A, yi, g0, end, lane, s);
#pragma unroll
      for (int c = 0; c < D; ++c)
        if (lane == c) acc += (double)s[c];
    }
  } else if (lane < A.dim) {
    const float *o = A.groups + group_slot(beg, i, 0) * A.dim + lane;
    for (int64_t g = 0, n = (end - beg + kGroup - 1) / kGroup; g < n; ++g) acc += (double)o[g * A.dim];
  }
  if (lane < A.dim) A.y_out[i * A.dim + lane] = (float)((double)A.y[i * A.dim + lane] + acc);
}

template <int D>
int launch_epoch(const EpochArgs &A, hipStream_t stream) {
  if (A.nnz > A.part) {                                              // no row is longer than a part otherwise
    const int64_t windows = (A.nnz + A.part - 1) / A.part;
    umap_parts_kernel<D><<<dim3((unsigned)((windows + 3) / 4)), dim3(256), 0, stream>>>(A);
    if (int rc = ampconv_launch_status()) return rc;
  }
  umap_epoch_kernel<D><<<dim3((unsigned)((A.M + 3) / 4)), dim3(256), 0, stream>>>(A);
  return ampconv_launch_status();
}

bool aligned8(const void *p) { return p && (uintptr_t)p % 8 == 0; }
bool aligned4(const void *p) { return p && (uintptr_t)p % 4 == 0; }

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
  umap_sum_kernel<<<dim3(1), dim3(256), 0, stream>>>(rowsum, M, total);
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
  return pad256((size_t)(nnz / kGroup + M + 1) * (size_t)dim * sizeof(float));
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
  A.y = y_in; A.y_out = y_out; A.M = M; A.nnz = nnz; A.dim = dim;
  A.indptr = indptr; A.indices = indices; A.eps = eps; A.next = next; A.nextneg = nextneg; A.drawn = drawn;
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
