// GCN baseline (the other side of the reference's TRAIN_AMPCONV switch): the normalised neighbourhood sum of a
// GCNConv layer and the first layer's linear map over the embedded input.  Reference: src/ampnet/module/
// gcn_classifier.py:17-109 (two PyG GCNConv layers behind cat(feature_embedding_table, zscore(x)) per node).
// Contract: include/ampconv.h, "GCN baseline".  fp32 throughout, no float atomics: every sum has a fixed order.
#include "common.h"
#include <algorithm>

namespace {

constexpr int kLong = AMPCONV_GCN_LONG_SEGMENT;   // a segment of at least this many entries is a long one
constexpr int kPart = AMPCONV_GCN_PART;           // entries of a long segment that one workgroup sums
constexpr int kSlots = 4;                         // edge slots of a short row's lane group

// ---- dinv[n] = deg[n]^-1/2: one wave per node, an integer count (exact in any order)
__global__ __launch_bounds__(256) void gcn_norm_kernel(const int32_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                       int64_t N, int self, float fill, float *__restrict__ dinv) {
  const int64_t n = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (n >= N) return;                                  // a whole wave at a time
  const int beg = ptr[n], end = ptr[n + 1];
  int cnt = end - beg;
  if (self) {
    cnt = 0;
    for (int p = beg + lane; p < end; p += 64) cnt += idx[p] != (int32_t)n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  }
  const float deg = (float)cnt + (self ? fill : 0.f);
  if (lane == 0) dinv[n] = deg > 0.f ? 1.f / sqrtf(deg) : 0.f;
}

struct AggArgs {
  const float *h;
  int64_t ld_h;
  int C;
  const int32_t *ptr, *idx;
  const float *dinv;
  int self;
  float fill;
  const float *bias;
  float *out;
  int64_t ld_out, N;
  // long segments (nullptr: every segment is walked by its lane group): {rows, parts, -, -}, then max_rows {row, first
  // part}, then max_parts {row, part of the row}, then max_parts partial rows of C floats
  int32_t *hdr;
  int max_rows, max_parts;
};
__device__ __forceinline__ int2 *long_rows(const AggArgs &a) { return reinterpret_cast<int2 *>(a.hdr + 4); }
__device__ __forceinline__ int2 *long_parts(const AggArgs &a) { return long_rows(a) + a.max_rows; }
__device__ __forceinline__ float *long_partials(const AggArgs &a) {
  return reinterpret_cast<float *>(long_parts(a) + a.max_parts);
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float *p, int rem) {
  if (VEC && rem >= 4) return *reinterpret_cast<const float4 *>(p);
  float4 v = {0.f, 0.f, 0.f, 0.f};
  v.x = p[0];
  if (rem > 1) v.y = p[1];
  if (rem > 2) v.z = p[2];
  if (rem > 3) v.w = p[3];
  return v;
}
template <bool VEC>
__device__ __forceinline__ void store4(float *p, const float4 &v, int rem) {
  if (VEC && rem >= 4) {
    *reinterpret_cast<float4 *>(p) = v;
    return;
  }
  p[0] = v.x;
  if (rem > 1) p[1] = v.y;
  if (rem > 2) p[2] = v.z;
  if (rem > 3) p[3] = v.w;
}
__device__ __forceinline__ void fma4(float4 &acc, float w, const float4 &v) {
  acc.x = fmaf(w, v.x, acc.x);
  acc.y = fmaf(w, v.y, acc.y);
  acc.z = fmaf(w, v.z, acc.z);
  acc.w = fmaf(w, v.w, acc.w);
}
__device__ __forceinline__ void add4(float4 &a, const float4 &b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}
__device__ __forceinline__ float4 shfl_xor4(const float4 &v, int o) {
  return float4{__shfl_xor(v.x, o, 64), __shfl_xor(v.y, o, 64), __shfl_xor(v.z, o, 64), __shfl_xor(v.w, o, 64)};
}

// the entries [beg, end) of row n that lane slot s of `slots` owns, in ascending order, into acc (columns c .. c + 3)
template <bool VEC>
__device__ __forceinline__ void walk(const AggArgs &a, int64_t n, int beg, int end, int s, int slots, int c, float4 &acc) {
  for (int p = beg + s; p < end; p += slots) {
    const int j = a.idx[p];
    if (a.self && j == (int32_t)n) continue;
    fma4(acc, a.dinv[j], load4<VEC>(a.h + (int64_t)j * a.ld_h + c, a.C - c));
  }
}

// out[n, c .. c + 3] from the neighbourhood sum
template <bool VEC>
__device__ __forceinline__ void finish(const AggArgs &a, int64_t n, int c, float4 sum) {
  const float dn = a.dinv[n];
  if (a.self) fma4(sum, a.fill * dn, load4<VEC>(a.h + n * a.ld_h + c, a.C - c));
  float4 b = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) b = load4<false>(a.bias + c, a.C - c);
  store4<VEC>(a.out + n * a.ld_out + c, float4{fmaf(dn, sum.x, b.x), fmaf(dn, sum.y, b.y), fmaf(dn, sum.z, b.z),
                                                fmaf(dn, sum.w, b.w)}, a.C - c);
}

// Short rows: a row on kSlots x Q lanes (edge slot x column quad), 64 / (4 Q) rows per wave.  A slot adds its entries in
// ascending order, the slots combine in a fixed xor order.  Long rows are filed for the two kernels below.
template <int Q, bool VEC>
__global__ __launch_bounds__(256) void gcn_aggregate_kernel(AggArgs a) {
  constexpr int G = kSlots * Q;
  const int l = threadIdx.x % G, s = l / Q, q = l % Q;
  const int64_t n = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G;
  const bool row = n < a.N;
  int beg = 0, end = 0;
  if (row) {
    beg = a.ptr[n];
    end = a.ptr[n + 1];
  }
  const bool is_long = a.hdr != nullptr && end - beg >= kLong;
  if (is_long && l == 0) {
    const int np = (end - beg + kPart - 1) / kPart;
    const int r = atomicAdd(a.hdr, 1), fp = atomicAdd(a.hdr + 1, np);        // integer counters: the order of arrival
    if (r < a.max_rows && fp + np <= a.max_parts) {                           // changes no sum
      long_rows(a)[r] = int2{(int)n, fp};
      for (int j = 0; j < np; ++j) long_parts(a)[fp + j] = int2{(int)n, j};
    }
  }
  for (int c0 = 0; c0 < a.C; c0 += 4 * Q) {
    const int c = c0 + 4 * q;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    if (row && !is_long && c < a.C) walk<VEC>(a, n, beg, end, s, kSlots, c, acc);
    add4(acc, shfl_xor4(acc, Q));
    add4(acc, shfl_xor4(acc, 2 * Q));
    if (row && !is_long && c < a.C && s == 0) finish<VEC>(a, n, c, acc);
  }
}

// Long rows, first step: a workgroup per part of kPart entries, 256 / Q slots, ordered LDS combine, one partial row.
template <int Q, bool VEC>
__global__ __launch_bounds__(256) void gcn_long_parts_kernel(AggArgs a) {
  __shared__ float4 red[256];
  constexpr int SL = 256 / Q;
  const int s = threadIdx.x / Q, q = threadIdx.x % Q;
  const int n_parts = min(a.hdr[1], a.max_parts);
  for (int i = blockIdx.x; i < n_parts; i += gridDim.x) {
    const int2 d = long_parts(a)[i];
    const int64_t n = d.x;
    const int beg = a.ptr[n] + d.y * kPart, end = min(a.ptr[n + 1], beg + kPart);
    for (int c0 = 0; c0 < a.C; c0 += 4 * Q) {
      const int c = c0 + 4 * q;
      float4 acc = {0.f, 0.f, 0.f, 0.f};
      if (c < a.C) walk<VEC>(a, n, beg, end, s, SL, c, acc);
      red[threadIdx.x] = acc;
      __syncthreads();
      for (int st = SL / 2; st >= 1; st >>= 1) {
        if (s < st) add4(red[threadIdx.x], red[threadIdx.x + st * Q]);
        __syncthreads();
      }
      if (s == 0 && c < a.C) store4<false>(long_partials(a) + (int64_t)i * a.C + c, red[threadIdx.x], a.C - c);
      __syncthreads();
    }
  }
}

// Long rows, second step: a row's partial rows added in part order, then the same finish as a short row.
__global__ __launch_bounds__(64) void gcn_long_combine_kernel(AggArgs a) {
  const int n_rows = min(a.hdr[0], a.max_rows);
  for (int i = blockIdx.x; i < n_rows; i += gridDim.x) {
    const int2 d = long_rows(a)[i];
    const int64_t n = d.x;
    const int np = (a.ptr[n + 1] - a.ptr[n] + kPart - 1) / kPart;
    for (int c = 4 * threadIdx.x; c < a.C; c += 256) {
      float4 sum = {0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < np; ++j) add4(sum, load4<false>(long_partials(a) + (int64_t)(d.y + j) * a.C + c, a.C - c));
      finish<false>(a, n, c, sum);
    }
  }
}

template <int Q>
int launch_aggregate(const AggArgs &a, bool vec, int64_t part_grid, int64_t row_grid, hipStream_t st) {
  const int64_t rows_per_block = 256 / (kSlots * Q), blocks = (a.N + rows_per_block - 1) / rows_per_block;
  if (blocks > INT32_MAX) return AMPCONV_E_BADARG;
  if (vec) gcn_aggregate_kernel<Q, true><<<(unsigned)blocks, 256, 0, st>>>(a);
  else gcn_aggregate_kernel<Q, false><<<(unsigned)blocks, 256, 0, st>>>(a);
  if (a.hdr) {
    if (vec) gcn_long_parts_kernel<Q, true><<<(unsigned)part_grid, 256, 0, st>>>(a);
    else gcn_long_parts_kernel<Q, false><<<(unsigned)part_grid, 256, 0, st>>>(a);
    gcn_long_combine_kernel<<<(unsigned)row_grid, 64, 0, st>>>(a);
  }
  return ampconv_launch_status();
}

inline int64_t long_max_rows(int64_t E) { return E / kLong; }
inline int64_t long_max_parts(int64_t E) { return E / kPart + E / kLong; }

// ---- deterministic column sum of g [N, C] (row stride ld): chunks of rows in ascending order, then the chunks
constexpr int kColsumChunks = 1024;
inline int colsum_chunks(int64_t N) { return (int)std::min<int64_t>(std::max<int64_t>((N + 31) / 32, 1), kColsumChunks); }

__global__ __launch_bounds__(64) void colsum_partial_kernel(const float *__restrict__ g, int64_t ld, int64_t N, int C,
                                                            float *__restrict__ partial) {
  const int c = blockIdx.y * 64 + threadIdx.x;
  if (c >= C) return;
  const int64_t per = (N + gridDim.x - 1) / gridDim.x, n0 = blockIdx.x * per, n1 = min(N, n0 + per);
  float s = 0.f;
  for (int64_t n = n0; n < n1; ++n) s += g[n * ld + c];
  partial[(int64_t)blockIdx.x * C + c] = s;
}
__global__ __launch_bounds__(64) void colsum_final_kernel(const float *__restrict__ partial, int chunks, int C,
                                                          float *__restrict__ out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int b = 0; b < chunks; ++b) s += partial[(int64_t)b * C + c];
  out[c] = s;
}
int colsum(const float *g, int64_t ld, int64_t N, int C, float *out, float *partial, hipStream_t st) {
  const int chunks = colsum_chunks(N), cb = (C + 63) / 64;
  colsum_partial_kernel<<<dim3(chunks, cb), 64, 0, st>>>(g, ld, N, C, partial);
  colsum_final_kernel<<<cb, 64, 0, st>>>(partial, chunks, C, out);
  return ampconv_launch_status();
}

// ---- the first layer over the embedded input.  W [C, F, De + 1], table [F, De]; z = (x - mean) inv_std.
constexpr int kPrepF = 64;    // features per workgroup of the preparation
// WvT[f, j] = W[j, f, De] (the value column, transposed so that a K chunk is contiguous) and, with a table, the partial
// sums over this workgroup's features of dot(table[f], W[j, f, :De])
__global__ __launch_bounds__(256) void input_prep_kernel(const float *__restrict__ W, const float *__restrict__ table, int F,
                                                         int De, int C, float *__restrict__ WvT,
                                                         float *__restrict__ cpart) {
  __shared__ float ws[4];
  const int j = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63, De1 = De + 1;
  float wsum = 0.f;
  for (int i = 0; i < kPrepF / 4; ++i) {
    const int f = blockIdx.x * kPrepF + w * (kPrepF / 4) + i;
    if (f >= F) break;                                                           // wave-uniform
    const float *wr = W + ((int64_t)j * F + f) * De1;
    float d = 0.f;
    if (table)
      for (int k = lane; k < De; k += 64) d = fmaf(table[(int64_t)f * De + k], wr[k], d);
    wsum += wave_sum(d);
    if (lane == 0) WvT[(int64_t)f * C + j] = wr[De];
  }
  if (lane == 0) ws[w] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) cpart[(int64_t)j * gridDim.x + blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}
__global__ __launch_bounds__(64) void input_const_kernel(const float *__restrict__ cpart, int nfb, float *__restrict__ cvec) {
  const int j = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < nfb; b += 64) s += cpart[(int64_t)j * nfb + b];
  s = wave_sum(s);
  if (threadIdx.x == 0) cvec[j] = s;
}

constexpr int kRows = 16, kKL = 16, kJ = 16, kKC = 128;
// h[n, j] = sum_f z[n, f] WvT[f, j] + cvec[j]: 16 rows x 16 K lanes per workgroup, 16 outputs per lane, WvT through LDS
// in chunks of 128 features; a lane adds its features in ascending order, the 16 K lanes combine in a fixed xor order
__global__ __launch_bounds__(256) void input_fwd_kernel(const float *__restrict__ x, int64_t N, int F,
                                                        const float *__restrict__ mean, const float *__restrict__ inv_std,
                                                        const float *__restrict__ WvT, const float *__restrict__ cvec, int C,
                                                        float *__restrict__ h, int64_t ld_h) {
  __shared__ __align__(16) float wt[kKC * kJ];
  const int kl = threadIdx.x % kKL;
  const int64_t n = (int64_t)blockIdx.x * kRows + threadIdx.x / kKL;
  const float *xr = x + (n < N ? n : 0) * F;
  for (int j0 = 0; j0 < C; j0 += kJ) {
    float acc[kJ];
#pragma unroll
    for (int jj = 0; jj < kJ; ++jj) acc[jj] = 0.f;
    for (int k0 = 0; k0 < F; k0 += kKC) {
      __syncthreads();
      for (int t = threadIdx.x; t < kKC * kJ; t += 256) {
        const int k = k0 + t / kJ, j = j0 + t % kJ;
        wt[t] = (k < F && j < C) ? WvT[(int64_t)k * C + j] : 0.f;
      }
      __syncthreads();
      if (n < N) {
        for (int kk = kl; kk < kKC && k0 + kk < F; kk += kKL) {
          const int k = k0 + kk;
          const float z = mean ? (xr[k] - mean[k]) * inv_std[k] : xr[k];
#pragma unroll
          for (int jj = 0; jj < kJ; ++jj) acc[jj] = fmaf(z, wt[kk * kJ + jj], acc[jj]);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < kKL; o <<= 1)
#pragma unroll
      for (int jj = 0; jj < kJ; ++jj) acc[jj] += __shfl_xor(acc[jj], o, 64);
    if (n < N && kl == 0)
#pragma unroll
      for (int jj = 0; jj < kJ; ++jj)
        if (j0 + jj < C) h[n * ld_h + j0 + jj] = acc[jj] + cvec[j0 + jj];
  }
}

constexpr int kWgF = 64, kWgRows = 64, kWgChunks = 64;
inline int wgrad_chunks(int64_t N) { return (int)std::min<int64_t>(std::max<int64_t>((N + kWgRows - 1) / kWgRows, 1), kWgChunks); }
// partial[nb, f, j] = sum over the rows of chunk nb, ascending, of z[n, f] g[n, j]: 64 features x 4 output quads per
// workgroup, g through LDS in tiles of 64 rows x 16 outputs
__global__ __launch_bounds__(256) void input_wgrad_kernel(const float *__restrict__ x, int64_t N, int F,
                                                          const float *__restrict__ mean, const float *__restrict__ inv_std,
                                                          const float *__restrict__ g, int64_t ld_g, int C,
                                                          float *__restrict__ partial) {
  __shared__ __align__(16) float gt[kWgRows * kJ];
  const int fl = threadIdx.x & 63, jq = threadIdx.x >> 6;
  const int f = blockIdx.x * kWgF + fl;
  const int64_t per = (N + gridDim.y - 1) / gridDim.y, n0 = blockIdx.y * per, n1 = min(N, n0 + per);
  float m = 0.f, is = 1.f;
  if (mean && f < F) {
    m = mean[f];
    is = inv_std[f];
  }
  for (int j0 = 0; j0 < C; j0 += kJ) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t t0 = n0; t0 < n1; t0 += kWgRows) {
      __syncthreads();
      for (int t = threadIdx.x; t < kWgRows * kJ; t += 256) {
        const int64_t n = t0 + t / kJ;
        const int j = j0 + t % kJ;
        gt[t] = (n < n1 && j < C) ? g[n * ld_g + j] : 0.f;
      }
      __syncthreads();
      if (f < F) {
        const int rows = (int)min((int64_t)kWgRows, n1 - t0);
        for (int r = 0; r < rows; ++r) {
          const float z = (x[(t0 + r) * F + f] - m) * is;
          fma4(acc, z, *reinterpret_cast<const float4 *>(gt + r * kJ + jq * 4));
        }
      }
    }
    if (f < F) {
      float *p = partial + ((int64_t)blockIdx.y * F + f) * C;
      const int j = j0 + jq * 4;
      if (j < C) p[j] = acc.x;
      if (j + 1 < C) p[j + 1] = acc.y;
      if (j + 2 < C) p[j + 2] = acc.z;
      if (j + 3 < C) p[j + 3] = acc.w;
    }
  }
}
// one lane per element (f, k) of a [F, De + 1] slice: k < De: dW[j, f, k] = s[j] table[f, k] and dtable[f, k] =
// sum_j s[j] W[j, f, k] (ascending j); k == De: dW[j, f, De] = the chunks of `partial` in ascending order
__global__ __launch_bounds__(256) void input_wgrad_final_kernel(const float *__restrict__ partial, int chunks,
                                                                const float *__restrict__ s, const float *__restrict__ W,
                                                                const float *__restrict__ table, int F, int De, int C,
                                                                float *__restrict__ dW, float *__restrict__ dtable) {
  const int De1 = De + 1;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, FD = (int64_t)F * De1;
  if (t >= FD) return;
  const int f = (int)(t / De1), k = (int)(t - (int64_t)f * De1);
  if (k < De) {
    const float tv = table[(int64_t)f * De + k];
    float dt = 0.f;
    for (int j = 0; j < C; ++j) {
      dW[j * FD + t] = s[j] * tv;
      dt = fmaf(s[j], W[j * FD + t], dt);
    }
    if (dtable) dtable[(int64_t)f * De + k] = dt;
  } else {
    for (int j = 0; j < C; ++j) {
      float sum = 0.f;
      for (int b = 0; b < chunks; ++b) sum += partial[((int64_t)b * F + f) * C + j];
      dW[j * FD + t] = sum;
    }
  }
}

inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
inline size_t input_fwd_bytes(int64_t F, int C) {
  return align16(sizeof(float) * C) + align16(sizeof(float) * F * C) + align16(sizeof(float) * C * ((F + kPrepF - 1) / kPrepF));
}
inline size_t input_bwd_bytes(int64_t N, int64_t F, int C) {
  return align16(sizeof(float) * C) + align16(sizeof(float) * (size_t)kColsumChunks * C) +
         align16(sizeof(float) * (size_t)wgrad_chunks(N) * F * C);
}

}  // namespace

extern "C" int ampconv_gcn_norm(const int32_t *ptr, const int32_t *idx, int64_t N, int add_self_loops, float fill,
                                float *dinv, void *stream) {
  if (!ptr || !idx || !dinv || N < 0 || N > INT32_MAX || !(fill >= 0.f)) return AMPCONV_E_BADARG;
  if (N == 0) return AMPCONV_OK;
  const int64_t blocks = (N + 3) / 4;
  gcn_norm_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(ptr, idx, N, add_self_loops != 0, fill, dinv);
  return ampconv_launch_status();
}

extern "C" size_t ampconv_gcn_aggregate_workspace_bytes(int64_t N, int64_t E, int C) {
  if (N <= 0 || E < kLong || C < 1) return 0;
  const int64_t rows = long_max_rows(E), parts = long_max_parts(E);
  return 16 + 8 * (size_t)rows + 8 * (size_t)parts + 4 * (size_t)parts * C;
}

extern "C" int ampconv_gcn_aggregate(const float *h, int64_t ld_h, int C, const int32_t *ptr, const int32_t *idx,
                                     const float *dinv, int add_self_loops, float fill, const float *bias, float *out,
                                     int64_t ld_out, int64_t N, int64_t E, void *workspace, size_t workspace_bytes,
                                     void *stream) {
  if (!h || !ptr || !idx || !dinv || !out || C < 1 || ld_h < C || ld_out < C || N < 0 || N > INT32_MAX || E < 0 ||
      E > INT32_MAX)
    return AMPCONV_E_BADARG;
  if (((uintptr_t)h | (uintptr_t)out | (uintptr_t)dinv | (uintptr_t)bias) & 3) return AMPCONV_E_BADARG;
  if (N == 0) return AMPCONV_OK;
  hipStream_t st = (hipStream_t)stream;
  AggArgs a{h, ld_h, C, ptr, idx, dinv, add_self_loops != 0, fill, bias, out, ld_out, N, nullptr, 0, 0};
  int64_t part_grid = 1, row_grid = 1;
  if (workspace && E >= kLong) {
    if (((uintptr_t)workspace & 15) || workspace_bytes < ampconv_gcn_aggregate_workspace_bytes(N, E, C))
      return AMPCONV_E_WORKSPACE;
    a.hdr = (int32_t *)workspace;
    a.max_rows = (int)long_max_rows(E);
    a.max_parts = (int)long_max_parts(E);
    part_grid = std::min<int64_t>(a.max_parts, 4096);
    row_grid = std::min<int64_t>(a.max_rows, 1024);
    hipError_t e = hipMemsetAsync(workspace, 0, 16, st);
    if (e != hipSuccess) return (int)e;
  }
  const bool vec = ld_h % 4 == 0 && ld_out % 4 == 0 && (((uintptr_t)h | (uintptr_t)out) & 15) == 0;
  const int quads = (C + 3) / 4;
  if (quads <= 1) return launch_aggregate<1>(a, vec, part_grid, row_grid, st);
  if (quads <= 2) return launch_aggregate<2>(a, vec, part_grid, row_grid, st);
  if (quads <= 4) return launch_aggregate<4>(a, vec, part_grid, row_grid, st);
  if (quads <= 8) return launch_aggregate<8>(a, vec, part_grid, row_grid, st);
  return launch_aggregate<16>(a, vec, part_grid, row_grid, st);
}

extern "C" size_t ampconv_gcn_colsum_workspace_bytes(int64_t N, int C) {
  (void)N;
  return C < 1 ? 0 : sizeof(float) * (size_t)kColsumChunks * C;
}

extern "C" int ampconv_gcn_colsum(const float *g, int64_t ld, int64_t N, int C, float *out, void *workspace,
                                  size_t workspace_bytes, void *stream) {
  if (!g || !out || C < 1 || ld < C || N < 0) return AMPCONV_E_BADARG;
  if (!workspace || workspace_bytes < ampconv_gcn_colsum_workspace_bytes(N, C)) return AMPCONV_E_WORKSPACE;
  return colsum(g, ld, N, C, out, (float *)workspace, (hipStream_t)stream);
}

extern "C" size_t ampconv_gcn_input_workspace_bytes(int64_t N, int64_t F, int C) {
  if (N < 0 || F < 1 || C < 1) return 0;
  return std::max(input_fwd_bytes(F, C), input_bwd_bytes(N, F, C));
}

static int input_args_ok(const float *x, int64_t N, int64_t F, const float *mean, const float *inv_std, const float *W,
                         const float *table, int De, int C) {
  if (!x || !W || N < 0 || F < 1 || F > INT32_MAX || De < 0 || C < 1 || (mean == nullptr) != (inv_std == nullptr) ||
      (De > 0 && !table) || (De == 0 && table) || (De > 0 && !mean))
    return 0;
  return F * (De + 1) <= INT32_MAX;                      // a [F, De + 1] slice is indexed by one lane id
}

extern "C" int ampconv_gcn_input_fwd(const float *x, int64_t N, int64_t F, const float *mean, const float *inv_std,
                                     const float *W, const float *table, int De, int C, float *h, int64_t ld_h,
                                     void *workspace, size_t workspace_bytes, void *stream) {
  if (!input_args_ok(x, N, F, mean, inv_std, W, table, De, C) || !h || ld_h < C) return AMPCONV_E_BADARG;
  // the size the header names covers both directions: held to it here too, though the forward uses less of it
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < ampconv_gcn_input_workspace_bytes(N, F, C))
    return AMPCONV_E_WORKSPACE;
  if (N == 0) return AMPCONV_OK;
  if ((N + kRows - 1) / kRows > INT32_MAX) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int nfb = (int)((F + kPrepF - 1) / kPrepF);
  float *cvec = (float *)workspace;
  float *WvT = (float *)((char *)workspace + align16(sizeof(float) * C));
  float *cpart = (float *)((char *)WvT + align16(sizeof(float) * F * C));
  input_prep_kernel<<<dim3(nfb, C), 256, 0, st>>>(W, table, (int)F, De, C, WvT, cpart);
  input_const_kernel<<<C, 64, 0, st>>>(cpart, nfb, cvec);
  input_fwd_kernel<<<(unsigned)((N + kRows - 1) / kRows), 256, 0, st>>>(x, N, (int)F, mean, inv_std, WvT, cvec, C, h, ld_h);
  return ampconv_launch_status();
}

extern "C" int ampconv_gcn_input_bwd(const float *x, int64_t N, int64_t F, const float *mean, const float *inv_std,
                                     const float *W, const float *table, int De, int C, const float *g, int64_t ld_g,
                                     float *dW, float *dtable, void *workspace, size_t workspace_bytes, void *stream) {
  if (!input_args_ok(x, N, F, mean, inv_std, W, table, De, C) || !g || !dW || ld_g < C || (De > 0 && !dtable) ||
      (De == 0 && dtable))
    return AMPCONV_E_BADARG;
  if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < input_bwd_bytes(N, F, C)) return AMPCONV_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  float *s = (float *)workspace;
  float *cpartial = (float *)((char *)workspace + align16(sizeof(float) * C));
  float *partial = (float *)((char *)cpartial + align16(sizeof(float) * (size_t)kColsumChunks * C));
  if (int rc = colsum(g, ld_g, N, C, s, cpartial, st)) return rc;
  const int chunks = wgrad_chunks(N);
  input_wgrad_kernel<<<dim3((unsigned)((F + kWgF - 1) / kWgF), chunks), 256, 0, st>>>(x, N, (int)F, mean, inv_std, g, ld_g,
                                                                                      C, partial);
  const int64_t FD = F * (De + 1);
  input_wgrad_final_kernel<<<(unsigned)((FD + 255) / 256), 256, 0, st>>>(partial, chunks, s, W, table, (int)F, De, C, dW,
                                                                         dtable);
  return ampconv_launch_status();
}
