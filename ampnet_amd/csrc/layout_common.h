// What the three layout methods share (tsne.hip, umap.hip, spring.hip; included by nothing else): the fixed fp64
// reductions, the chunked N-body pass of the repulsive terms, and the gather over CSR rows with its long-row scheme.
// Everything is static or in the anonymous namespace: each object holds its own copy.
//
// N-body chunks.  A VALU all-pairs kernel: the inner dimension is 2 or 3, the matrix cores have nothing to offer.  A
// workgroup of 256 lanes owns a tile of 1024 query points (four per lane: four independent reciprocals in flight, a
// key is read once for four pairs) and one chunk of keys.  Keys are read at a workgroup-uniform address (one scalar
// load serves the wave: no LDS, no vector memory traffic) and enter the VALU as scalar operands.  A lane's fp32 sums
// live for a run of 256 keys, in key order, then go into its fp64 sums; a chunk's fp64 sums go to the workspace
// [chunk][plane][N] and fold_chunks adds the chunks in order.  The chunk length (nbody_chunk_keys) is a function of N
// alone, so the bits do not depend on how the work is spread.  The chunk kernels themselves are the methods' own: their
// register forms differ (scalar fp32 with an index compare in t-SNE, packed pairs of query points in spring) and a
// frame over both was longer than the two kernels (profiles/layout_common_refactor.md).  Shared are the chunk rule, the
// workspace layout and the fold.
//
// CSR rows.  One wave per row; lane l takes the entries l, l + 64, ... of the row and a butterfly adds the lanes.  A
// row longer than `part` entries is cut into parts of that length, counted from the row's start, which a launch in
// front sums: one wave per WINDOW of `part` positions of the entry array (for_window_parts).  At most two parts start
// in a window -- one of the row that holds the window's first position (side 0), one of a long row that starts inside
// the window (side 1) -- so no plan and no read-back is needed, and the row's wave adds its parts in order in fp64.
//
// Grouped gather (UMAP, spring).  A row is cut into GROUPS of 64 entries counted from its start, lane l takes entry l
// of the group, the row's groups are added in order in fp64, coordinate c on lane c.  The part length is a multiple
// of 64, so a part is whole groups: gather_parts stores every group's sum of the long rows and gather_row adds the
// stored groups in the same order.  The part length therefore only decides who computes a group, never what is added
// to what: the bits do not depend on it.  What one entry contributes is the method's (its entry functor); every entry
// is visited by exactly one lane of one launch.
#pragma once
#include "common.h"

namespace {

constexpr int kGroup = 64;
constexpr int kMaxChunks = 64;
static_assert(kGroup == AMPCONV_WAVE, "lane l takes entry l of a group");

// ------------------------------------------------------------------------------------------------------ reductions
// the tree of a 256-lane workgroup, one fixed order
__device__ __forceinline__ double block_sum_f64(double v, double *s) {
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}

// out[b] = the sum of in[b n .. b n + n): lane t adds the elements t, t + 256, ... in order, then the tree
[[maybe_unused]] __global__ __launch_bounds__(256) void sum_rows_kernel(const double *__restrict__ in, int64_t n,
                                                                        double *__restrict__ out) {
  __shared__ double s[256];
  const double *p = in + (int64_t)blockIdx.x * n;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) v += p[i];
  v = block_sum_f64(v, s);
  if (threadIdx.x == 0) out[blockIdx.x] = v;
}

// --------------------------------------------------------------------------------------------------- N-body chunks
// keys per chunk, from N alone: chunk0 times ceil(ceil(N / chunk0) / 64), so at most 64 chunks
inline int nbody_chunk_keys(int64_t N, int chunk0) {
  const int64_t c0 = (N + chunk0 - 1) / chunk0;
  return chunk0 * (int)((c0 + kMaxChunks - 1) / kMaxChunks);
}
inline int nbody_chunk_count(int64_t N, int chunk0) {
  return (int)((N + nbody_chunk_keys(N, chunk0) - 1) / nbody_chunk_keys(N, chunk0));
}

// point i's sums over the chunks, in chunk order, in fp64
template <int P>
__device__ __forceinline__ void fold_chunks(const double *__restrict__ part, int chunks, int N, int i, double (&s)[P]) {
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = 0.0;
  for (int c = 0; c < chunks; ++c) {
    const double *o = part + (int64_t)c * P * N;
#pragma unroll
    for (int p = 0; p < P; ++p) s[p] += o[(int64_t)p * N + i];
  }
}

// -------------------------------------------------------------------------------------------------------- CSR rows
// Nothing read from indptr or indices is followed out of the arrays: positions are clamped to [0, nnz], columns to
// [0, N).
struct CsrRows {
  const int64_t *indptr, *indices;
  int64_t N, nnz;

  __device__ __forceinline__ int64_t clamp_pos(int64_t p) const { return p < 0 ? 0 : (p > nnz ? nnz : p); }
  // the largest row r with indptr[r] <= p: the row that holds entry p
  __device__ __forceinline__ int64_t row_of(int64_t p) const {
    int64_t lo = 0, hi = N - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (indptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
  }
  // the entries [beg, end) of row i, end >= beg
  __device__ __forceinline__ void span(int64_t i, int64_t &beg, int64_t &end) const {
    beg = clamp_pos(indptr[i]);
    end = max(beg, clamp_pos(indptr[i + 1]));
  }
  __device__ __forceinline__ int64_t col(int64_t e) const {
    const int64_t j = indices[e];
    return j < 0 ? 0 : (j >= N ? N - 1 : j);
  }
};

inline int64_t window_count(int64_t nnz, int64_t part) { return (nnz + part - 1) / part; }

// f(r, beg, end, ps, pe, side) for each part [ps, pe) of a row r = [beg, end) longer than `part` that starts in
// window w; wave-uniform
template <class F>
__device__ __forceinline__ void for_window_parts(const CsrRows &R, int64_t part, int64_t w, const F &f) {
  const int64_t p0 = w * part;
  if (p0 >= R.nnz) return;
  const int64_t pl = min(p0 + part, R.nnz) - 1;
  const int64_t ra = R.row_of(p0), rb = R.row_of(pl);
  for (int side = 0; side < 2; ++side) {
    if (side == 1 && rb == ra) break;
    const int64_t r = side ? rb : ra;
    int64_t beg, end;
    R.span(r, beg, end);
    if (end - beg <= part) continue;
    int64_t ps = beg;                                                // side 1: the row starts inside the window
    if (side == 0) {
      ps = beg + (p0 - beg + part - 1) / part * part;                // the first part of row ra that starts at or after p0
      if (ps > pl || ps >= end || ps < p0) continue;
    } else if (beg <= p0 || beg > pl) {
      continue;
    }
    f(r, beg, end, ps, min(ps + part, end), side);
  }
}

// -------------------------------------------------------------------------------------------------- grouped gather
// where the sum of group g of a row that starts at entry `beg` lies: rows r' < r hold at most beg / 64 + r groups
__device__ __forceinline__ int64_t group_slot(int64_t beg, int64_t r, int64_t g) { return beg / kGroup + r + g; }
// the workspace [nnz / 64 + N + 1][dim] of the group sums of the rows longer than a part
inline size_t groups_bytes(int64_t N, int64_t nnz, int dim) {
  return pad256((size_t)(nnz / kGroup + N + 1) * (size_t)dim * sizeof(float));
}

// point j of y[.][dim] into D >= dim registers
template <int D>
__device__ __forceinline__ void load_point(const float *y, int dim, int64_t j, float (&v)[D]) {
  if constexpr (D == 2) {
    const float2 t = reinterpret_cast<const float2 *>(y)[j];
    v[0] = t.x; v[1] = t.y;
  } else {
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = c < dim ? y[j * dim + c] : 0.f;
  }
}

// d = a - b per coordinate; returns |d|^2 by FMAs over the coordinates in order
template <int D>
__device__ __forceinline__ float difference(const float (&a)[D], const float (&b)[D], float (&d)[D]) {
  float d2 = 0.f;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    d[c] = a[c] - b[c];
    d2 = fmaf(d[c], d[c], d2);
  }
  return d2;
}

// the group of 64 entries at g0 of a row at yi that ends at `end`; entry(yi, e, s) adds what entry e contributes to
// s.  Every lane returns the sums.
template <int D, class E>
__device__ __forceinline__ void group_sum(const E &entry, const float (&yi)[D], int64_t g0, int64_t end, int lane,
                                          float (&s)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) s[c] = 0.f;
  if (g0 + lane < end) entry(yi, g0 + lane, s);
#pragma unroll
  for (int c = 0; c < D; ++c) s[c] = wave_sum(s[c]);
}

// the parts launch: grid ceil(windows / 4), 256 lanes; stores the group sums of every part
template <int D, class E>
__device__ __forceinline__ void gather_parts(const CsrRows &R, const float *y, int dim, int64_t part,
                                             float *groups, const E &entry) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for_window_parts(R, part, w, [&](int64_t r, int64_t beg, int64_t, int64_t ps, int64_t pe, int) {
    float yi[D], s[D];
    load_point<D>(y, dim, r, yi);
    for (int64_t g0 = ps; g0 < pe; g0 += kGroup) {
      group_sum<D>(entry, yi, g0, pe, lane, s);
      float *o = groups + group_slot(beg, r, (g0 - beg) / kGroup) * dim;
#pragma unroll
      for (int c = 0; c < D; ++c)
        if (lane == c && c < dim) o[c] = s[c];
    }
  });
}

// row i by its wave: lane c < dim returns the fp64 sum of coordinate c over the row's groups in order
template <int D, class E>
__device__ __forceinline__ double gather_row(const CsrRows &R, const float *y, int dim, int64_t part, const float *groups,
                                             int64_t i, int lane, const E &entry) {
  int64_t beg, end;
  R.span(i, beg, end);
  double acc = 0.0;
  if (end - beg <= part) {
    float yi[D], s[D];
    load_point<D>(y, dim, i, yi);
    for (int64_t g0 = beg; g0 < end; g0 += kGroup) {
      group_sum<D>(entry, yi, g0, end, lane, s);
#pragma unroll
      for (int c = 0; c < D; ++c)
        if (lane == c) acc += (double)s[c];
    }
  } else if (lane < dim) {
    const float *o = groups + group_slot(beg, i, 0) * dim + lane;
    for (int64_t g = 0, n = (end - beg + kGroup - 1) / kGroup; g < n; ++g) acc += (double)o[g * dim];
  }
  return acc;
}

}  // namespace
