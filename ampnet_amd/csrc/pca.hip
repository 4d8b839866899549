// PCA of node features and embeddings (include/ampconv.h, "principal components"): the means, the W x W matrix
// Sm = A^T A of the shifted rows in fp64, and the projection of the shifted rows on a few vectors.  The eigen-
// decomposition between the two is a library call on the Python side (ampnet_amd/pca.py).
//
// Gram.  A workgroup owns a 128 x 128 block of Sm -- 8 x 8 tiles of 16 x 16, only blocks and tiles on or above the
// diagonal -- and one split of the rows.  Rows come through LDS in 32-row tiles (row_stream.h's raw4 / cook4, asked for
// one tile ahead, the shift subtracted in fp32 on the way in): the block's two column panels side by side, one on the
// diagonal.  Wave w of the eight owns tile row w: per four rows one A operand (panel I, columns 16 w ..) and up to
// eight B operands (panel J) from LDS, v_mfma_f32_16x16x4_f32 (exact fp32 products).  The fp32 accumulators live for a
// run of AMPCONV_PCA_RUN rows (one tile), then go into fp64 registers; a split's fp64 tiles are written to the workspace and
// pca_fold_kernel adds the splits in order and mirrors.  No atomics: the result is bitwise reproducible.
//   LDS: 32 x 272 floats (row stride 16 mod 64 banks: the four rows of an operand read fall on different banks) + 256
//   shift values = 35 840 bytes; registers: 32 fp32 + 64 (fp64) accumulators, 16 for the tile in flight.
// Projection.  A workgroup owns 64 rows (a wave 16) and all k <= 128 outputs: x in [64][32] and V in [32][16 nt] LDS
// tiles per 32-column step, the same MFMA, fp32 accumulators over all of W.
#include "row_stream.h"

namespace {

constexpr int kRun = AMPCONV_PCA_RUN;
constexpr int kRunTiles = kRun / kTS;
static_assert(kRun % kTS == 0, "a run is whole tiles");

struct RowsArgs {                    // what row_stream.h's loaders read
  const void *Z;
  int64_t ldz;
  int D, bf16, vec;
};

// ---------------------------------------------------------------------------------------------------------- means
constexpr int kMeanChunks = 512;     // at most this many row chunks (fp64 partial sums [chunk][W] in the workspace)
constexpr int kMeanMinRows = 64;

struct MeanSplit { int64_t per; int n; };
MeanSplit mean_split(int64_t R) {
  MeanSplit s;
  s.per = std::max<int64_t>(kMeanMinRows, (R + kMeanChunks - 1) / kMeanChunks);
  s.n = (int)((R + s.per - 1) / s.per);
  return s;
}

// per column: the sum of one chunk of rows.  Lane = column (coalesced rows), wave w walks rows w, w + 4, ... of the
// chunk in order; the four waves' sums are added in order.
__global__ __launch_bounds__(256) void pca_colsum_kernel(const RowsArgs a, int64_t R, int64_t per, double *part) {
  __shared__ double s_p[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = min(r0 + per, R);
  double s = 0.0;
  if (col < a.D)
    for (int64_t r = r0 + wave; r < r1; r += 4) s += (double)load1(a, r, col);
  s_p[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && col < a.D)
    part[(int64_t)blockIdx.y * a.D + col] = ((s_p[0][lane] + s_p[1][lane]) + s_p[2][lane]) + s_p[3][lane];
}
__global__ __launch_bounds__(256) void pca_colmean_kernel(const double *part, int n, int W, int64_t R, float *out) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= W) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += part[(int64_t)i * W + col];
  out[col] = (float)(s / (double)R);
}
// per row: 16 lanes per row, lane l sums the columns l, l + 16, ... in order, then the lanes pairwise
__global__ __launch_bounds__(256) void pca_rowmean_kernel(const RowsArgs a, int64_t R, float *out) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  const int l = (int)(gid & 15);
  for (int64_t row = gid >> 4; row < R; row += stride >> 4) {        // the 16 lanes of a row stay in the loop together
    double s = 0.0;
    for (int c = l; c < a.D; c += 16) s += (double)load1(a, row, c);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (l == 0) out[row] = (float)(s / (double)a.D);
  }
}

// ----------------------------------------------------------------------------------------------------------- Gram
constexpr int kGT = 512;             // eight waves
constexpr int kGB = 128;             // columns of a panel: 8 tiles
constexpr int kGLd = 2 * kGB + 16;   // LDS row stride in floats
constexpr int kGNL = kTS * (2 * kGB / 4) / kGT;      // 16-byte chunks of a tile per thread: 4, two per panel
constexpr size_t kGramCap = (size_t)64 << 20;        // the partials stay under 64 MiB from the second split on
constexpr int kGramMaxSplit = 128;
constexpr int kGramMinTiles = 8;             // a split is at least this many tiles (256 rows) long

struct GramArgs {
  const void *Z;
  int64_t ldz;
  int D, bf16, vec;                  // D = W
  int64_t R;
  const float *rs, *cs;
  int tiles, per, panels;
  double *part;                      // [split][W][W], the elements on and above the diagonal
};

struct GramSplit { int tiles, per, n, panels, pairs; };
// splits of the rows, from the shape alone: enough workgroups for the card, a split at least 256 rows long, at most
// 128, and the fp64 partials [split][W][W] under 64 MiB from the second split on
GramSplit gram_split(int64_t R, int W) {
  GramSplit s;
  s.tiles = (int)((R + kTS - 1) / kTS);
  s.panels = (W + kGB - 1) / kGB;
  s.pairs = s.panels * (s.panels + 1) / 2;
  int64_t n = (768 + s.pairs - 1) / s.pairs;
  n = std::min<int64_t>(n, (s.tiles + kGramMinTiles - 1) / kGramMinTiles);
  n = std::max<int64_t>(std::min<int64_t>(n, kGramMaxSplit), 1);
  while (n > 1 && (size_t)n * (size_t)W * (size_t)W * sizeof(double) > kGramCap) --n;
  s.per = (int)((s.tiles + n - 1) / n);
  s.per = std::max(1, (s.per + kRunTiles - 1) / kRunTiles * kRunTiles);      // whole runs
  s.n = std::max(1, (s.tiles + s.per - 1) / s.per);
  return s;
}

template <int PATH>
__device__ __forceinline__ void gram_body(const GramArgs &a, float *tile, const float *s_cs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, ks = lane >> 4;
  int bi = 0, p = blockIdx.x;
  while (p >= a.panels - bi) { p -= a.panels - bi; ++bi; }
  const int bj = bi + p;
  const bool diag = bi == bj;
  const int offI = bi * kGB, offJ = bj * kGB, ldsJ = diag ? 0 : kGB;
  const int sp = blockIdx.y;
  const int t0 = sp * a.per, t1 = min(t0 + a.per, a.tiles);

  // this thread's chunks of a tile: rows lrow and lrow + 16, chunk lch of panel I (kk 0, 1) and of panel J (kk 2, 3)
  const int lrow = tid >> 5, lch = tid & 31;
  const int nl = diag ? 2 : kGNL;
  uint4 pf[kGNL];
  float prs[2] = {0.f, 0.f};
  auto load_rows = [&](int t) {
#pragma unroll
    for (int kk = 0; kk < kGNL; ++kk) {
      if (kk >= nl) continue;                                          // workgroup-uniform
      const int64_t s = (int64_t)t * kTS + lrow + 16 * (kk & 1);
      pf[kk] = raw4<PATH>(a, s < a.R ? s : a.R - 1, (kk < 2 ? offI : offJ) + 4 * lch);
    }
    if (a.rs) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int64_t s = (int64_t)t * kTS + lrow + 16 * h;
        prs[h] = a.rs[s < a.R ? s : a.R - 1];
      }
    }
  };

  const bool active = offI + 16 * wave < a.D;                          // wave-uniform
  const int tlo = diag ? wave : 0, thi = min(8, (a.D - offJ + 15) / 16);
  f32x4 acc[8];
  double dacc[8][4];
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) dacc[tt][q] = 0.0;
  }

  if (t0 < t1) load_rows(t0);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kGNL; ++kk) {
      if (kk >= nl) continue;
      const int row = lrow + 16 * (kk & 1), gc = (kk < 2 ? offI : offJ) + 4 * lch, lc = (kk < 2 ? 0 : kGB) + 4 * lch;
      const bool ok = (int64_t)t * kTS + row < a.R;
      float4 v = cook4<PATH>(a, pf[kk], gc, ok);
      const float4 cs = *reinterpret_cast<const float4 *>(s_cs + lc);
      const float sh = prs[kk & 1];
      v.x = ok && gc < a.D ? (v.x - sh) - cs.x : 0.f;                  // one of the two shifts is 0: one rounding
      v.y = ok && gc + 1 < a.D ? (v.y - sh) - cs.y : 0.f;
      v.z = ok && gc + 2 < a.D ? (v.z - sh) - cs.z : 0.f;
      v.w = ok && gc + 3 < a.D ? (v.w - sh) - cs.w : 0.f;
      *reinterpret_cast<float4 *>(tile + row * kGLd + lc) = v;
    }
    __syncthreads();
    if (t + 1 < t1) load_rows(t + 1);

    if (active) {
      // a pair of tiles at a time (two independent MFMA chains), one wave-uniform branch per pair: a branch per product
      // made the compiler spill the accumulators
      const float *rowp = tile + ks * kGLd + c;
      float av[kTS / 4];
#pragma unroll
      for (int s = 0; s < kTS / 4; ++s) av[s] = rowp[4 * s * kGLd + 16 * wave];
#pragma unroll
      for (int tp = 0; tp < 4; ++tp) {
        if (2 * tp + 1 < tlo || 2 * tp >= thi) continue;
#pragma unroll
        for (int s = 0; s < kTS / 4; ++s) {
          acc[2 * tp] = MFMA16(av[s], rowp[4 * s * kGLd + ldsJ + 32 * tp], acc[2 * tp]);
          acc[2 * tp + 1] = MFMA16(av[s], rowp[4 * s * kGLd + ldsJ + 32 * tp + 16], acc[2 * tp + 1]);
        }
      }
      if ((t - t0 + 1) % kRunTiles == 0 || t + 1 == t1) {              // the end of a run: fp32 -> fp64
#pragma unroll
        for (int tt = 0; tt < 8; ++tt) {
#pragma unroll
          for (int q = 0; q < 4; ++q) dacc[tt][q] += (double)acc[tt][q];
          acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
  }

  if (!active) return;
  double *P = a.part + (int64_t)sp * a.D * a.D;
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    if (!(tt >= tlo && tt < thi)) continue;
    const int j = offJ + 16 * tt + c;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = offI + 16 * wave + 4 * ks + q;                     // C/D: lane (c, ks), reg q = <row 4 ks + q, column c>
      if (i < a.D && j < a.D && i <= j) P[(int64_t)i * a.D + j] = dacc[tt][q];
    }
  }
}

__global__ __launch_bounds__(kGT) void pca_gram_kernel(const GramArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kTS * kGLd];
  __shared__ __attribute__((aligned(16))) float s_cs[2 * kGB];
  {
    int bi = 0, p = blockIdx.x;
    while (p >= a.panels - bi) { p -= a.panels - bi; ++bi; }
    const int tid = threadIdx.x;
    if (tid < 2 * kGB) {
      const int col = tid < kGB ? bi * kGB + tid : (bi + p) * kGB + tid - kGB;
      s_cs[tid] = a.cs && col < a.D ? a.cs[col] : 0.f;                 // read after the loop's first barrier
    }
  }
  by_path(a, [&](auto path) { gram_body<decltype(path)::value>(a, tile, s_cs); });
}

// Sm[i][j] = Sm[j][i] = the splits' partials added in order, i <= j
__global__ __launch_bounds__(256) void pca_fold_kernel(const double *part, int n, int W, double *Sm) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= W || j >= W || i > j) return;
  double s = 0.0;
  for (int sp = 0; sp < n; ++sp) s += part[((int64_t)sp * W + i) * W + j];
  Sm[(int64_t)i * W + j] = s;
  Sm[(int64_t)j * W + i] = s;
}

// ----------------------------------------------------------------------------------------------------- projection
constexpr int kPT = 256;             // four waves of 16 rows
constexpr int kPR = 64;
constexpr int kPK = 32;              // columns of x per step
constexpr int kPLdx = kPK + 4;       // x tile row stride: 16 rows x 4 columns of an operand read on 64 different banks
constexpr int kPLdv = 128 + 16;      // V tile row stride: 16 mod 64

struct ProjArgs {
  const void *Z;
  int64_t ldz;
  int D, bf16, vec;
  int64_t R;
  const float *rs, *cs, *V, *scale;
  int k, nt;                         // nt = ceil(k / 16)
  float *out;
  int64_t ldo;
};

template <int PATH>
__device__ __forceinline__ void proj_body(const ProjArgs &a, float *xt, float *vt) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, ks = lane >> 4;
  const int64_t row0 = (int64_t)blockIdx.x * kPR;
  const int lrow = tid >> 3, lch = tid & 7;                            // rows lrow and lrow + 32, chunk lch
  const int steps = (a.D + kPK - 1) / kPK, kp = 16 * a.nt;

  float rsv[2] = {0.f, 0.f};
  bool rok[2];
  int64_t rid[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t r = row0 + lrow + 32 * h;
    rok[h] = r < a.R;
    rid[h] = rok[h] ? r : a.R - 1;
    if (a.rs) rsv[h] = a.rs[rid[h]];
  }
  uint4 pf[2];
  float pcs[4] = {0.f, 0.f, 0.f, 0.f};
  auto load_x = [&](int st) {
    const int gc = kPK * st + 4 * lch;
#pragma unroll
    for (int h = 0; h < 2; ++h) pf[h] = raw4<PATH>(a, rid[h], gc);
    if (a.cs) {
#pragma unroll
      for (int e = 0; e < 4; ++e) pcs[e] = a.cs[gc + e < a.D ? gc + e : 0];
    }
  };

  f32x4 acc[8];
#pragma unroll
  for (int tt = 0; tt < 8; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_x(0);
  for (int st = 0; st < steps; ++st) {
    __syncthreads();
    const int gc = kPK * st + 4 * lch;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float4 v = cook4<PATH>(a, pf[h], gc, rok[h]);
      v.x = rok[h] && gc < a.D ? (v.x - rsv[h]) - pcs[0] : 0.f;
      v.y = rok[h] && gc + 1 < a.D ? (v.y - rsv[h]) - pcs[1] : 0.f;
      v.z = rok[h] && gc + 2 < a.D ? (v.z - rsv[h]) - pcs[2] : 0.f;
      v.w = rok[h] && gc + 3 < a.D ? (v.w - rsv[h]) - pcs[3] : 0.f;
      *reinterpret_cast<float4 *>(xt + (lrow + 32 * h) * kPLdx + 4 * lch) = v;
    }
    for (int e = tid; e < kPK * kp; e += kPT) {                        // V rows of this step, zero beyond W and k
      const int w = e / kp, j = e - w * kp, gw = kPK * st + w;
      vt[w * kPLdv + j] = gw < a.D && j < a.k ? a.V[(int64_t)gw * a.k + j] : 0.f;
    }
    __syncthreads();
    if (st + 1 < steps) load_x(st + 1);

#pragma unroll
    for (int s = 0; s < kPK / 4; ++s) {
      const float av = xt[(16 * wave + c) * kPLdx + 4 * s + ks];       // A: lane (row c, k ks)
      const float *vp = vt + (4 * s + ks) * kPLdv + c;                 // B: lane (k ks, column c)
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
        if (tt < a.nt) acc[tt] = MFMA16(av, vp[16 * tt], acc[tt]);
    }
  }

#pragma unroll
  for (int tt = 0; tt < 8; ++tt) {
    if (tt >= a.nt) continue;
    const int j = 16 * tt + c;
    if (j >= a.k) continue;
    const float sc = a.scale ? a.scale[j] : 1.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = row0 + 16 * wave + 4 * ks + q;
      if (r < a.R) a.out[r * a.ldo + j] = a.scale ? sc * acc[tt][q] : acc[tt][q];
    }
  }
}

__global__ __launch_bounds__(kPT) void pca_project_kernel(const ProjArgs a) {
  __shared__ __attribute__((aligned(16))) float xt[kPR * kPLdx];
  __shared__ __attribute__((aligned(16))) float vt[kPK * kPLdv];
  by_path(a, [&](auto path) { proj_body<decltype(path)::value>(a, xt, vt); });
}

// ---- host side
constexpr int64_t kMaxRows = INT32_MAX;

bool shape_ok(int64_t R, int W, int64_t ldx, int dtype) {
  return R >= 1 && R <= kMaxRows && W >= 1 && W <= AMPCONV_PCA_MAX_W && ldx >= W && (dtype == AMPCONV_F32 || dtype == AMPCONV_BF16);
}
template <typename A>
void set_rows(A &a, const void *x, int W, int64_t ldx, int dtype) {
  a.Z = x; a.ldz = ldx; a.D = W;
  a.bf16 = dtype == AMPCONV_BF16;
  a.vec = W % 4 == 0 && ldx % 4 == 0 && (uintptr_t)x % (4 * (a.bf16 ? 2 : 4)) == 0;
}

}  // namespace

extern "C" size_t ampconv_pca_shift_workspace_bytes(int64_t R, int W, int axis) {
  if (R < 1 || R > kMaxRows || W < 1 || W > AMPCONV_PCA_MAX_W || (axis != 0 && axis != 1)) return 0;
  return axis == 0 ? pad256((size_t)mean_split(R).n * (size_t)W * sizeof(double)) : 0;
}

extern "C" int ampconv_pca_shift(const void *x, int64_t R, int W, int64_t ldx, int axis, float *out, void *workspace,
                                 size_t workspace_bytes, int dtype, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!shape_ok(R, W, ldx, dtype) || (axis != 0 && axis != 1) || !x || !out) return AMPCONV_E_BADARG;
  RowsArgs a = {};
  set_rows(a, x, W, ldx, dtype);
  if (axis == 1) {
    const int64_t blocks = std::min<int64_t>((R * 16 + 255) / 256, 1 << 16);
    pca_rowmean_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(a, R, out);
    return ampconv_launch_status();
  }
  if (!workspace || workspace_bytes < ampconv_pca_shift_workspace_bytes(R, W, axis)) return AMPCONV_E_WORKSPACE;
  const MeanSplit s = mean_split(R);
  pca_colsum_kernel<<<dim3((unsigned)((W + 63) / 64), (unsigned)s.n), dim3(256), 0, stream>>>(a, R, s.per, (double *)workspace);
  if (int rc = ampconv_launch_status()) return rc;
  pca_colmean_kernel<<<dim3((unsigned)((W + 255) / 256)), dim3(256), 0, stream>>>((const double *)workspace, s.n, W, R, out);
  return ampconv_launch_status();
}

extern "C" int ampconv_pca_gram_splits(int64_t R, int W) {
  if (R < 1 || R > kMaxRows || W < 1 || W > AMPCONV_PCA_MAX_W) return 0;
  return gram_split(R, W).n;
}

extern "C" size_t ampconv_pca_gram_workspace_bytes(int64_t R, int W) {
  if (R < 1 || R > kMaxRows || W < 1 || W > AMPCONV_PCA_MAX_W) return 0;
  return pad256((size_t)gram_split(R, W).n * (size_t)W * (size_t)W * sizeof(double));
}

extern "C" int ampconv_pca_gram(const void *x, int64_t R, int W, int64_t ldx, const float *row_shift,
                                const float *col_shift, double *Sm, void *workspace, size_t workspace_bytes, int dtype,
                                void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!shape_ok(R, W, ldx, dtype) || !x || !Sm) return AMPCONV_E_BADARG;
  if (!workspace || workspace_bytes < ampconv_pca_gram_workspace_bytes(R, W)) return AMPCONV_E_WORKSPACE;
  const GramSplit s = gram_split(R, W);
  GramArgs a = {};
  set_rows(a, x, W, ldx, dtype);
  a.R = R; a.rs = row_shift; a.cs = col_shift;
  a.tiles = s.tiles; a.per = s.per; a.panels = s.panels;
  a.part = (double *)workspace;
  pca_gram_kernel<<<dim3((unsigned)s.pairs, (unsigned)s.n), dim3(kGT), 0, stream>>>(a);
  if (int rc = ampconv_launch_status()) return rc;
  pca_fold_kernel<<<dim3((unsigned)((W + 63) / 64), (unsigned)((W + 3) / 4)), dim3(256), 0, stream>>>(a.part, s.n, W, Sm);
  return ampconv_launch_status();
}

extern "C" int ampconv_pca_project(const void *x, int64_t R, int W, int64_t ldx, const float *row_shift,
                                   const float *col_shift, const float *V, int k, const float *scale, float *out,
                                   int64_t ldo, int dtype, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!shape_ok(R, W, ldx, dtype) || !x || !V || !out) return AMPCONV_E_BADARG;
  if (k < 1 || k > AMPCONV_PCA_MAX_K || ldo < k) return AMPCONV_E_BADARG;
  ProjArgs a = {};
  set_rows(a, x, W, ldx, dtype);
  a.R = R; a.rs = row_shift; a.cs = col_shift; a.V = V; a.scale = scale;
  a.k = k; a.nt = (k + 15) / 16;
  a.out = out; a.ldo = ldo;
  pca_project_kernel<<<dim3((unsigned)((R + kPR - 1) / kPR)), dim3(kPT), 0, stream>>>(a);
  return ampconv_launch_status();
}
