// Feature-to-feature attention heatmap, accumulated on the device (include/ampconv.h, ampconv_attn_heatmap).
//
// Reference: experiments/visualize_cora_attn_coeffs.py:212-216 (calculate_attn_heatmap) averages every coefficient of
// conv.attn_output_weights [E, L, L] into the cell (feature of the source token, feature of the destination token).
// Here the [E, L, L] tensor never exists: per edge the scores, the softmax and the head mean stay on chip and each
// weight goes straight into the table.
//
// Deterministic: a weight w in [0, 1] is added as the integer rint(w * 2^AMPCONV_HEATMAP_SHIFT) with 64-bit integer
// atomics, so the tables are bitwise independent of launch order, of how the edges are split over calls and of the
// number of ranks that are summed later.  Quantised ONCE per (edge, i, j), after the head mean.
//
// Work distribution: a wave takes windows of 64 consecutive edges.  Lane l of a window tests edge l -- mask, node ids
// in range, at least one selected source token AND one selected destination token (2 L position reads) -- and only the
// edges that pass (one ballot) ever touch Q or K.
//   heat_mfma    : shapes of ampconv_mfma_supported (L <= 20, dh in {16, 32}): S^T = K_s Q_d^T on
//                  v_mfma_f32_16x16x4_f32, both operands cut straight from global memory with the lane maps of
//                  mfma_tile.h (each tile is used for ONE product, so an LDS image would be written and read once),
//                  the forward kernel's in-register column softmax, 8 waves per workgroup.
//   heat_generic : any L, any dh; the tile loads, score loop and softmax of attn_weights_generic (edge_generic.hip),
//                  one wave per workgroup.
// Two accumulation targets with the same arithmetic (the integers added are the same, so are the results):
//   LDS    : tables of at most kLdsCells cells -- the workgroup keeps a private copy (64-bit sums, 32-bit counts) and
//            adds its non-empty cells to the global tables once, at its end;
//   global : larger tables, global atomics per weight.  AMPCONV_HEATMAP_GLOBAL=1 in the environment pins this target
//            (used by the tests to cross-check the two).
#include <cstdlib>
#include "mfma_tile.h"

namespace {

typedef unsigned long long u64;

constexpr int kLdsCells = 4096;            // 12 bytes per cell: 48 KB
constexpr int kHeatWaves = 8;              // waves per workgroup of heat_mfma
constexpr int64_t kMaxTriples = AMPCONV_HEATMAP_MAX_TRIPLES;

struct HeatArgs {
  ampconv_view_t Q, K;
  const int64_t *edge_index;
  int64_t E, N;
  const uint8_t *mask;
  const int32_t *rowpos, *colpos;
  u64 *sum, *cnt;
  int L, dh, dhp, H, rows, cols;
  float scale;                             // heat_mfma: log2(e) / sqrt(dh); heat_generic: 1 / sqrt(dh)
  float invH;
  int64_t n_windows;
};

__device__ __forceinline__ u64 quantise(float w) {
  const float q = __builtin_rintf(w * (float)(1 << AMPCONV_HEATMAP_SHIFT));    // w * 2^S is exact
  return (u64)(unsigned)__builtin_fminf(__builtin_fmaxf(q, 0.f), (float)(1 << AMPCONV_HEATMAP_SHIFT));
}

// the workgroup's private tables (LDS = true) or the global ones
template <bool LDS>
struct Target {
  u64 *sum;
  unsigned *lcnt;
  u64 *gcnt;
  int cols;
  __device__ __forceinline__ void add(int r, int c, float w) const {
    if (LDS) {
      const int cell = r * cols + c;
      atomicAdd(sum + cell, quantise(w));
      atomicAdd(lcnt + cell, 1u);
    } else {
      const int64_t cell = (int64_t)r * cols + c;
      atomicAdd(sum + cell, quantise(w));
      atomicAdd(gcnt + cell, (u64)1);
    }
  }
};

template <bool LDS>
__device__ __forceinline__ Target<LDS> target_begin(const HeatArgs &a, void *lds_table) {
  Target<LDS> t;
  t.cols = a.cols;
  t.gcnt = a.cnt;
  if (LDS) {
    const int cells = a.rows * a.cols;
    t.sum = reinterpret_cast<u64 *>(lds_table);
    t.lcnt = reinterpret_cast<unsigned *>(t.sum + cells);
    for (int i = threadIdx.x; i < cells; i += blockDim.x) {
      t.sum[i] = 0;
      t.lcnt[i] = 0;
    }
    __syncthreads();
  } else {
    t.sum = a.sum;
    t.lcnt = nullptr;
  }
  return t;
}

template <bool LDS>
__device__ __forceinline__ void target_end(const HeatArgs &a, const Target<LDS> &t) {
  if (!LDS) return;
  __syncthreads();
  const int cells = a.rows * a.cols;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const unsigned n = t.lcnt[i];
    if (n) {
      atomicAdd(a.sum + i, t.sum[i]);
      atomicAdd(a.cnt + i, (u64)n);
    }
  }
}

// softmax over the 20 source tokens of one destination-token column, held as (t0[0..3] = tokens 4g..4g+3,
// t1[0] = token 16+g) across the 4 lane groups g: the forward kernel's column_softmax (edge_mfma.hip) with the
// tokens >= L masked.
__device__ __forceinline__ void column_softmax(f32x4 &t0, f32x4 &t1, int L, int g) {
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (4 * g + q >= L) t0[q] = kNegBig;
  if (16 + g >= L) t1[0] = kNegBig;
  float m = fmaxf(fmaxf(fmaxf(t0[0], t0[1]), fmaxf(t0[2], t0[3])), t1[0]);
  m = groups_max(m);
#pragma unroll
  for (int q = 0; q < 4; ++q) t0[q] = fast_exp2(t0[q] - m);
  t1[0] = fast_exp2(t1[0] - m);
  float l = (t0[0] + t0[1]) + (t0[2] + t0[3]) + t1[0];
  l = groups_sum(l);
  const float inv = fast_rcp(l);
#pragma unroll
  for (int q = 0; q < 4; ++q) t0[q] *= inv;
  t1[0] *= inv;
}

// position of a token in the table, or -1 (not selected, or outside the table)
__device__ __forceinline__ int table_pos(const int32_t *pos, int64_t node, int L, int tok, int extent) {
  if (tok >= L) return -1;
  const int p = pos[node * L + tok];
  return (unsigned)p < (unsigned)extent ? p : -1;
}

// Lane l tests edge e0 + l; returns the ballot of the edges that contribute, s / d = the lane's edge.
__device__ __forceinline__ u64 window_scan(const HeatArgs &a, int64_t e0, int lane, int64_t &s, int64_t &d) {
  const int64_t e = e0 + lane;
  bool ok = e < a.E && (!a.mask || a.mask[e] != 0);
  s = ok ? a.edge_index[e] : 0;
  d = ok ? a.edge_index[a.E + e] : 0;
  ok = ok && (u64)s < (u64)a.N && (u64)d < (u64)a.N;
  bool any_r = false, any_c = false;
  if (ok) {
    const int32_t *rp = a.rowpos + s * a.L, *cp = a.colpos + d * a.L;
    for (int j = 0; j < a.L; ++j) {
      any_r |= (unsigned)rp[j] < (unsigned)a.rows;
      any_c |= (unsigned)cp[j] < (unsigned)a.cols;
    }
  }
  return __ballot(ok && any_r && any_c);
}

__device__ __forceinline__ int64_t lane_value(int64_t v, int k) {      // k is wave-uniform
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)(u64)v, k);
  const unsigned hi = __builtin_amdgcn_readlane((int)(unsigned)((u64)v >> 32), k);
  return (int64_t)(((u64)hi << 32) | lo);
}

// ---- MFMA path.  C/D layout of S^T (mfma_tile.h): lane (i' = lane & 15, g = lane >> 4) of column tile nt holds
// destination token i' + 16 nt against the source tokens 4 g + q (row tile 0, reg q) and 16 + g (row tile 1, reg 0).
template <int DH, bool LDS>
__global__ __launch_bounds__(64 * kHeatWaves) void heat_mfma(HeatArgs a) {
  using C = TileCfg<DH>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_table[];
  const Target<LDS> tgt = target_begin<LDS>(a, lds_table);
  const int lane = threadIdx.x & 63, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int L = a.L;
  const int64_t n_waves = (int64_t)gridDim.x * kHeatWaves;
  for (int64_t win = (int64_t)blockIdx.x * kHeatWaves + wave; win < a.n_windows; win += n_waves) {
    int64_t s_l, d_l;
    u64 act = window_scan(a, win * 64, lane, s_l, d_l);
    while (act) {
      const int k = __builtin_ctzll(act);
      act &= act - 1;
      const int64_t s = lane_value(s_l, k), d = lane_value(d_l, k);
      int cp[2], rp[5];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) cp[nt] = table_pos(a.colpos, d, L, (lane & 15) + 16 * nt, a.cols);
#pragma unroll
      for (int q = 0; q < 4; ++q) rp[q] = table_pos(a.rowpos, s, L, 4 * g + q, a.rows);
      rp[4] = table_pos(a.rowpos, s, L, 16 + g, a.rows);

      float W[2][5];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < 5; ++q) W[nt][q] = 0.f;
      for (int h = 0; h < a.H; ++h) {
        const float *kb = tile_ptr<const float>(a.K, s, h), *qb = tile_ptr<const float>(a.Q, d, h);
        float kA[2][C::KK], qB[2][C::KK];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          rowop_from_global<DH>(kA[t], kb, a.K.row_stride, t, false, 1.f, L, lane);
          rowop_from_global<DH>(qB[t], qb, a.Q.row_stride, t, true, a.scale, L, lane);
        }
        f32x4 S[2][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          S[mt][0] = S[mt][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kk = 0; kk < C::KK; ++kk) {
            S[mt][0] = MFMA16(kA[mt][kk], qB[0][kk], S[mt][0]);
            S[mt][1] = MFMA16(kA[mt][kk], qB[1][kk], S[mt][1]);
          }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          column_softmax(S[0][nt], S[1][nt], L, g);
#pragma unroll
          for (int q = 0; q < 4; ++q) W[nt][q] = fmaf(S[0][nt][q], a.invH, W[nt][q]);
          W[nt][4] = fmaf(S[1][nt][0], a.invH, W[nt][4]);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < 5; ++q)
          if (cp[nt] >= 0 && rp[q] >= 0) tgt.add(rp[q], cp[nt], W[nt][q]);
    }
  }
  target_end<LDS>(a, tgt);
}

// ---- shape-generic path: one wave per workgroup; LDS = Q tile, K tile, one softmax row, the head-mean weights
// [L, L], the positions of the 2 L tokens, then the private tables.
template <bool LDS>
__global__ __launch_bounds__(AMPCONV_WAVE) void heat_generic(HeatArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x;
  const int L = a.L, dh = a.dh, dhp = a.dhp, T = L * dhp;
  float *Qs = reinterpret_cast<float *>(lds_raw), *Ks = Qs + T, *P = Ks + T, *Wl = P + L;
  int *rp = reinterpret_cast<int *>(Wl + L * L), *cp = rp + L;
  const size_t table_off = (((size_t)2 * T + L + (size_t)L * L + 2 * L) * sizeof(float) + 15) & ~(size_t)15;
  const Target<LDS> tgt = target_begin<LDS>(a, lds_raw + table_off);
  for (int64_t win = blockIdx.x; win < a.n_windows; win += gridDim.x) {
    int64_t s_l, d_l;
    u64 act = window_scan(a, win * 64, lane, s_l, d_l);
    while (act) {
      const int k = __builtin_ctzll(act);
      act &= act - 1;
      const int64_t s = lane_value(s_l, k), d = lane_value(d_l, k);
      __syncthreads();
      for (int j = lane; j < L; j += AMPCONV_WAVE) {
        rp[j] = table_pos(a.rowpos, s, L, j, a.rows);
        cp[j] = table_pos(a.colpos, d, L, j, a.cols);
      }
      for (int h = 0; h < a.H; ++h) {
        __syncthreads();
        const float *qb = tile_ptr<const float>(a.Q, d, h), *kb = tile_ptr<const float>(a.K, s, h);
        for (int idx = lane; idx < L * dh; idx += AMPCONV_WAVE) {
          const int j = idx / dh, c = idx - j * dh;
          Qs[j * dhp + c] = a.scale * qb[(int64_t)j * a.Q.row_stride + c];
          Ks[j * dhp + c] = kb[(int64_t)j * a.K.row_stride + c];
        }
        __syncthreads();
        for (int i = 0; i < L; ++i) {
          // softmax over the source tokens of destination token i (softmax_row of edge_generic.hip)
          const float *Qi = Qs + i * dhp;
          float m = -INFINITY;
          for (int j = lane; j < L; j += AMPCONV_WAVE) {
            float sc = 0.f;
            for (int c = 0; c < dh; ++c) sc = fmaf(Qi[c], Ks[j * dhp + c], sc);
            P[j] = sc;
            m = fmaxf(m, sc);
          }
          m = wave_max(m);
          float l = 0.f;
          for (int j = lane; j < L; j += AMPCONV_WAVE) {
            const float p = expf(P[j] - m);
            P[j] = p;
            l += p;
          }
          l = wave_sum(l);
          const float inv = 1.f / l;
          for (int j = lane; j < L; j += AMPCONV_WAVE) {       // P[j] is this lane's own
            float w = P[j] * inv * a.invH;
            if (h > 0) w += Wl[i * L + j];
            Wl[i * L + j] = w;
          }
        }
      }
      __syncthreads();
      for (int idx = lane; idx < L * L; idx += AMPCONV_WAVE) {
        const int i = idx / L, j = idx - i * L;
        if (rp[j] >= 0 && cp[i] >= 0) tgt.add(rp[j], cp[i], Wl[idx]);
      }
    }
  }
  target_end<LDS>(a, tgt);
}

bool force_global() { return env_switch("AMPCONV_HEATMAP_GLOBAL", false); }

template <typename K>
int set_dynamic_lds(K kernel, size_t bytes) {
  if (bytes > 160 * 1024) return AMPCONV_E_BADARG;
  if (bytes > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return (int)e;
  }
  return AMPCONV_OK;
}

template <typename K>
int launch(K kernel, const HeatArgs &a, unsigned grid, unsigned block, size_t lds, hipStream_t stream) {
  if (int rc = set_dynamic_lds(kernel, lds)) return rc;
  kernel<<<grid, block, lds, stream>>>(a);
  return ampconv_launch_status();
}

}  // namespace

extern "C" int ampconv_attn_heatmap(ampconv_view_t Q, ampconv_view_t K, const int64_t *edge_index, int64_t E,
                                    int64_t N, const uint8_t *edge_mask, const int32_t *rowpos,
                                    const int32_t *colpos, int L, int D, int H, int rows, int cols, int64_t *sum,
                                    int64_t *cnt, int64_t prior_triples, int dtype, void *stream) {
  if (dtype != AMPCONV_F32) return AMPCONV_E_DTYPE;
  if (L <= 0 || D <= 0 || H <= 0 || D % H != 0) return AMPCONV_E_BADARG;
  if (E < 0 || E > INT32_MAX || N < 0 || rows <= 0 || cols <= 0 || prior_triples < 0) return AMPCONV_E_BADARG;
  if ((int64_t)rows * cols > INT32_MAX || L > 4096) return AMPCONV_E_BADARG;
  if (!sum || !cnt || ((uintptr_t)sum & 7) || ((uintptr_t)cnt & 7)) return AMPCONV_E_BADARG;
  // a cell receives at most 2^SHIFT per (edge, i, j): refuse what could pass INT64_MAX instead of wrapping
  if (prior_triples > kMaxTriples || E * (int64_t)L * L > kMaxTriples - prior_triples) return AMPCONV_E_BADARG;
  if (E == 0) return AMPCONV_OK;
  if (!view_ok(Q) || !view_ok(K) || !edge_index || !rowpos || !colpos) return AMPCONV_E_BADARG;

  const int dh = D / H;
  HeatArgs a{};
  a.Q = Q; a.K = K;
  a.edge_index = edge_index; a.E = E; a.N = N;
  a.mask = edge_mask; a.rowpos = rowpos; a.colpos = colpos;
  a.sum = reinterpret_cast<u64 *>(sum); a.cnt = reinterpret_cast<u64 *>(cnt);
  a.L = L; a.dh = dh; a.dhp = dh | 1; a.H = H; a.rows = rows; a.cols = cols;
  a.invH = 1.f / (float)H;
  a.n_windows = (E + 63) / 64;
  const int64_t cells = (int64_t)rows * cols;
  const size_t table_bytes = (size_t)cells * (sizeof(u64) + sizeof(unsigned));
  const ampconv_view_t views[2] = {Q, K};
  const bool mfma = ampconv_mfma_supported(L, D, H) && ampconv_mfma_views_ok(views, 2);
  const int waves_per_block = mfma ? kHeatWaves : 1;
  const int64_t max_blocks = mfma ? 1024 : 4096;
  const int64_t want = (a.n_windows + waves_per_block - 1) / waves_per_block;
  const unsigned grid = (unsigned)(want < max_blocks ? want : max_blocks);
  // the private counts are 32 bits wide: a workgroup must not see 2^32 triples
  const int64_t windows_per_wave = (a.n_windows + (int64_t)grid * waves_per_block - 1) / ((int64_t)grid * waves_per_block);
  const bool lds = cells <= kLdsCells && !force_global() &&
                   windows_per_wave * 64 * waves_per_block * L * L < ((int64_t)1 << 32);
  hipStream_t st = (hipStream_t)stream;
  if (mfma) {
    a.scale = 1.4426950408889634f / sqrtf((float)dh);
    const size_t bytes = lds ? table_bytes : 0;
    const unsigned block = 64 * kHeatWaves;
    if (dh == 32) return lds ? launch(heat_mfma<32, true>, a, grid, block, bytes, st)
                             : launch(heat_mfma<32, false>, a, grid, block, bytes, st);
    return lds ? launch(heat_mfma<16, true>, a, grid, block, bytes, st)
               : launch(heat_mfma<16, false>, a, grid, block, bytes, st);
  }
  a.scale = 1.f / sqrtf((float)dh);
  const size_t tiles = ((((size_t)2 * L * a.dhp + L + (size_t)L * L + 2 * L) * sizeof(float)) + 15) & ~(size_t)15;
  if (lds && tiles + table_bytes <= 160 * 1024) return launch(heat_generic<true>, a, grid, AMPCONV_WAVE, tiles + table_bytes, st);
  return launch(heat_generic<false>, a, grid, AMPCONV_WAVE, tiles, st);
}

extern "C" int ampconv_attn_heatmap_shift(void) { return AMPCONV_HEATMAP_SHIFT; }
