// GraphSAGE pair loss over node embeddings (include/ampconv.h, "pair loss"): logits A N^T tiled on chip, never in memory.
//
// One kernel skeleton serves the three products.  A wave keeps 16 rows of the FIXED side in registers and walks the
// STREAMED side in 32-row LDS tiles that the four waves of a workgroup share:
//   forward: fixed = anchors,   streamed = negatives: online (max, sum) per anchor, or the softplus sum
//   pass 1 : fixed = anchors,   streamed = negatives: pi N   (anchor role; the positive role falls out of the epilogue)
//   pass 2 : fixed = negatives, streamed = anchors  : pi^T A (negative role)
// Products on v_mfma_f32_16x16x4_f32 (exact fp32; bf16 rows widened on load), K zero-padded to DP = 16 KQ4 channels.
//   logits : A operand = streamed tile (lane (r, g): row r, channel g KQ + t at step t), B operand = fixed rows in the same
//            channel order -> C/D lane (r, g), reg q = logit(fixed r, streamed 4 g + q)
//   second : that register IS the A operand of the second product (row = fixed r, k = g <-> streamed 4 g + q), B operand
//            = tile[4 g + q][16 ct + r] -> C/D lane (r, g), reg q = out(fixed 4 g + q, channel 16 ct + r): no transposes.
// The streamed range is split over blockIdx.y where the fixed side alone does not fill the card; every split writes its own
// partial, merged in split order (forward: pair_rows_kernel; backward: pair_fold_kernel).  No atomics anywhere.
#include "row_stream.h"

namespace {

constexpr int kThreads = 256;      // four waves = 64 fixed rows per workgroup
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

struct PairArgs {
  const void *Z;
  int64_t ldz, N;
  int D, Dq, bf16, vec;
  const int64_t *fid, *sid, *pos;      // fixed ids, streamed ids, positives (pass 1)
  int nf, ns, tiles, tiles_per_split;
  float scale, neg_weight;
  int xent, exclude;
  const float *aff, *neg_term, *weight, *g0;
  float *out, *outp;                   // pass 1 / 2: partials [split][nf][Dq]; pass 1: positive role [nf][Dq]
  float *pm, *ps;                      // forward: partial (max, sum) [split][nf]
};

__device__ __forceinline__ float exp_f(float x) { return fast_exp2(x * kLog2e); }
__device__ __forceinline__ float softplus_f(float x) {        // max(x, 0) + log1p(exp(-|x|))
  return fmaxf(x, 0.f) + kLn2 * __builtin_amdgcn_logf(1.f + exp_f(-__builtin_fabsf(x)));
}
__device__ __forceinline__ float sigmoid_f(float x) {         // no overflow at either end
  const float e = exp_f(-__builtin_fabsf(x)), s = fast_rcp(1.f + e);
  return x >= 0.f ? s : e * s;
}

// MODE 0: forward, 1: pass 1 (anchor tiles), 2: pass 2 (negative tiles)
template <int KQ4, int MODE, bool XENT>
__global__ __launch_bounds__(kThreads) void pair_kernel(const PairArgs a) {
  constexpr int KQ = 4 * KQ4, DP = 16 * KQ4, LDR = DP + 4, CH = DP / 4;
  constexpr int XCH = KQ4 < 8 ? KQ4 : 8;               // row-operand chunks in flight
  constexpr bool PRELOAD = KQ4 <= 8;                    // all 4 KQ4 column operands of a sub-tile at once, else per step
  constexpr int NL = (kTS * CH + kThreads - 1) / kThreads;
  __shared__ __attribute__((aligned(16))) float tile[kTS * LDR];
  __shared__ int s_id[kTS];
  __shared__ float s_lse[kTS], s_w[kTS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int f0 = (blockIdx.x * (kThreads / 64) + wave) * 16, fr = f0 + r;
  const bool valid_f = fr < a.nf;
  const int sp = blockIdx.y;
  const int64_t fidc = clamp_id(a.fid[valid_f ? fr : 0], a.N);

  float fx[KQ];
#pragma unroll
  for (int j = 0; j < KQ4; ++j) {
    const float4 v = load4(a, fidc, g * KQ + 4 * j);
    fx[4 * j] = v.x; fx[4 * j + 1] = v.y; fx[4 * j + 2] = v.z; fx[4 * j + 3] = v.w;
  }
  const float lse_f = (MODE == 1 && valid_f) ? a.neg_term[fr] : 0.f;

  f32x4 acc[MODE == 0 ? 1 : KQ4];
  if (MODE != 0) {
#pragma unroll
    for (int ct = 0; ct < KQ4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float run_m = kNegBig, run_s = 0.f;

  const int t0 = sp * a.tiles_per_split, t1 = min(t0 + a.tiles_per_split, a.tiles);

  // The rows of a tile are one tile ahead in registers and their ids two: a row's address hangs on its id, and a wave that
  // waits for the id before it can ask for the row stands still for a memory round trip per chunk, in front of its products.
  // Nothing that was asked for is looked at before the next iteration: ids stay as loaded until load_rows clamps them, rows
  // and the per-row terms until the LDS stores convert and mask them.
  uint4 pf[NL];                         // as loaded (raw4); converted and zero-padded on the way into LDS (cook4)
  int64_t rid[NL];                      // id of the row of chunk k, as loaded
  int64_t nx_id = 0;                    // lanes < kTS of wave 0: the id of tile row `tid`, for s_id
  int pf_id = -1;
  float pf_lse = 0.f, pf_w = 1.f;
  auto load_ids = [&](int t) {
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int i = tid + kThreads * k, row = i / CH, s = t * kTS + row;
      rid[k] = a.sid[row < kTS && s < a.ns ? s : 0];
    }
    if (tid < kTS) nx_id = a.sid[t * kTS + tid < a.ns ? t * kTS + tid : 0];
  };
  auto load_rows = [&](int t) {         // the tile whose ids load_ids brought; rows behind the end read row id 0, masked later
    by_path(a, [&](auto path) {
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        const int i = tid + kThreads * k, row = i / CH, ch = i - row * CH;
        pf[k] = raw4<decltype(path)::value>(a, clamp_id(rid[k], a.N), 4 * ch);
      }
    });
    if (tid < kTS) {
      const int s = t * kTS + tid;
      pf_id = s < a.ns ? (int)clamp_id(nx_id, a.N) : -1;
      if (MODE == 2) {
        pf_lse = a.neg_term[s < a.ns ? s : 0];
        if (a.weight) pf_w = a.weight[s < a.ns ? s : 0];
      }
    }
  };

  load_ids(t0);
  load_rows(t0);
  load_ids(t0 + 1);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
    by_path(a, [&](auto path) {
#pragma unroll
      for (int k = 0; k < NL; ++k) {
        const int i = tid + kThreads * k, row = i / CH, ch = i - row * CH;
        if (row < kTS)
          *reinterpret_cast<float4 *>(tile + row * LDR + 4 * ch) =
              cook4<decltype(path)::value>(a, pf[k], 4 * ch, t * kTS + row < a.ns);
      }
    });
    if (tid < kTS) {
      s_id[tid] = pf_id;
      if (MODE == 2) { s_lse[tid] = pf_lse; s_w[tid] = pf_id >= 0 ? pf_w : 0.f; }
    }
    __syncthreads();
    if (t + 1 < t1) {
      load_rows(t + 1);
      load_ids(t + 2);
    }

    const int cnt = min(kTS, a.ns - t * kTS);
#pragma unroll
    for (int sub = 0; sub < kTS / 16; ++sub) {
      if (sub * 16 >= cnt) break;                       // workgroup-uniform
      // every LDS operand of the sub-tile is asked for before the product that reads it: the loads of the second product
      // travel under the logits and the exponentials instead of one round trip in front of every MFMA pair
      const float *rowp = tile + (sub * 16 + r) * LDR + g * KQ;
      const float *bp = tile + (sub * 16 + 4 * g) * LDR + r;
      f32x4 lg = {0.f, 0.f, 0.f, 0.f}, lg1 = {0.f, 0.f, 0.f, 0.f};
      float bs[MODE != 0 && PRELOAD ? 4 * KQ4 : 1];
#pragma unroll
      for (int j0 = 0; j0 < KQ4; j0 += XCH) {
        float4 xs[XCH];
#pragma unroll
        for (int j = 0; j < XCH; ++j)
          if (j0 + j < KQ4) xs[j] = *reinterpret_cast<const float4 *>(rowp + 4 * (j0 + j));
        if (MODE != 0 && PRELOAD && j0 == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int ct = 0; ct < KQ4; ++ct) bs[q * KQ4 + ct] = bp[q * LDR + 16 * ct];
        }
        if (PRELOAD) __builtin_amdgcn_sched_barrier(0);   // the scheduler would sink every load back to its first use
#pragma unroll
        for (int j = 0; j < XCH; ++j) {
          if (j0 + j >= KQ4) continue;
          lg = MFMA16(xs[j].x, fx[4 * (j0 + j)], lg);         // two chains: a dependent MFMA issues 8 cycles late
          lg1 = MFMA16(xs[j].y, fx[4 * (j0 + j) + 1], lg1);
          lg = MFMA16(xs[j].z, fx[4 * (j0 + j) + 2], lg);
          lg1 = MFMA16(xs[j].w, fx[4 * (j0 + j) + 3], lg1);
        }
      }
      lg += lg1;
      float gl[4];
      bool kept[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int id = s_id[sub * 16 + 4 * g + q];      // -1 behind the end of the streamed side
        gl[q] = a.scale * lg[q];
        kept[q] = id >= 0 && valid_f && !(a.exclude && id == (int)fidc);
      }
      if (MODE == 0) {
        if (XENT) {
#pragma unroll
          for (int q = 0; q < 4; ++q) run_s += kept[q] ? softplus_f(gl[q]) : 0.f;
        } else {
          float m = run_m;
#pragma unroll
          for (int q = 0; q < 4; ++q) m = kept[q] ? fmaxf(m, gl[q]) : m;
          run_s *= exp_f(run_m - m);
#pragma unroll
          for (int q = 0; q < 4; ++q) run_s += kept[q] ? exp_f(gl[q] - m) : 0.f;
          run_m = m;
        }
      } else {
        float p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int srow = sub * 16 + 4 * g + q;
          float v = XENT ? a.neg_weight * sigmoid_f(gl[q]) : exp_f(gl[q] - (MODE == 1 ? lse_f : s_lse[srow]));
          if (MODE == 2) v *= s_w[srow];
          p[q] = kept[q] ? v : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (PRELOAD) {
#pragma unroll
            for (int ct = 0; ct < KQ4; ++ct) acc[ct] = MFMA16(p[q], bs[q * KQ4 + ct], acc[ct]);
          } else {
            float bq[KQ4];
#pragma unroll
            for (int ct = 0; ct < KQ4; ++ct) bq[ct] = bp[q * LDR + 16 * ct];
#pragma unroll
            for (int ct = 0; ct < KQ4; ++ct) acc[ct] = MFMA16(p[q], bq[ct], acc[ct]);
          }
        }
      }
    }
  }

  if (MODE == 0) {
    // the four lane groups of a fixed row, merged pairwise: every lane ends with the same (max, sum)
#pragma unroll
    for (int o = 16; o <= 32; o <<= 1) {
      const float om = __shfl_xor(run_m, o, 64), os = __shfl_xor(run_s, o, 64);
      if (XENT) {
        run_s += os;
      } else {
        const float m = fmaxf(run_m, om);
        run_s = run_s * exp_f(run_m - m) + os * exp_f(om - m);
        run_m = m;
      }
    }
    if (g == 0 && valid_f) {
      a.pm[(int64_t)sp * a.nf + fr] = run_m;
      a.ps[(int64_t)sp * a.nf + fr] = run_s;
    }
    return;
  }

  const float g0 = *a.g0;
  if (MODE == 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = f0 + 4 * g + q;
      if (row >= a.nf) continue;
      const float coef = g0 * (a.weight ? a.weight[row] : 1.f) * a.scale;
      const float cb = XENT ? -sigmoid_f(-a.aff[row]) : -1.f;
      const int64_t pid = clamp_id(a.pos[row], a.N);
      float *o = a.out + ((int64_t)sp * a.nf + row) * a.Dq;
#pragma unroll
      for (int ct = 0; ct < KQ4; ++ct) {
        const int c = 16 * ct + r;
        if (c < a.Dq) o[c] = coef * (acc[ct][q] + (sp == 0 ? cb * load1(a, pid, c) : 0.f));
      }
    }
    if (sp == 0 && valid_f) {                          // positive role: g0 w scale c_b a_b, from the fixed registers
      const float cb = XENT ? -sigmoid_f(-a.aff[fr]) : -1.f;
      const float coef = g0 * (a.weight ? a.weight[fr] : 1.f) * a.scale * cb;
      float *o = a.outp + (int64_t)fr * a.Dq;
#pragma unroll
      for (int j = 0; j < KQ4; ++j) {
        const int c = g * KQ + 4 * j;
        if (c < a.Dq)
          *reinterpret_cast<float4 *>(o + c) =
              make_float4(coef * fx[4 * j], coef * fx[4 * j + 1], coef * fx[4 * j + 2], coef * fx[4 * j + 3]);
      }
    }
  } else {
    const float coef = g0 * a.scale;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = f0 + 4 * g + q;
      if (row >= a.nf) continue;
      float *o = a.out + ((int64_t)sp * a.nf + row) * a.Dq;
#pragma unroll
      for (int ct = 0; ct < KQ4; ++ct) {
        const int c = 16 * ct + r;
        if (c < a.Dq) o[c] = coef * acc[ct][q];
      }
    }
  }
}

// ---- forward, per pair: aff, the partials of the splits merged in split order, w_b l_b; bounds flag of every id
struct RowsArgs {
  const void *Z;
  int64_t ldz, N;
  int D, bf16, xent, splits;
  const int64_t *anchor, *positive, *negative;
  const float *weight, *pm, *ps;
  int B, S;
  float scale, neg_weight;
  float *aff, *neg_term, *wl;
  int32_t *oob;
};
__global__ __launch_bounds__(256) void pair_rows_kernel(const RowsArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, b = gid >> 4;
  const int l = (int)(gid & 15);
  bool bad = false;
  for (int64_t i = gid; i < a.S; i += (int64_t)gridDim.x * 256) {
    const int64_t v = a.negative[i];
    bad |= v < 0 || v >= a.N;
  }
  if (b < a.B) {                                       // 16 lanes per pair; B is covered by the grid
    const int64_t ia = a.anchor[b], ip = a.positive[b];
    bad |= ia < 0 || ia >= a.N || ip < 0 || ip >= a.N;
    const int64_t ra = clamp_id(ia, a.N), rp = clamp_id(ip, a.N);
    float dot = 0.f;
    for (int c = l; c < a.D; c += 16) {
      float x, y;
      if (a.bf16) {
        x = bf16_f32(reinterpret_cast<const uint16_t *>(a.Z)[ra * a.ldz + c]);
        y = bf16_f32(reinterpret_cast<const uint16_t *>(a.Z)[rp * a.ldz + c]);
      } else {
        x = reinterpret_cast<const float *>(a.Z)[ra * a.ldz + c];
        y = reinterpret_cast<const float *>(a.Z)[rp * a.ldz + c];
      }
      dot = fmaf(x, y, dot);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (l == 0) {
      const float aff = a.scale * dot;
      float neg, loss;
      if (a.xent) {
        neg = 0.f;
        for (int k = 0; k < a.splits; ++k) neg += a.ps[(int64_t)k * a.B + b];
        loss = softplus_f(-aff) + a.neg_weight * neg;
      } else {
        float m = kNegBig, s = 0.f;
        for (int k = 0; k < a.splits; ++k) m = fmaxf(m, a.pm[(int64_t)k * a.B + b]);
        for (int k = 0; k < a.splits; ++k) s += a.ps[(int64_t)k * a.B + b] * exp_f(a.pm[(int64_t)k * a.B + b] - m);
        neg = s > 0.f ? m + logf(s) : 0.f;           // no kept negative: a negative term of 0
        loss = neg - aff;
      }
      a.aff[b] = aff;
      a.neg_term[b] = neg;
      a.wl[b] = (a.weight ? a.weight[b] : 1.f) * loss;
    }
  }
  if (bad) *a.oob = 1;
}

// loss = sum_b wl[b]: one workgroup, fixed order
__global__ __launch_bounds__(1024) void pair_sum_kernel(const float *wl, int B, float *loss) {
  __shared__ float part[1024];
  float s = 0.f;
  for (int i = threadIdx.x; i < B; i += 1024) s += wl[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = part[0];
}

// ---- backward, per node: the role gradients of its slots summed in slot-list order, partials in split order
struct FoldArgs {
  const float *ra, *rp, *rn;        // [sa][B][Dq], [B][Dq], [sn][S][Dq]
  const int32_t *ptr, *idx;
  int64_t N, lddz;
  int B, S, D, Dq, sa, sn, bf16;
  void *dZ;
};
__global__ __launch_bounds__(256) void pair_fold_kernel(const FoldArgs a) {
  const int chunks = a.Dq / 4;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, n = gid / chunks;
  if (n >= a.N) return;
  const int c = 4 * (int)(gid - n * chunks), total = 2 * a.B + a.S;
  const int beg = max(0, min(a.ptr[n], total)), end = max(beg, min(a.ptr[n + 1], total));
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p = beg; p < end; ++p) {
    const int slot = max(0, min(a.idx[p], total - 1));
    const float *base;
    int parts;
    int64_t step;
    if (slot < a.B) { base = a.ra + (int64_t)slot * a.Dq; parts = a.sa; step = (int64_t)a.B * a.Dq; }
    else if (slot < 2 * a.B) { base = a.rp + (int64_t)(slot - a.B) * a.Dq; parts = 1; step = 0; }
    else { base = a.rn + (int64_t)(slot - 2 * a.B) * a.Dq; parts = a.sn; step = (int64_t)a.S * a.Dq; }
    for (int k = 0; k < parts; ++k) {
      const float4 v = *reinterpret_cast<const float4 *>(base + k * step + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  const float v[4] = {s.x, s.y, s.z, s.w};
  for (int i = 0; i < 4 && c + i < a.D; ++i) {
    if (a.bf16) {
      unsigned u = __float_as_uint(v[i]);
      u = (u & 0x7F800000u) == 0x7F800000u ? (u | ((u & 0xFFFFu) ? 0x10000u : 0u)) : u + 0x7FFFu + ((u >> 16) & 1u);   // RNE
      reinterpret_cast<uint16_t *>(a.dZ)[n * a.lddz + c + i] = (uint16_t)(u >> 16);
    } else {
      reinterpret_cast<float *>(a.dZ)[n * a.lddz + c + i] = v[i];
    }
  }
}

// ---- host side
int dq_of(int D) { return (D + 3) & ~3; }

struct BwdLayout { Split a, n; size_t off_p, off_n, bytes; };
BwdLayout bwd_layout(int64_t B, int64_t S, int D) {
  BwdLayout l;
  const size_t rb = (size_t)dq_of(D) * sizeof(float);
  l.a = stream_split(B, S, rb);
  l.n = stream_split(S, B, rb);
  l.off_p = pad256((size_t)l.a.n * B * rb);
  l.off_n = l.off_p + pad256((size_t)B * rb);
  l.bytes = l.off_n + pad256((size_t)l.n.n * S * rb);
  return l;
}
size_t fwd_bytes(int64_t B, int64_t S) {
  return pad256((size_t)stream_split(B, S, 0).n * B * sizeof(float)) * 2 + pad256((size_t)B * sizeof(float));
}

template <int KQ4, int MODE>
void launch_kq(const PairArgs &a, dim3 grid, hipStream_t stream) {
  if (a.xent) pair_kernel<KQ4, MODE, true><<<grid, dim3(kThreads), 0, stream>>>(a);
  else pair_kernel<KQ4, MODE, false><<<grid, dim3(kThreads), 0, stream>>>(a);
}
template <int MODE>
int launch_pair(const PairArgs &a, int splits, hipStream_t stream) {
  const dim3 grid((unsigned)((a.nf + 63) / 64), (unsigned)splits);
  const int kq4 = (a.D + 15) / 16;
  if (kq4 <= 1) launch_kq<1, MODE>(a, grid, stream);
  else if (kq4 <= 2) launch_kq<2, MODE>(a, grid, stream);
  else if (kq4 <= 4) launch_kq<4, MODE>(a, grid, stream);
  else if (kq4 <= 7) launch_kq<7, MODE>(a, grid, stream);
  else if (kq4 <= 8) launch_kq<8, MODE>(a, grid, stream);
  else launch_kq<16, MODE>(a, grid, stream);
  return ampconv_launch_status();
}

bool pair_args_ok(const void *Z, int64_t N, int D, int64_t ldz, const int64_t *anchor, const int64_t *positive, int64_t B,
                  const int64_t *negative, int64_t S, int kind, int dtype) {
  if (B < 0 || S < 0 || N < 0 || D < 1 || D > AMPCONV_PAIR_MAX_D || ldz < D) return false;
  if (kind != AMPCONV_PAIR_SKIPGRAM && kind != AMPCONV_PAIR_XENT) return false;
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return false;
  if (B > 0 && (S < 1 || N < 1 || !Z || !anchor || !positive || !negative)) return false;
  if (N > INT32_MAX || B > (1 << 29) || S > (1 << 29)) return false;      // 2 B + S and every row index fit an int32
  return true;
}

PairArgs base_args(const void *Z, int64_t N, int D, int64_t ldz, float scale, float neg_weight, int kind, int exclude,
                   const float *weight, int dtype) {
  PairArgs a = {};
  a.Z = Z; a.ldz = ldz; a.N = N; a.D = D; a.Dq = dq_of(D);
  a.bf16 = dtype == AMPCONV_BF16;
  const size_t el = a.bf16 ? 2 : 4;
  a.vec = D % 4 == 0 && ldz % 4 == 0 && (uintptr_t)Z % (4 * el) == 0;
  a.scale = scale; a.neg_weight = neg_weight; a.xent = kind == AMPCONV_PAIR_XENT; a.exclude = exclude != 0;
  a.weight = weight;
  return a;
}

}  // namespace

extern "C" size_t ampconv_pair_loss_workspace_bytes(int64_t B, int64_t S, int D) {
  if (B <= 0 || S < 0 || D < 1 || D > AMPCONV_PAIR_MAX_D) return 0;
  return std::max(fwd_bytes(B, S), bwd_layout(B, S, D).bytes);
}

extern "C" int ampconv_pair_loss_fwd(const void *Z, int64_t N, int D, int64_t ldz, const int64_t *anchor,
                                     const int64_t *positive, int64_t B, const int64_t *negative, int64_t S,
                                     const float *weight, int kind, float scale, float neg_weight, int exclude_anchor,
                                     float *aff, float *neg_term, float *loss, int32_t *oob, void *workspace,
                                     size_t workspace_bytes, int dtype, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!pair_args_ok(Z, N, D, ldz, anchor, positive, B, negative, S, kind, dtype) || !loss || !oob) return AMPCONV_E_BADARG;
  if (B == 0) {
    hipMemsetAsync(loss, 0, sizeof(float), stream);
    hipMemsetAsync(oob, 0, sizeof(int32_t), stream);
    return ampconv_launch_status();
  }
  if (!aff || !neg_term || !workspace) return AMPCONV_E_BADARG;
  if (workspace_bytes < fwd_bytes(B, S)) return AMPCONV_E_WORKSPACE;
  const Split sp = stream_split(B, S, 0);
  const size_t part = pad256((size_t)sp.n * B * sizeof(float));
  float *pm = (float *)workspace, *ps = (float *)((char *)workspace + part), *wl = (float *)((char *)workspace + 2 * part);

  hipMemsetAsync(oob, 0, sizeof(int32_t), stream);
  PairArgs a = base_args(Z, N, D, ldz, scale, neg_weight, kind, exclude_anchor, weight, dtype);
  a.fid = anchor; a.sid = negative; a.nf = (int)B; a.ns = (int)S;
  a.tiles = sp.tiles; a.tiles_per_split = sp.per; a.pm = pm; a.ps = ps;
  if (int rc = launch_pair<0>(a, sp.n, stream)) return rc;

  RowsArgs r = {};
  r.Z = Z; r.ldz = ldz; r.N = N; r.D = D; r.bf16 = a.bf16; r.xent = a.xent; r.splits = sp.n;
  r.anchor = anchor; r.positive = positive; r.negative = negative; r.weight = weight; r.pm = pm; r.ps = ps;
  r.B = (int)B; r.S = (int)S; r.scale = scale; r.neg_weight = neg_weight;
  r.aff = aff; r.neg_term = neg_term; r.wl = wl; r.oob = oob;
  pair_rows_kernel<<<dim3((unsigned)((B * 16 + 255) / 256)), dim3(256), 0, stream>>>(r);
  if (int rc = ampconv_launch_status()) return rc;
  pair_sum_kernel<<<dim3(1), dim3(1024), 0, stream>>>(wl, (int)B, loss);
  return ampconv_launch_status();
}

extern "C" int ampconv_pair_loss_bwd(const void *Z, int64_t N, int D, int64_t ldz, const int64_t *anchor,
                                     const int64_t *positive, int64_t B, const int64_t *negative, int64_t S,
                                     const float *weight, int kind, float scale, float neg_weight, int exclude_anchor,
                                     const float *aff, const float *neg_term, const float *gout, const int32_t *slot_ptr,
                                     const int32_t *slot_idx, void *dZ, int64_t lddz, void *workspace,
                                     size_t workspace_bytes, int dtype, void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!pair_args_ok(Z, N, D, ldz, anchor, positive, B, negative, S, kind, dtype) || lddz < D || (N > 0 && !dZ))
    return AMPCONV_E_BADARG;
  if (N == 0) return AMPCONV_OK;
  const size_t el = dtype == AMPCONV_BF16 ? 2 : 4;
  if (B == 0) {                                        // no pair: zero gradients
    hipMemset2DAsync(dZ, (size_t)lddz * el, 0, (size_t)D * el, (size_t)N, stream);
    return ampconv_launch_status();
  }
  if (!aff || !neg_term || !gout || !slot_ptr || !slot_idx || !workspace) return AMPCONV_E_BADARG;
  const BwdLayout l = bwd_layout(B, S, D);
  if (workspace_bytes < l.bytes) return AMPCONV_E_WORKSPACE;
  float *ra = (float *)workspace, *rp = (float *)((char *)workspace + l.off_p), *rn = (float *)((char *)workspace + l.off_n);

  PairArgs a = base_args(Z, N, D, ldz, scale, neg_weight, kind, exclude_anchor, weight, dtype);
  a.aff = aff; a.neg_term = neg_term; a.g0 = gout;
  PairArgs p1 = a;                                     // anchor tiles: pi N, and the positive role
  p1.fid = anchor; p1.sid = negative; p1.pos = positive; p1.nf = (int)B; p1.ns = (int)S;
  p1.tiles = l.a.tiles; p1.tiles_per_split = l.a.per; p1.out = ra; p1.outp = rp;
  if (int rc = launch_pair<1>(p1, l.a.n, stream)) return rc;
  PairArgs p2 = a;                                     // negative tiles: pi^T A
  p2.fid = negative; p2.sid = anchor; p2.nf = (int)S; p2.ns = (int)B;
  p2.tiles = l.n.tiles; p2.tiles_per_split = l.n.per; p2.out = rn;
  if (int rc = launch_pair<2>(p2, l.n.n, stream)) return rc;

  FoldArgs f = {};
  f.ra = ra; f.rp = rp; f.rn = rn; f.ptr = slot_ptr; f.idx = slot_idx; f.N = N; f.lddz = lddz;
  f.B = (int)B; f.S = (int)S; f.D = D; f.Dq = a.Dq; f.sa = l.a.n; f.sn = l.n.n; f.bf16 = a.bf16; f.dZ = dZ;
  const int64_t threads = N * (a.Dq / 4);
  pair_fold_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream>>>(f);
  return ampconv_launch_status();
}
