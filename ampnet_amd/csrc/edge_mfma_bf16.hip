// bf16-storage edge kernels for gfx950 (BASELINE config 5): Q/K/V/O and the gradients live in HBM
// as bf16, every product runs on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, softmax and all
// sums are fp32.  L <= 20, dh = 32 (or dh = 16 as a half-filled dh = 32 tile: `HALF`, see below).  Half the HBM bytes
// of the fp32 path and 1/16 of its MFMA
// cycles per product; the reference itself is fp32 only, so this is an extension checked against
// the fp32 oracle at bf16 tolerance (tests/test_gpu_parity.py::test_bf16_storage).
//
// Structure = the one-wave-per-unit skeleton of edge_wave16.h with ONE plane: a streamed 20 x 32 bf16 tile (64-byte token
// rows, 16 rows per wave-wide 16-B/lane load) goes straight into the swizzled LDS plane image (plane16.h);
// channel-product fragments are one ds_read_b128, token-product fragments two
// ds_read_b64_tr_b16 (hardware transpose), softmax results are converted to bf16 in registers
// and are the B operand of the next product as they stand (tokens 16..19 sit in lane group 0).
// Scales that the fp32 kernels fold into operands (log2e/sqrt(dh), 1/deg) are applied to the fp32
// accumulators instead.  Long segments (hubs) reduce into fp32 partial tiles (hub.hip).
// This file: the format policy (FmtB), the forward and destination kernels as wrappers of the shared bodies, and the
// source pass, which is this format's own algorithm.
#include "edge_wave16.h"

namespace {
using namespace wave16;       // the skeleton; plane16: conversions, the swizzled plane image (plane_off, rowfrag, colfrag), TR_FRAG_FENCE

typedef unsigned short bf16_t;

// HALF (dh = 16, BASELINE config 3's head width): the head's 16 channels occupy the lower half of a 32-channel tile;
// the upper half is never loaded (zero operands: the 32-deep channel contraction is zero-padded), its output tile
// (mc = 1) is never stored (the source still names its products; the compiler drops them where it sees them dead).
// Functional, not tuned: half of every load and MFMA is padding.

#define MFMA_BF16(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), (c), 0, 0, 0)

struct Args {
  ampconv_view_t Q, K, V, dO, O, dK, dV;   // O = forward output / dQ
  const int32_t *ptr, *idx, *qidx;
  const float *cinv;
  HubArgs hub;
  int64_t n_units;
  int L, H;
  float qscale, oscale;
};

// output tile store: C/D layout lane (i' = lane & 15, g), reg q -> channel 4g + q + 16 mc, token
// i' + 16 nt; `to_f32` = hub pass (fp32 partial tiles)
template <bool HALF>
__device__ __forceinline__ void store_tile(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[2][2],
                                           float scale, bool to_f32, int L, int lane) {
  const int g = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int i = (lane & 15) + 16 * nt;
    if (i < L) {
#pragma unroll
      for (int mc = 0; mc < (HALF ? 1 : 2); ++mc) {
        const float a = T[mc][nt][0] * scale, b = T[mc][nt][1] * scale, c = T[mc][nt][2] * scale,
                    d = T[mc][nt][3] * scale;
        const int64_t off = node * v.node_stride + (int64_t)h * v.head_stride + (int64_t)i * v.row_stride +
                            4 * g + 16 * mc;
        if (to_f32)
          *reinterpret_cast<float4 *>(reinterpret_cast<float *>(v.ptr) + off) = make_float4(a, b, c, d);
        else
          *reinterpret_cast<i32x2 *>(reinterpret_cast<bf16_t *>(v.ptr) + off) =
              i32x2{cvt_pk_bf16(a, b), cvt_pk_bf16(c, d)};
      }
    }
  }
}

// ---- the format: one bf16 plane as it lies in memory, one product
struct FmtB {
  using Args = ::Args;
  static constexpr int kPlanes = 1, kElemBytes = 2, kLoOff = 0, kTileBytes = kPlaneBytes;
  using Frag = wave16::Frag<1>;
  // 4 lanes per 64-byte row, 3 loads; HALF: chunks 2, 3 of a row do not exist -- zero in the lane's registers at load
  // time, so the images need no zero fill for it
  template <bool HALF> using Geom = PairGeom<4, 3, HALF ? 2 : 4, 1>;
  static constexpr bool kHalfZeroLds = false;
  template <bool HALF> static constexpr int mc_tiles() { return 2; }      // (HALF: tile 1 is computed on zeros, not stored)
  static constexpr bool kShadow = false;
  static constexpr float kMasked = kNegBig, kPMul = 1.f;

  static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) { return MFMA_BF16(a.p[0], b.p[0], c); }
  // C/D registers -> token-product fragment (t1[1..3] are zero: only reg 0 of tile 1 is a token)
  static __device__ __forceinline__ Frag cd_frag(const f32x4 &t0, const f32x4 &t1) {
    return Frag{{i32x4{cvt_pk_bf16(t0[0], t0[1]), cvt_pk_bf16(t0[2], t0[3]), cvt_pk_bf16(t1[0], t1[1]),
                       cvt_pk_bf16(t1[2], t1[3])}}};
  }

  // scales: qscale = log2e / sqrt(dh) in the exponent, 1/deg on the forward accumulator at the store and on dS in the
  // destination pass, oscale = 1 / sqrt(dh) at the dQ store
  struct Scales {
    float sc;
  };
  template <bool HALF> static __device__ __forceinline__ Scales scales(const Args &a) { return Scales{a.qscale}; }
  static __device__ __forceinline__ int64_t qrow(const Args &a, int64_t r) { return a.qidx ? uniform_ld(a.qidx + r) : r; }
  static __device__ __forceinline__ float fwd_scale(const Scales &, float mean) { return mean; }
  static __device__ __forceinline__ float ds_mul(const Args &, int deg, const Frag (&)[2]) {
    return deg > 0 ? 1.f / (float)deg : 0.f;      // dO is the gradient of the MEAN
  }
  template <bool HALF> static __device__ __forceinline__ float dq_scale(const Args &a, const Scales &, float, bool hubp) {
    return hubp ? 1.f : a.oscale;
  }

  // bf16, or fp32 partial tiles in the hub pass
  template <bool HALF>
  static __device__ __forceinline__ float store(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[2][2],
                                                float scale, bool hubp, int L, int lane) {
    store_tile<HALF>(v, node, h, T, scale, hubp, L, lane);
    return 0.f;
  }
  template <bool HALF>
  static __device__ __forceinline__ void store_zero(const ampconv_view_t &v, int64_t node, int h, int L, int lane) {
    f32x4 Z[2][2];
#pragma unroll
    for (int mc = 0; mc < 2; ++mc) Z[mc][0] = Z[mc][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    store_tile<HALF>(v, node, h, Z, 0.f, false, L, lane);
  }
  static __device__ __forceinline__ void record_absmax(const Args &, float) {}
};

template <bool FULL, bool HALF>
__global__ __launch_bounds__(64 * kWavesPerBlock) void fwd_bf16(Args a) { fwd_body<FmtB, FULL, HALF>(a); }
template <bool FULL, bool HALF>
__global__ __launch_bounds__(64 * kWavesPerBlock) void bwd_dst_bf16(Args a) { bwd_dst_body<FmtB, FULL, false, HALF>(a); }

// ---------------------------------------------------------------- backward, source pass (transposing)
// The source pass needs two different axes of the 20 x 20 score tile: the softmax (and delta) sum over the SOURCE tokens
// j, the products dV = P^T dO, dK = dS^T Q sum over the DESTINATION tokens i.  Kept as S[i][j] (i in the C/D registers:
// ready as the B operand of the products) the softmax costs three 16-lane DPP reductions per row -- ~200 of ~260 vector
// instructions per (edge, head) in a pass bound by vector issue (profiles/r04_sq_counters.md: VALU active 0.82).  This
// kernel computes the tile as S^T[j][i] -- own tokens on the MFMA
// rows, as the forward and destination passes do: the softmax is in-lane plus two cross-group swaps per column -- and
// turns P^T, dS^T round through a wave-private LDS image: each lane files its column as 8 + 2 bytes of row i, the B
// fragments come back by ds_read_b64_tr_b16 with the k index (i) contiguous, and the A fragments (dO^T, Q^T) are cut from
// 32-row images with the same contiguous k map.  Rows 20..31 of every image are zero (written once per unit).
constexpr int kTile32 = 32 * kRowBytes;       // 2 KiB: 32 token rows

// channel-product fragment with the PLAIN column map (column n of tile 1 = token 16 + n; rows 20..31 of the image are zero)
__device__ __forceinline__ i32x4 rowfrag_plain(const char *tile, int nt, int lane) {
  const int n = lane & 15, kg = lane >> 4;
  return *reinterpret_cast<const i32x4 *>(tile + plane_off(16 * nt + n, kg));
}
// token-product fragment with the k index contiguous: slots 0..7 of lane group kg = token rows 8 kg .. 8 kg + 7 of a
// 32-row image, 16-column block `blk` (channels of tile mc, or the source tokens of tile nt in a transposed image)
__device__ __forceinline__ i32x4 colfrag32(const char *tile, int blk, int lane) {
  const int q = (lane >> 2) & 3, pp = lane & 3, kg = lane >> 4;
  const int ch = 2 * blk + (pp >> 1), half = (pp & 1) << 3;
  return tr_frag(tile + plane_off(8 * kg + q, ch) + half, tile + plane_off(8 * kg + 4 + q, ch) + half);
}
// a lane's column of a C/D tile pair (t0[q] = own token 4 g + q, t1_0 = own token 16 + g) -> row i of the transposed image
__device__ __forceinline__ void file_column(char *img, int i, const f32x4 &t0, float t1_0, int g) {
  *reinterpret_cast<i32x2 *>(img + plane_off(i, g >> 1) + 8 * (g & 1)) = i32x2{cvt_pk_bf16(t0[0], t0[1]), cvt_pk_bf16(t0[2], t0[3])};
  *reinterpret_cast<unsigned short *>(img + plane_off(i, 2) + 2 * g) = (unsigned short)cvt_pk_bf16(t1_0, 0.f);
}

template <bool FULL, bool HALF>
__global__ __launch_bounds__(64 * kWavesPerBlock) void bwd_src_bf16_tr(Args a) {
  using G = FmtB::Geom<HALF>;
  __shared__ __attribute__((aligned(16))) char lds_all[kWavesPerBlock][4 * kTile32];
  for_unit<FmtB, HALF>(a, a.dK, &a.dV, [&](const Unit &u) __attribute__((always_inline)) {
    const int lane = u.lane, h = u.h, beg = u.beg, end = u.end;
    const int L = a.L, n = lane & 15, g = lane >> 4;
    char *Qt = lds_all[u.wave], *Gt = Qt + kTile32, *Pi = Gt + kTile32, *Si = Pi + kTile32;

    i32x4 kA[2], vA[2];      // own side on the MFMA rows (quarter map)
    {
      const char *kb = slot_ptr<2>(a.K, u.row, h), *vb = slot_ptr<2>(a.V, u.row, h);
      const unsigned krb = (unsigned)a.K.row_stride * 2u, vrb = (unsigned)a.V.row_stride * 2u;
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        kA[mt] = frag_global<1, HALF, true>(kb, krb, mt, L, lane).p[0];
        vA[mt] = frag_global<1, HALF, true>(vb, vrb, mt, L, lane).p[0];
      }
    }
    // all four images zero once: rows >= L (>= 20) of the streamed tiles and of the transposed images are never written
    lds_zero(Qt, 4 * kTile32, lane);
    f32x4 dKT[2][2], dVT[2][2];
#pragma unroll
    for (int mc = 0; mc < 2; ++mc)
      dKT[mc][0] = dKT[mc][1] = dVT[mc][0] = dVT[mc][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    Pair16<G::NLD> qg;
    float inv = 0.f, inv_next = 0.f;
    IdxWindow win;
    const unsigned qrb = (unsigned)a.Q.row_stride * 2u, grb = (unsigned)a.dO.row_stride * 2u;
    auto fetch = [&](int p, float &w) {
      const int64_t d = idxwin_get<true>(win, a.idx, a.cinv, p, end, lane, &w);
      pair16_load<FULL, G>(qg, slot_ptr<2>(a.Q, d, h), qrb, slot_ptr<2>(a.dO, d, h), grb, L, lane);
    };
    if (beg < end) {
      idxwin_load<true>(win, a.idx, a.cinv, beg, end, lane);
      fetch(beg, inv_next);
    }
    for (int p = beg; p < end; ++p) {
      pair16_to_lds<FULL, G, kTile32>(Qt, qg, L, lane);
      inv = inv_next;
      if (p + 1 < end) fetch(p + 1, inv_next);
      __builtin_amdgcn_wave_barrier();

      // S^T = K Q^T and dP^T = V dO^T: own source tokens on the rows (quarter map), destination tokens on the columns
      f32x4 S[2][2], dP[2][2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const i32x4 qB = rowfrag_plain(Qt, nt, lane), gB = rowfrag_plain(Gt, nt, lane);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          S[mt][nt] = MFMA_BF16(kA[mt], qB, (f32x4{0.f, 0.f, 0.f, 0.f}));
          dP[mt][nt] = MFMA_BF16(vA[mt], gB, (f32x4{0.f, 0.f, 0.f, 0.f}));
        }
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        column_softmax<FULL>(S[0][nt], S[1][nt], a.qscale, 1.f, kNegBig, L, g);        // P^T; tile-1 regs 1..3 come out 0
        float part = S[1][nt][0] * dP[1][nt][0];
#pragma unroll
        for (int q = 0; q < 4; ++q) part = fmaf(S[0][nt][q], dP[0][nt][q], part);
        const float delta = groups_sum(part);
#pragma unroll
        for (int q = 0; q < 4; ++q) {                                     // dS^T and P^T, both with the edge's 1 / in-degree
          dP[0][nt][q] = S[0][nt][q] * (dP[0][nt][q] - delta) * inv;
          S[0][nt][q] *= inv;
        }
        dP[1][nt][0] = S[1][nt][0] * (dP[1][nt][0] - delta) * inv;
        S[1][nt][0] *= inv;
        // column i = 16 nt + n of the tile pair -> row i of the transposed images (tile 1: destination tokens 16..19 only)
        const int i = 16 * nt + n;
        if (i < kLmax && (FULL || i < L)) {
          file_column(Pi, i, S[0][nt], S[1][nt][0], g);
          file_column(Si, i, dP[0][nt], dP[1][nt][0], g);
        }
      }
      __builtin_amdgcn_wave_barrier();
      i32x4 pB[2], sB[2], gC[2], qC[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        pB[nt] = colfrag32(Pi, nt, lane);
        sB[nt] = colfrag32(Si, nt, lane);
      }
#pragma unroll
      for (int mc = 0; mc < (HALF ? 1 : 2); ++mc) {
        gC[mc] = colfrag32(Gt, mc, lane);
        qC[mc] = colfrag32(Qt, mc, lane);
      }
      TR_FRAG_FENCE();
#pragma unroll
      for (int mc = 0; mc < (HALF ? 1 : 2); ++mc) {
        dVT[mc][0] = MFMA_BF16(gC[mc], pB[0], dVT[mc][0]);
        dVT[mc][1] = MFMA_BF16(gC[mc], pB[1], dVT[mc][1]);
        dKT[mc][0] = MFMA_BF16(qC[mc], sB[0], dKT[mc][0]);
        dKT[mc][1] = MFMA_BF16(qC[mc], sB[1], dKT[mc][1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop 7" ::: "memory");       // (the next edge's reads do not redefine fragment registers right behind these MFMAs)
      __builtin_amdgcn_wave_barrier();
    }
    const bool hubp = a.hub.mode == 2;
    store_tile<HALF>(a.dK, u.onode, h, dKT, hubp ? 1.f : a.oscale, hubp, L, lane);
    store_tile<HALF>(a.dV, u.onode, h, dVT, 1.f, hubp, L, lane);
  });
}

typedef void (*EdgeKernel)(Args);
int launch(Args &a, int L, int D, int H, EdgeKernel const (&kernels)[2][2], hipStream_t stream) {
  const int dh = D / H;
  if (dh != DH && dh != DH / 2) return AMPCONV_E_BADARG;
  a.qscale = kLog2e / sqrtf((float)dh);
  a.oscale = 1.f / sqrtf((float)dh);
  return launch_wave16(kernels, a, L, dh == DH / 2, stream);
}

inline bool aligned16h(const ampconv_view_t &v) {
  return ((uintptr_t)v.ptr % 16 == 0) && (v.node_stride % 8 == 0) && (v.row_stride % 8 == 0) &&
         (v.head_stride % 8 == 0);
}

}  // namespace

bool ampconv_bf16_supported(int L, int D, int H, const ampconv_view_t *views, int n) {
  if (!(L >= 1 && L <= kLmax && (D / H == DH || D / H == DH / 2) && D % H == 0)) return false;
  for (int i = 0; i < n; ++i)
    if (!aligned16h(views[i])) return false;
  return true;
}

int ampconv_fwd_edge_bf16(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, const int32_t *rowptr,
                          const int32_t *col, const int32_t *qidx, int64_t n_rows, int L, int D, int H,
                          ampconv_view_t O, HubArgs hub, hipStream_t stream) {
  Args a{};
  a.Q = Q; a.K = K; a.V = V; a.O = O;
  a.ptr = rowptr; a.idx = col; a.qidx = qidx; a.hub = hub;
  a.n_units = n_rows * H; a.L = L; a.H = H;
  static const EdgeKernel kernels[2][2] = WAVE16_KERNELS(fwd_bf16);
  return launch(a, L, D, H, kernels, stream);
}

int ampconv_bwd_edge_dst_bf16(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dO,
                              const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D,
                              int H, ampconv_view_t dQ, HubArgs hub, hipStream_t stream) {
  Args a{};
  a.Q = Q; a.K = K; a.V = V; a.dO = dO; a.O = dQ;
  a.ptr = rowptr; a.idx = col; a.hub = hub;
  a.n_units = n_rows * H; a.L = L; a.H = H;
  static const EdgeKernel kernels[2][2] = WAVE16_KERNELS(bwd_dst_bf16);
  return launch(a, L, D, H, kernels, stream);
}

int ampconv_bwd_edge_src_bf16(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dO,
                              const int32_t *cscptr, const int32_t *crow, const float *cinv,
                              int64_t n_src, int L, int D, int H, ampconv_view_t dK, ampconv_view_t dV,
                              HubArgs hub, hipStream_t stream) {
  Args a{};
  a.Q = Q; a.K = K; a.V = V; a.dO = dO; a.dK = dK; a.dV = dV;
  a.ptr = cscptr; a.idx = crow; a.cinv = cinv; a.hub = hub;
  a.n_units = n_src * H; a.L = L; a.H = H;
  static const EdgeKernel kernels[2][2] = WAVE16_KERNELS(bwd_src_bf16_tr);
  return launch(a, L, D, H, kernels, stream);
}
