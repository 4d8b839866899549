// fp32-grade edge kernels off the FP32 pipe (gfx950): Q/K/V and dObar arrive as TWO fp16 PLANES of the
// power-of-two-scaled fp32 value (written that way by the projection that produces them: proj_gemm.hip, PLANES
// epilogue; scale and split are defined once for both sides, plane16.h), every product is the fp32 sum of three
// v_mfma_f32_16x16x32_f16 partial products
//      a b ~ a_lo b_hi + a_hi b_lo + a_hi b_hi        (dropped: a_lo b_lo <= 2^-22 |a b|)
// softmax, delta and all sums stay fp32, outputs (Obar, dQ, dK, dV) are plain fp32.  Same bytes per element as the
// fp32 path, 5 % of its matrix-pipe cycles per product (3 x 16 instead of 8 x 32 x 4 tiles), and the 16-bit matrix
// pipe runs beside the VALU instead of on it.
//
// Reference arithmetic replaced: torch functional.py:6578 (scale), :6589 (QK^T), :6590 (softmax), :6594 (PV) per edge,
// the mean aggregation of amp_conv.py:11, and their autograd backward.
//
// PLANE FORMAT ("f16x2", include/ampconv.h): the 128-byte slot of the 32 fp32 channels of one (token row, head) holds
//   bytes  0.. 63: hi[c] = fp16(x[c] * 2^e),               c = 0..31
//   bytes 64..127: lo[c] = fp16(x[c] * 2^e - hi[c])
// with ONE exponent e per tensor, e = 14 - floor(log2 bound) for a device-side bound of max |x| (plane_scale: the scaled
// maximum lies below 2^15).  Views keep the strides of the fp32 tensor the planes replace (in 4-byte elements).
//
// Structure = the one-wave-per-unit skeleton of edge_wave16.h with two plane images per tile: one wavefront owns one
// (row, head) unit, streams a
// pair of 20 x 128-byte tiles per edge (five full wave-wide 16-B/lane loads) through registers into private LDS
// images (per plane the swizzled 64-byte-row image of the bf16 kernels, plane16.h: conflict-free ds_write_b128,
// ds_read_b128 and transposed reads), channel-product fragments are one ds_read_b128 per plane, token-product fragments two
// ds_read_b64_tr_b16 per plane, softmax results are split into two fp16 planes in registers and are the B operand of
// the next product as they stand.  dObar arrives DIVIDED by the in-degree of its node (the producing projection's
// epilogue does it), so neither backward pass carries a per-edge weight.  Softmax statistics (optional, as in the fp32
// kernels: 20 log2-sum-exp + 20 delta floats per edge and head, filed at the edge's CSC position by the destination pass):
// with them the source pass's softmax is element-wise -- its three 16-lane reductions per row are a third of its
// vector instructions, and these passes are bound by vector issue and by the clock the chip holds under them.
// This file: the format policy (FmtP), the forward and destination kernels as wrappers of the shared bodies, and the
// source pass, which is this format's own algorithm.
#include "edge_wave16.h"

namespace {
using namespace wave16;       // the skeleton; plane16: plane_scale, split2, frag_sumsq, the swizzled plane image (plane_off, rowfrag, colfrag), TR_*

// HALF (dh = 16, BASELINE config 3's head width): the head's slot is 64 bytes (16 hi, 16 lo); its 16 channels occupy the
// lower half of every 32-channel plane row, the upper half is never written (the images are zeroed once per unit: the
// 32-deep channel contraction is zero-padded) and only channel tile mc = 0 exists.  Half the bytes per (edge, head) at the
// same vector work: these shapes are bound by instruction issue, not by HBM.
// the lo image sits an odd multiple of 64 bytes behind the hi image: the 8 lanes that file one 128-byte row (4 hi
// chunks, 4 lo chunks) then cover all 32 store banks once
constexpr int kLoOff = kPlaneBytes + 64;               // 1344
constexpr int kTileBytes = kLoOff + kPlaneBytes;       // 2624 (a multiple of 16)
constexpr float kPScale = 16384.f;                     // softmax weights (<= 1) are split as P * 2^14
constexpr float kPUnscale = 1.f / 16384.f;
// dS = P (dP - delta), in the units of dP' = dO' V'^T, is split with ONE power-of-two scale per unit from a bound of
// what the unit can see: |dP'_ij| <= |dO'_i| |V'_j| (Cauchy-Schwarz over the 32 channels), |dP - delta| <= 2 max |dP|,
// P <= 1.  The unit's OWN side enters with the largest token-row norm it really has (computed once per unit from its
// hi plane), the streamed side with sqrt(32) x the recorded maximum of its tensor.  (The a-priori worst case --
// 32 channels at 2^15 each -- is 2^17 above typical data: scaled by it, dS sits at 2^-9 and its low plane is a
// subnormal with four bits left.  Measured: dx error 4e-6 of the maximum instead of 8e-7.)
constexpr float kSqrtDh = 5.656854249492381f;
// mask value of the softmaxes: the scores here are in the units of Q' K'^T and meet their scale only inside the
// exponential, so a large finite mask (kNegBig) could be scaled back into range; -inf stays -inf (every column / row
// has at least one finite score: token 0)
constexpr float kMasked = -__builtin_inff();

#define MFMA_F16(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), (c), 0, 0, 0)

// the three partial products of one fp32-grade product, smallest first
__device__ __forceinline__ f32x4 mfma3(const i32x4 &ah, const i32x4 &al, const i32x4 &bh, const i32x4 &bl, f32x4 c) {
  c = MFMA_F16(al, bh, c);
  c = MFMA_F16(ah, bl, c);
  return MFMA_F16(ah, bh, c);
}

// largest token-row norm^2 of a tile given as its two channel-product fragments (lane (n, kg) = 8 channels of the token
// of column n): wave-uniform
__device__ __forceinline__ float tile_max_norm2(const i32x4 &f0, const i32x4 &f1) {
  const float t = fmaxf(groups_sum(frag_sumsq(f0)), groups_sum(frag_sumsq(f1)));
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, row16_max(t))));
}
// scale of dS for a unit whose own side has largest row norm^2 `own2` and whose streamed side is bounded by `other`
// per element (both in plane units): dS * scale < 2^15
__device__ __forceinline__ float ds_scale(float own2, float other) {
  return plane_scale(2.f * __builtin_sqrtf(own2) * (kSqrtDh * other));
}

// C/D registers (already in the split's units, |x| < 2^16) -> the two planes of a token-product fragment: slots 0..3 =
// t0 (tokens 4 g + q), slot 4 = t1_0 (token 16 + g), slots 5..7 zero
__device__ __forceinline__ void cd_frag2(const f32x4 &t0, float t1_0, i32x4 &hi, i32x4 &lo) {
  int h0, l0, h1, l1, h2, l2;
  split2(t0[0], t0[1], h0, l0);
  split2(t0[2], t0[3], h1, l1);
  split2(t1_0, 0.f, h2, l2);
  hi = i32x4{h0, h1, h2, 0};
  lo = i32x4{l0, l1, l2, 0};
}

struct Args {
  ampconv_view_t Q, K, V, dO, O, dK, dV;   // O = forward output / dQ (fp32); Q, K, V, dO: planes
  const int32_t *ptr, *idx;
  const float *bounds;                      // device: {bound of |Q|K|V|, bound of |dObar|: the planes' scales;
                                            //          recorded max |V|, recorded max |dObar|: the scale of dS}
  float *absmax;                            // or null: atomic max of the finite magnitudes written (backward passes)
  // softmax statistics handed from the destination pass to the source pass (kStatsPerUnit floats per (CSC position,
  // head): 20 log2-sum-exp values, then 20 delta values in the units of dP' = dO' V'^T), or null
  const int32_t *spos;                      // CSR position -> CSC position (destination pass)
  float *stats;
  HubArgs hub;
  int64_t n_units;
  int L, H;
};

// output tile store (fp32): C/D layout lane (n = lane & 15, g), reg q -> channel 4 g + q + 16 mc, token of column n of
// tile nt: n / 16 + n (plain map) or, QUARTER (the source pass's own tokens sit on quarter-mapped columns), 16 + (n >> 2)
// for the lanes n % 4 == 0 of tile 1.  Returns the largest finite magnitude stored.
template <bool QUARTER, int MC>
__device__ __forceinline__ float store_tile(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[MC][2],
                                            float scale, int L, int lane) {
  const int g = lane >> 4, n = lane & 15;
  float m = 0.f;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int i = nt == 0 ? n : (QUARTER ? 16 + (n >> 2) : 16 + n);
    if (i < L && (nt == 0 || !QUARTER || (n & 3) == 0)) {
#pragma unroll
      for (int mc = 0; mc < MC; ++mc) {
        const float4 o = make_float4(T[mc][nt][0] * scale, T[mc][nt][1] * scale, T[mc][nt][2] * scale,
                                     T[mc][nt][3] * scale);
        const int64_t off = node * v.node_stride + (int64_t)h * v.head_stride + (int64_t)i * v.row_stride + 4 * g + 16 * mc;
        *reinterpret_cast<float4 *>(reinterpret_cast<float *>(v.ptr) + off) = o;
        m = finite_abs_max(m, o);
      }
    }
  }
  return m;
}

// ---- the format: two fp16 planes (hi at 0, lo at kLoOff) of the scaled value, three products
struct FmtP {
  using Args = ::Args;
  static constexpr int kPlanes = 2, kElemBytes = 4, kLoOff = ::kLoOff, kTileBytes = ::kTileBytes;
  using Frag = wave16::Frag<2>;      // p[0] = hi, p[1] = lo
  // dh = 32: 8 lanes per 128-byte slot row, 5 loads; HALF: 4 lanes per 64-byte slot row (chunks 0, 1 hi; 2, 3 lo), 3 loads.
  // The registers are never touched for HALF: the images are zeroed once per unit instead
  template <bool HALF> using Geom = PairGeom<HALF ? 4 : 8, HALF ? 3 : 5, HALF ? 4 : 8, 2, ::kLoOff>;
  static constexpr bool kHalfZeroLds = true;
  template <bool HALF> static constexpr int mc_tiles() { return HALF ? 1 : 2; }
  // TR_PRE_READ in front of the transposed reads, the split of the softmax results in the shadow of those reads
  static constexpr bool kShadow = true;
  static constexpr float kMasked = ::kMasked, kPMul = kPScale;

  static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) { return mfma3(a.p[0], a.p[1], b.p[0], b.p[1], c); }
  static __device__ __forceinline__ Frag cd_frag(const f32x4 &t0, const f32x4 &t1) {
    Frag f;
    cd_frag2(t0, t1[0], f.p[0], f.p[1]);
    return f;
  }

  // scales: the planes' power-of-two scales are undone in the exponent (uq^2) and at the stores, softmax weights travel
  // as P * kPScale, dS in the unit's own split scale; dObar arrives divided by the in-degree, so 1/deg enters nowhere
  // but the forward mean
  struct Scales {
    float uq, ug, sc;      // 1 / scale of Q|K|V, 1 / scale of dObar (exact: powers of two), log2e / sqrt(dh) / (scale of Q' K'^T)
  };
  template <bool HALF> static constexpr float inv_sqrt_dh() { return HALF ? 0.25f : 0.17677669529663687f; }
  template <bool HALF> static __device__ __forceinline__ Scales scales(const Args &a) {
    const float uq = 1.f / plane_scale(uniform_ld(a.bounds)), ug = 1.f / plane_scale(uniform_ld(a.bounds + 1));
    return Scales{uq, ug, (kLog2e * inv_sqrt_dh<HALF>() * uq) * uq};
  }
  static __device__ __forceinline__ int64_t qrow(const Args &, int64_t r) { return r; }
  static __device__ __forceinline__ float fwd_scale(const Scales &k, float mean) { return kPUnscale * k.uq * mean; }
  // dS scale of this unit: its own dObar rows against the bound of any V row
  static __device__ __forceinline__ float ds_mul(const Args &a, int, const Frag (&gB)[2]) {
    return ds_scale(tile_max_norm2(gB[0].p[0], gB[1].p[0]), uniform_ld(a.bounds + 2) * plane_scale(uniform_ld(a.bounds)));
  }
  // dQ = sum dS K / sqrt(dh): undo the split scale, the scales of dP' (Q|K|V and dObar) and of K'
  template <bool HALF> static __device__ __forceinline__ float dq_scale(const Args &, const Scales &k, float ss, bool hubp) {
    return (((1.f / ss) * k.uq) * k.ug) * k.uq * (hubp ? 1.f : inv_sqrt_dh<HALF>());
  }

  // fp32 (the hub pass's partial tiles are fp32 too); returns the largest finite magnitude stored
  template <bool HALF>
  static __device__ __forceinline__ float store(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[HALF ? 1 : 2][2],
                                                float scale, bool, int L, int lane) {
    return store_tile<false, HALF ? 1 : 2>(v, node, h, T, scale, L, lane);
  }
  template <bool HALF>
  static __device__ __forceinline__ void store_zero(const ampconv_view_t &v, int64_t node, int h, int L, int lane) {
    constexpr int MC = HALF ? 1 : 2;
    f32x4 Z[MC][2];
#pragma unroll
    for (int mc = 0; mc < MC; ++mc) Z[mc][0] = Z[mc][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    store_tile<false, MC>(v, node, h, Z, 0.f, L, lane);
  }
  static __device__ __forceinline__ void record_absmax(const Args &a, float m) {
    if (a.absmax) wave_record_absmax(a.absmax, m);
  }
};

template <bool FULL, bool HALF>
__global__ __launch_bounds__(64 * kWavesPerBlock, 4) void fwd_f16x2(Args a) { fwd_body<FmtP, FULL, HALF>(a); }
template <bool FULL, bool STATS, bool HALF>
__global__ __launch_bounds__(64 * kWavesPerBlock, 3) void bwd_dst_f16x2(Args a) { bwd_dst_body<FmtP, FULL, STATS, HALF>(a); }

// ---------------------------------------------------------------- backward, source pass
// The unit's OWN K / V tiles live in two more LDS images and are re-read per edge (the registers they would occupy are
// the difference between two and three waves per SIMD).  Their tokens sit on the MFMA COLUMNS, tile 1 in the quarter
// map (column n <-> token 16 + (n >> 2): every tail token four times, no row of the 20-row image is read out of
// range); the row softmax masks the replicas, the store takes the lanes n % 4 == 0.
constexpr int kSrcLds = 4 * kTileBytes + 2 * kLmax * 4 + 32;      // four tile images + the edge's statistics (padded to 16)
template <bool FULL, bool STATS, bool HALF>
__global__ __launch_bounds__(64 * kWavesPerBlock, 3) void bwd_src_f16x2(Args a) {
  using G = FmtP::Geom<HALF>;
  constexpr int MC = HALF ? 1 : 2;
  __shared__ __attribute__((aligned(16))) char lds_all[kWavesPerBlock][kSrcLds];
  for_unit<FmtP, HALF>(a, a.dK, &a.dV, [&](const Unit &u) __attribute__((always_inline)) {
    const int lane = u.lane, h = u.h, beg = u.beg, end = u.end;
    const int L = a.L, n = lane & 15;
    char *Qt = lds_all[u.wave], *Gt = Qt + kTileBytes, *Ko = Gt + kTileBytes, *Vo = Ko + kTileBytes;
    const FmtP::Scales k = FmtP::scales<HALF>(a);
    const float ug = k.ug, sc = k.sc;

    if (!FULL || HALF) lds_zero(Qt, 4 * kTileBytes, lane);
    Pair16<G::NLD> qg;
    pair16_load<FULL, G>(qg, slot_ptr<4>(a.K, u.row, h), (unsigned)a.K.row_stride * 4u, slot_ptr<4>(a.V, u.row, h),
                       (unsigned)a.V.row_stride * 4u, L, lane);
    pair16_to_lds<FULL, G, kTileBytes>(Ko, qg, L, lane);
    __builtin_amdgcn_wave_barrier();
    // dS scale of this unit: its own V rows against the bound of any dObar row
    const float ss = ds_scale(tile_max_norm2(rowfrag(Vo, 0, lane), rowfrag(Vo, 1, lane)), uniform_ld(a.bounds + 3) * plane_scale(uniform_ld(a.bounds + 1)));
    f32x4 dKT[MC][2], dVT[MC][2];
#pragma unroll
    for (int mc = 0; mc < MC; ++mc)
      dKT[mc][0] = dKT[mc][1] = dVT[mc][0] = dVT[mc][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    IdxWindow win;
    const unsigned qrb = (unsigned)a.Q.row_stride * 4u, grb = (unsigned)a.dO.row_stride * 4u;
    float *stl = reinterpret_cast<float *>(Vo + kTileBytes);      // the edge's 40 statistics, staged for the row reads
    float sv = 0.f;                                               // lane l < 40: statistic l of the edge in flight
    auto fetch = [&](int p) {
      const int64_t d = idxwin_get<false>(win, a.idx, nullptr, p, end, lane, nullptr);
      pair16_load<FULL, G>(qg, slot_ptr<4>(a.Q, d, h), qrb, slot_ptr<4>(a.dO, d, h), grb, L, lane);
      if (STATS && lane < kStatsPerUnit) sv = a.stats[((int64_t)p * a.H + h) * kStatsPerUnit + lane];
    };
    if (beg < end) {
      idxwin_load<false>(win, a.idx, nullptr, beg, end, lane);
      fetch(beg);
    }
    // own tokens on the columns: tile 0 column n = token n, tile 1 column n = token 16 + (n >> 2), one lane per token
    const bool v0 = FULL || n < L, v1 = (n & 3) == 0 && 16 + (n >> 2) < L;
    for (int p = beg; p < end; ++p) {
      pair16_to_lds<FULL, G, kTileBytes>(Qt, qg, L, lane);
      if (STATS && lane < kStatsPerUnit) stl[lane] = sv;
      if (p + 1 < end) fetch(p + 1);
      __builtin_amdgcn_wave_barrier();

      f32x4 S[2][2], dP[2][2];
      {
        i32x4 kh[2], kl[2], vh[2], vl[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          kh[nt] = rowfrag(Ko, nt, lane);
          kl[nt] = rowfrag(Ko + kLoOff, nt, lane);
          vh[nt] = rowfrag(Vo, nt, lane);
          vl[nt] = rowfrag(Vo + kLoOff, nt, lane);
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const i32x4 ah = rowfrag(Qt, mt, lane), al = rowfrag(Qt + kLoOff, mt, lane);
          const i32x4 bh = rowfrag(Gt, mt, lane), bl = rowfrag(Gt + kLoOff, mt, lane);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) {
            S[mt][nt] = mfma3(ah, al, kh[nt], kl[nt], f32x4{0.f, 0.f, 0.f, 0.f});
            dP[mt][nt] = mfma3(bh, bl, vh[nt], vl[nt], f32x4{0.f, 0.f, 0.f, 0.f});
          }
        }
      }
      // row softmax over the source tokens (columns across the 16 lanes of a DPP row); rows: tile 0 reg q = destination
      // token 4 g + q, tile 1 reg 0 = token 16 + g (quarter map).  After this block S holds P * 2^14 (for dV) and dP holds
      // dS in the unit's split scale.
      if (STATS) {
        // element-wise with the statistics of the destination pass: rows of tile 0 = tokens 4 g .. 4 g + 3, tile 1 reg 0 =
        // token 16 + g
        const int g = lane >> 4;
        const f32x4 l0 = *reinterpret_cast<const f32x4 *>(stl + 4 * g), d0 = *reinterpret_cast<const f32x4 *>(stl + kLmax + 4 * g);
        const float l1 = stl[16 + g], d1 = stl[kLmax + 16 + g];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
          for (int q = 0; q < (mt == 0 ? 4 : 1); ++q) {
            // (rows of tokens >= L have no statistics: their weights are zero, not exp2 of whatever the buffer holds --
            // which the destination pass never wrote and may be a NaN or an infinity, so it is not read into ls / dl)
            const bool vr = FULL || (mt == 0 ? 4 * g + q : 16 + g) < L;
            const float ls = !vr ? 0.f : mt == 0 ? l0[q] : l1, dl = !vr ? 0.f : mt == 0 ? d0[q] : d1;
            const float s0 = (v0 && vr) ? S[mt][0][q] : kMasked, s1 = (v1 && vr) ? S[mt][1][q] : kMasked;
            const float p0 = fast_exp2(fmaf(s0, sc, -ls)), p1 = fast_exp2(fmaf(s1, sc, -ls));
            S[mt][0][q] = p0 * kPScale;
            S[mt][1][q] = p1 * kPScale;
            dP[mt][0][q] = p0 * (dP[mt][0][q] - dl) * ss;
            dP[mt][1][q] = p1 * (dP[mt][1][q] - dl) * ss;
          }
        }
      } else {
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int q = 0; q < (mt == 0 ? 4 : 1); ++q) {
          const float s0 = v0 ? S[mt][0][q] : kMasked, s1 = v1 ? S[mt][1][q] : kMasked;
          const float m = row16_max(fmaxf(s0, s1));
          float p0 = fast_exp2((s0 - m) * sc), p1 = fast_exp2((s1 - m) * sc);
          const float rinv = fast_rcp(row16_sum(p0 + p1));
          p0 *= rinv;
          p1 *= rinv;
          const float delta = row16_sum(fmaf(p0, dP[mt][0][q], p1 * dP[mt][1][q]));
          S[mt][0][q] = p0 * kPScale;
          S[mt][1][q] = p1 * kPScale;
          dP[mt][0][q] = p0 * (dP[mt][0][q] - delta) * ss;
          dP[mt][1][q] = p1 * (dP[mt][1][q] - delta) * ss;
        }
      }
      }
      {
        i32x4 ph[2], pl[2], gh[MC], gl[MC];
        TR_PRE_READ();
#pragma unroll
        for (int mc = 0; mc < MC; ++mc) {
          gh[mc] = colfrag(Gt, mc, lane);
          gl[mc] = colfrag(Gt + kLoOff, mc, lane);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) cd_frag2(S[0][nt], S[1][nt][0], ph[nt], pl[nt]);
        TR_FRAG_FENCE();
#pragma unroll
        for (int mc = 0; mc < MC; ++mc)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) dVT[mc][nt] = mfma3(gh[mc], gl[mc], ph[nt], pl[nt], dVT[mc][nt]);
        TR_WAR_GUARD();
      }
      {
        i32x4 sh[2], sl[2], qh[MC], ql[MC];
#pragma unroll
        for (int mc = 0; mc < MC; ++mc) {
          qh[mc] = colfrag(Qt, mc, lane);
          ql[mc] = colfrag(Qt + kLoOff, mc, lane);
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) cd_frag2(dP[0][nt], dP[1][nt][0], sh[nt], sl[nt]);
        TR_FRAG_FENCE();
#pragma unroll
        for (int mc = 0; mc < MC; ++mc)
#pragma unroll
          for (int nt = 0; nt < 2; ++nt) dKT[mc][nt] = mfma3(qh[mc], ql[mc], sh[nt], sl[nt], dKT[mc][nt]);
      }
      __builtin_amdgcn_wave_barrier();
    }
    // dK = sum dS^T Q / sqrt(dh), dV = sum P^T dObar (1/deg is inside dObar); the hub pass leaves 1/sqrt(dh) to the combine
    const bool hubp = a.hub.mode == 2;
    float m = store_tile<true, MC>(a.dK, u.onode, h, dKT, FmtP::dq_scale<HALF>(a, k, ss, hubp), L, lane);
    m = fmaxf(m, store_tile<true, MC>(a.dV, u.onode, h, dVT, kPUnscale * ug, L, lane));
    FmtP::record_absmax(a, m);
  });
}

typedef void (*EdgeKernel)(Args);
// kernels[stats][half][full]
int launch_fwd(Args &a, int L, bool half, hipStream_t st) {
  static const EdgeKernel k[2][2] = WAVE16_KERNELS(fwd_f16x2);
  return launch_wave16(k, a, L, half, st);
}
int launch_dst(Args &a, int L, bool half, hipStream_t st) {
  static const EdgeKernel k[2][2][2] = {WAVE16_KERNELS_STATS(bwd_dst_f16x2, false), WAVE16_KERNELS_STATS(bwd_dst_f16x2, true)};
  return launch_wave16(k[a.stats != nullptr], a, L, half, st);
}
int launch_src(Args &a, int L, bool half, hipStream_t st) {
  static const EdgeKernel k[2][2][2] = {WAVE16_KERNELS_STATS(bwd_src_f16x2, false), WAVE16_KERNELS_STATS(bwd_src_f16x2, true)};
  return launch_wave16(k[a.stats != nullptr], a, L, half, st);
}

// planes: 16-byte aligned, the head's dh channels one 4 dh-byte slot, rows a whole number of 16-byte pieces apart
inline bool plane_view_ok(const ampconv_view_t &v, int dh) {
  return v.ptr && ((uintptr_t)v.ptr % 16 == 0) && v.head_stride == dh && (v.node_stride % 4 == 0) && (v.row_stride % 4 == 0);
}
inline bool f32_view_ok(const ampconv_view_t &v) {
  return v.ptr && ((uintptr_t)v.ptr % 16 == 0) && (v.head_stride % 4 == 0) && (v.node_stride % 4 == 0) && (v.row_stride % 4 == 0);
}
int check_shape(int64_t n, int L, int D, int H, const float *bounds) {
  if (L <= 0 || D <= 0 || H <= 0 || D % H != 0 || n < 0 || !bounds) return AMPCONV_E_BADARG;
  if (L > kLmax || (D / H != DH && D / H != DH / 2)) return AMPCONV_E_DTYPE;
  return AMPCONV_OK;
}

}  // namespace

extern "C" int ampconv_planes_supported(int L, int D, int H) {
  return L >= 1 && L <= kLmax && H > 0 && D % H == 0 && (D / H == DH || D / H == DH / 2);
}

extern "C" int ampconv_fwd_edge_planes(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, const int32_t *rowptr,
                                       const int32_t *col, int64_t n_rows, int L, int D, int H, ampconv_view_t O,
                                       const void *hub_plan, int64_t hub_chunks, void *hub_ws, const float *bounds,
                                       void *stream) {
  if (int rc = check_shape(n_rows, L, D, H, bounds)) return rc;
  if (n_rows == 0) return AMPCONV_OK;
  if (!plane_view_ok(Q, D / H) || !plane_view_ok(K, D / H) || !plane_view_ok(V, D / H) || !f32_view_ok(O) || !rowptr) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  Args a{};
  a.Q = Q; a.K = K; a.V = V;
  a.ptr = rowptr; a.idx = col; a.bounds = bounds; a.L = L; a.H = H;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *) {
    a.hub = hub; a.n_units = n * H; a.O = o[0];
    return launch_fwd(a, L, D / H == DH / 2, st);
  };
  return run_edge_pass(run, n_rows, {O}, hub_plan, hub_chunks, hub_ws, L, D, H, rowptr, {1.f}, 0, nullptr, st);
}

extern "C" int ampconv_bwd_edge_dst_planes(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                                           const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D, int H,
                                           ampconv_view_t dQ, const void *hub_plan, int64_t hub_chunks, void *hub_ws,
                                           const float *bounds, const int32_t *spos, float *stats, float *out_absmax,
                                           void *stream) {
  if (int rc = check_shape(n_rows, L, D, H, bounds)) return rc;
  if (stats && (!spos || (uintptr_t)stats % 16 != 0)) return AMPCONV_E_BADARG;
  if (n_rows == 0) return AMPCONV_OK;
  if (!plane_view_ok(Q, D / H) || !plane_view_ok(K, D / H) || !plane_view_ok(V, D / H) || !plane_view_ok(dObar, D / H) || !f32_view_ok(dQ) || !rowptr)
    return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  Args a{};
  a.Q = Q; a.K = K; a.V = V; a.dO = dObar;
  a.ptr = rowptr; a.idx = col; a.bounds = bounds; a.L = L; a.H = H;
  a.spos = spos; a.stats = stats;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *absmax) {
    a.hub = hub; a.n_units = n * H; a.O = o[0]; a.absmax = absmax;
    return launch_dst(a, L, D / H == DH / 2, st);
  };
  return run_edge_pass(run, n_rows, {dQ}, hub_plan, hub_chunks, hub_ws, L, D, H, nullptr,
                       {1.f / sqrtf((float)(D / H))}, 0, out_absmax, st);
}

extern "C" int ampconv_bwd_edge_src_planes(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                                           const int32_t *cscptr, const int32_t *crow, int64_t n_src, int L, int D, int H,
                                           ampconv_view_t dK, ampconv_view_t dV, const void *hub_plan, int64_t hub_chunks,
                                           void *hub_ws, const float *bounds, const float *stats, float *out_absmax,
                                           void *stream) {
  if (int rc = check_shape(n_src, L, D, H, bounds)) return rc;
  if (stats && (uintptr_t)stats % 16 != 0) return AMPCONV_E_BADARG;
  if (n_src == 0) return AMPCONV_OK;
  if (!plane_view_ok(Q, D / H) || !plane_view_ok(K, D / H) || !plane_view_ok(V, D / H) || !plane_view_ok(dObar, D / H) || !f32_view_ok(dK) ||
      !f32_view_ok(dV) || !cscptr)
    return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  Args a{};
  a.Q = Q; a.K = K; a.V = V; a.dO = dObar;
  a.ptr = cscptr; a.idx = crow; a.bounds = bounds; a.L = L; a.H = H;
  a.stats = const_cast<float *>(stats);
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *absmax) {
    a.hub = hub; a.n_units = n * H; a.dK = o[0]; a.dV = o[1]; a.absmax = absmax;
    return launch_src(a, L, D / H == DH / 2, st);
  };
  return run_edge_pass(run, n_src, {dK, dV}, hub_plan, hub_chunks, hub_ws, L, D, H, nullptr,
                       {1.f / sqrtf((float)(D / H)), 1.f}, 0, out_absmax, st);
}
