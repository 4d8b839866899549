// The one-wave-per-unit edge kernels on the 16-bit matrix pipe, once: what edge_mfma_bf16.hip (bf16 storage, one plane)
// and edge_mfma_f16x2.hip (two fp16 planes of the scaled fp32 value) share.  One wavefront owns one (row, head) unit,
// streams a pair of 20-token tiles per edge through registers into private swizzled LDS images (plane16.h), reads
// channel-product fragments with ds_read_b128 and token-product fragments with ds_read_b64_tr_b16, and hands softmax
// results on as the B operand of the next product in registers.  L <= 20, dh = 32, or dh = 16 as a half-filled tile (HALF).
//
// Written once here: the unit prologue, the staging of a tile pair, the own-side fragments, the LDS zero fill, the
// column softmax, the forward and destination-pass bodies, the launch table.  The two source passes are different
// algorithms and live in their files, on the same helpers.
//
// A format policy `Fmt` names what really differs (each file defines its own, next to the reasons):
//   Args, Frag (kPlanes x i32x4), kPlanes, kElemBytes, kTileBytes, Geom<HALF>        storage and LDS image
//   mc_tiles<HALF>(), kHalfZeroLds                                                  how a half-filled tile is padded
//   mma, cd_frag, kShadow                                                           the product, C/D tile -> B operand
//   kMasked, kPMul, Scales, scales, fwd_scale, ds_mul, dq_scale, qrow               where scales enter
//   store, store_zero, record_absmax                                                output format
#pragma once
#include "plane16.h"

namespace wave16 {
using namespace plane16;

constexpr int kWavesPerBlock = 4;
constexpr int DH = 32;
constexpr int kRowBytes = DH * 2;                 // one plane of a token row
constexpr int kPlaneBytes = kLmax * kRowBytes;    // 1280: one plane image

template <int P>
struct Frag {
  i32x4 p[P];
};

// ---- unit prologue: lane, wave-uniform wave (unit, row, head and tile bases live in SGPRs), the unit's row, head and
// edge range, then `body(unit)` -- unless there is nothing to do: no such unit, a row left to the hub pass, or a unit
// without edges, whose output rows are zero and stored here: nothing of its own side needs to be read (R-MAT graphs: half
// of the units of cfg5's main launch).  (The pass is the callee, not code behind a returned flag: the compiler then still
// merges the zero-tile stores with the pass's final stores, as it did when every kernel carried these lines itself.)
struct Unit {
  int lane, wave;
  int64_t row, onode;
  int h, beg, end, deg;
};
template <class Fmt, bool HALF, class Body>
__device__ __forceinline__ void for_unit(const typename Fmt::Args &a, const ampconv_view_t &out0, const ampconv_view_t *out1,
                                         const Body &body) {
  Unit u;
  u.lane = threadIdx.x & 63;
  u.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t unit = (int64_t)blockIdx.x * kWavesPerBlock + u.wave;
  if (unit >= a.n_units) return;
  if (!map_unit(a.hub, a.ptr, unit, a.n_units, a.H, u.row, u.onode, u.h, u.beg, u.end, u.deg)) return;
  if (u.beg >= u.end && a.hub.mode != 2) {
    Fmt::template store_zero<HALF>(out0, u.onode, u.h, a.L, u.lane);
    if (out1) Fmt::template store_zero<HALF>(*out1, u.onode, u.h, a.L, u.lane);
    return;
  }
  body(u);
}

// a wave-uniform scalar that no kernel of the launch writes (operand bounds, a row of the query subset), read behind the
// prologue: through the constant address space, so that it stays a scalar load whatever path the compiler finds from the
// prologue's zero-tile stores to it (behind such a path a plain load of a uniform address becomes a vector load)
template <class T>
__device__ __forceinline__ T uniform_ld(const T *p) {
  return *(const __attribute__((address_space(4))) T *)p;
}

// byte address of the row-0 slot of (node n, head h); EB = bytes per view element
template <int EB>
__device__ __forceinline__ const char *slot_ptr(const ampconv_view_t &v, int64_t n, int h) {
  return reinterpret_cast<const char *>(v.ptr) + EB * (n * v.node_stride + (int64_t)h * v.head_stride);
}

// ---- streamed tile pair.  Geometry: LPR lanes file one slot row in 16-byte chunks, of which the row really has CHUNKS
// (fewer: the others are zero in the lane's registers, never loaded), lane (r = lane / LPR, q = lane % LPR) owns chunk q
// of pair-rows r + (64 / LPR) i, i < NLD; pair-rows 0..19 = tile A, 20..39 = tile B.  Chunk q goes to plane image
// q / (LPR / PLANES) (LO_OFF bytes apart), plane_off chunk q % (LPR / PLANES).
//      bf16, dh 32 : <4, 3, 4, 1>      bf16, HALF   : <4, 3, 2, 1>
//      planes, 32  : <8, 5, 8, 2>      planes, HALF : <4, 3, 4, 2>   (chunks 0, 1 hi; 2, 3 lo)
template <int LPR_, int NLD_, int CHUNKS_, int PLANES_, int LO_OFF_ = 0>
struct PairGeom {
  static constexpr int LPR = LPR_, RPL = 64 / LPR_, NLD = NLD_, CHUNKS = CHUNKS_, CPP = LPR_ / PLANES_, LO_OFF = LO_OFF_;
};
template <int N>
struct Pair16 {
  i32x4 v[N];
};

// strides in bytes
template <bool FULL, class G>
__device__ __forceinline__ void pair16_load(Pair16<G::NLD> &t, const char *baseA, unsigned strideA, const char *baseB,
                                          unsigned strideB, int L, int lane) {
  const int r = lane / G::LPR, q = lane % G::LPR;
#pragma unroll
  for (int i = 0; i < G::NLD; ++i) {
    const int R = r + G::RPL * i;
    const bool isB = R >= kLmax;
    const int j = isB ? R - kLmax : R;
    const bool valid = (R < 2 * kLmax) && (FULL || j < L) && (G::CHUNKS == G::LPR || q < G::CHUNKS);
    if (G::CHUNKS < G::LPR) t.v[i] = i32x4{0, 0, 0, 0};
    // per-lane part as a 32-bit byte offset on top of a tile base that is uniform per edge (base stays in SGPRs)
    const unsigned off = (unsigned)j * (isB ? strideB : strideA) + 16u * (unsigned)q;
    const char *p = (isB ? baseB : baseA) + off;
    if (valid) t.v[i] = *reinterpret_cast<const i32x4 *>(p);
  }
}

// TILE = byte stride from tile A's images to tile B's
template <bool FULL, class G, int TILE>
__device__ __forceinline__ void pair16_to_lds(char *tileA, const Pair16<G::NLD> &t, int L, int lane) {
  const int r = lane / G::LPR, q = lane % G::LPR;
#pragma unroll
  for (int i = 0; i < G::NLD; ++i) {
    const int R = r + G::RPL * i;
    const bool isB = R >= kLmax;
    const int j = isB ? R - kLmax : R;
    if ((R < 2 * kLmax) && (FULL || j < L))
      *reinterpret_cast<i32x4 *>(tileA + (isB ? TILE : 0) + (G::CPP < G::LPR && q >= G::CPP ? G::LO_OFF : 0) +
                                 plane_off(j, G::CPP < G::LPR ? q % G::CPP : q)) = t.v[i];
  }
}

__device__ __forceinline__ void lds_zero(char *p, int bytes, int lane) {
  int *z = reinterpret_cast<int *>(p);
  for (int i = lane; i < bytes / 4; i += AMPCONV_WAVE) z[i] = 0;
}

// ---- channel-product fragment (rowfrag: plane16.h; every one of the P planes) of tile t straight from global memory (the
// unit's own side, once per unit; token rows >= L read as zero).  Plain map: column m of tile 1 is token 16 + m; QUARTER:
// row m of tile 1 is token 16 + (m >> 2).  `base` = the row-0 slot of the (node, head), which holds its planes one after
// the other, 2 dh bytes each
template <int P, bool HALF, bool QUARTER>
__device__ __forceinline__ Frag<P> frag_global(const char *base, unsigned row_bytes, int t, int L, int lane) {
  const int m = lane & 15, kg = lane >> 4;
  const int j = t == 0 ? m : 16 + (QUARTER ? m >> 2 : m);
  Frag<P> f;
#pragma unroll
  for (int pl = 0; pl < P; ++pl) f.p[pl] = i32x4{0, 0, 0, 0};
  if (j < L && (!HALF || kg < 2)) {
    // (plane 0 last: what reads a unit's own side before the edge loop -- the planes' dS scale -- reads plane 0, and its
    // wait then covers every own-side load; one left pending becomes a vmcnt(0) inside the loop, in front of the
    // prefetched tile pair: +9 % on the destination pass at L < 20)
#pragma unroll
    for (int pl = P - 1; pl >= 0; --pl)
      f.p[pl] = *reinterpret_cast<const i32x4 *>(base + (unsigned)j * row_bytes + pl * (HALF ? kRowBytes / 2 : kRowBytes) + 16 * kg);
  }
  return f;
}
// the fragments of plane16.h for every plane of a tile image
template <class Fmt>
__device__ __forceinline__ typename Fmt::Frag lds_rowfrag(const char *img, int mt, int lane) {
  typename Fmt::Frag f;
#pragma unroll
  for (int pl = 0; pl < Fmt::kPlanes; ++pl) f.p[pl] = rowfrag(img + pl * Fmt::kLoOff, mt, lane);
  return f;
}
template <class Fmt>
__device__ __forceinline__ typename Fmt::Frag lds_colfrag(const char *img, int mc, int lane) {
  typename Fmt::Frag f;
#pragma unroll
  for (int pl = 0; pl < Fmt::kPlanes; ++pl) f.p[pl] = colfrag(img + pl * Fmt::kLoOff, mc, lane);
  return f;
}

// ---- softmax over the 20 source tokens of one destination-token column; `sc` = log2e / sqrt(dh) (/ the scale of the
// scores, where they carry one) is applied to the raw scores here, the result leaves multiplied by `mul`.  t0[q] = token
// 4 g + q, t1[0] = token 16 + g (regs 1..3 of tile 1 replicate it and come out as 0).  `masked` = the format's mask value.
// Returns m * sc + log2(sum): P = exp2(S * sc - that), what a source pass needs to rebuild P without reducing again.
template <bool FULL>
__device__ __forceinline__ float column_softmax(f32x4 &t0, f32x4 &t1, float sc, float mul, float masked, int L, int g) {
  if (!FULL) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * g + q >= L) t0[q] = masked;
    if (16 + g >= L) t1[0] = masked;
  }
  float m = fmaxf(fmaxf(fmaxf(t0[0], t0[1]), fmaxf(t0[2], t0[3])), t1[0]);
  m = groups_max(m);
#pragma unroll
  for (int q = 0; q < 4; ++q) t0[q] = fast_exp2((t0[q] - m) * sc);
  t1[0] = fast_exp2((t1[0] - m) * sc);
  float l = ((t0[0] + t0[1]) + (t0[2] + t0[3])) + t1[0];
  l = groups_sum(l);
  const float inv = fast_rcp(l) * mul;
#pragma unroll
  for (int q = 0; q < 4; ++q) t0[q] *= inv;
  t1[0] *= inv;
  t1[1] = t1[2] = t1[3] = 0.f;
  return fmaf(m, sc, __builtin_amdgcn_logf(l));
}

// ---------------------------------------------------------------- forward
template <class Fmt, bool FULL, bool HALF>
__device__ __forceinline__ void fwd_body(const typename Fmt::Args &a) {
  using F = typename Fmt::Frag;
  using G = typename Fmt::template Geom<HALF>;
  constexpr int MC = Fmt::template mc_tiles<HALF>(), TB = Fmt::kTileBytes, EB = Fmt::kElemBytes;
  __shared__ __attribute__((aligned(16))) char lds_all[kWavesPerBlock][2 * TB];
  for_unit<Fmt, HALF>(a, a.O, nullptr, [&](const Unit &u) __attribute__((always_inline)) {
    const int lane = u.lane, h = u.h, beg = u.beg, end = u.end;
    const int L = a.L, g = lane >> 4;
    char *Kt = lds_all[u.wave], *Vt = Kt + TB;
    const typename Fmt::Scales k = Fmt::template scales<HALF>(a);

    F qB[2];
    {
      const char *qb = slot_ptr<EB>(a.Q, Fmt::qrow(a, u.row), h);
      const unsigned rb = (unsigned)a.Q.row_stride * EB;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) qB[nt] = frag_global<Fmt::kPlanes, HALF, false>(qb, rb, nt, L, lane);
    }
    if (!FULL || (HALF && Fmt::kHalfZeroLds)) lds_zero(Kt, 2 * TB, lane);
    f32x4 OT[MC][2];
#pragma unroll
    for (int mc = 0; mc < MC; ++mc) OT[mc][0] = OT[mc][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    Pair16<G::NLD> kv;
    IdxWindow win;
    const unsigned krb = (unsigned)a.K.row_stride * EB, vrb = (unsigned)a.V.row_stride * EB;
    auto fetch = [&](int p) {
      const int64_t s = idxwin_get<false>(win, a.idx, nullptr, p, end, lane, nullptr);
      pair16_load<FULL, G>(kv, slot_ptr<EB>(a.K, s, h), krb, slot_ptr<EB>(a.V, s, h), vrb, L, lane);
    };
    if (beg < end) {
      idxwin_load<false>(win, a.idx, nullptr, beg, end, lane);
      fetch(beg);
    }
    for (int p = beg; p < end; ++p) {
      pair16_to_lds<FULL, G, TB>(Kt, kv, L, lane);
      if (p + 1 < end) fetch(p + 1);
      __builtin_amdgcn_wave_barrier();

      f32x4 S[2][2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const F kA = lds_rowfrag<Fmt>(Kt, mt, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) S[mt][nt] = Fmt::mma(kA, qB[nt], f32x4{0.f, 0.f, 0.f, 0.f});
      }
      F pB[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        column_softmax<FULL>(S[0][nt], S[1][nt], k.sc, Fmt::kPMul, Fmt::kMasked, L, g);
        if (!Fmt::kShadow) pB[nt] = Fmt::cd_frag(S[0][nt], S[1][nt]);
      }
      F vA[MC];
      if (Fmt::kShadow) TR_PRE_READ();
#pragma unroll
      for (int mc = 0; mc < MC; ++mc) vA[mc] = lds_colfrag<Fmt>(Vt, mc, lane);
      if (Fmt::kShadow) {      // (in the shadow of the reads)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) pB[nt] = Fmt::cd_frag(S[0][nt], S[1][nt]);
      }
      TR_FRAG_FENCE();
#pragma unroll
      for (int mc = 0; mc < MC; ++mc)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) OT[mc][nt] = Fmt::mma(vA[mc], pB[nt], OT[mc][nt]);
      __builtin_amdgcn_wave_barrier();
    }
    const bool hubp = a.hub.mode == 2;       // the hub pass leaves the mean to the combine pass
    Fmt::template store<HALF>(a.O, u.onode, h, OT, Fmt::fwd_scale(k, hubp ? 1.f : (u.deg > 0 ? 1.f / (float)u.deg : 0.f)),
                              hubp, L, lane);
  });
}

// ---------------------------------------------------------------- backward, destination pass
// STATS: the statistics hand-off to the source pass (formats whose Args carry spos / stats): the index window's weight
// slot carries the bits of spos[p], the CSC position of the edge
template <class Fmt, bool FULL, bool STATS, bool HALF>
__device__ __forceinline__ void bwd_dst_body(const typename Fmt::Args &a) {
  using F = typename Fmt::Frag;
  using G = typename Fmt::template Geom<HALF>;
  constexpr int MC = Fmt::template mc_tiles<HALF>(), TB = Fmt::kTileBytes, EB = Fmt::kElemBytes;
  __shared__ __attribute__((aligned(16))) char lds_all[kWavesPerBlock][2 * TB];
  for_unit<Fmt, HALF>(a, a.O, nullptr, [&](const Unit &u) __attribute__((always_inline)) {
    const int lane = u.lane, h = u.h, beg = u.beg, end = u.end;
    const int L = a.L, g = lane >> 4;
    char *Kt = lds_all[u.wave], *Vt = Kt + TB;
    const typename Fmt::Scales k = Fmt::template scales<HALF>(a);

    F qB[2], gB[2];
    {
      const char *qb = slot_ptr<EB>(a.Q, u.row, h), *gb = slot_ptr<EB>(a.dO, u.row, h);
      const unsigned qrb = (unsigned)a.Q.row_stride * EB, grb = (unsigned)a.dO.row_stride * EB;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        qB[nt] = frag_global<Fmt::kPlanes, HALF, false>(qb, qrb, nt, L, lane);
        gB[nt] = frag_global<Fmt::kPlanes, HALF, false>(gb, grb, nt, L, lane);
      }
    }
    const float dsm = Fmt::ds_mul(a, u.deg, gB);      // what dS is multiplied by before it becomes a B operand
    if (!FULL || (HALF && Fmt::kHalfZeroLds)) lds_zero(Kt, 2 * TB, lane);
    f32x4 dQT[MC][2];
#pragma unroll
    for (int mc = 0; mc < MC; ++mc) dQT[mc][0] = dQT[mc][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    Pair16<G::NLD> kv;
    IdxWindow win;
    const unsigned krb = (unsigned)a.K.row_stride * EB, vrb = (unsigned)a.V.row_stride * EB;
    const float *sposf = nullptr;
    if constexpr (STATS) sposf = reinterpret_cast<const float *>(a.spos);
    float cposf = 0.f, cposf_next = 0.f;
    auto fetch = [&](int p) {
      const int64_t s = idxwin_get<STATS>(win, a.idx, sposf, p, end, lane, &cposf_next);
      pair16_load<FULL, G>(kv, slot_ptr<EB>(a.K, s, h), krb, slot_ptr<EB>(a.V, s, h), vrb, L, lane);
    };
    if (beg < end) {
      idxwin_load<STATS>(win, a.idx, sposf, beg, end, lane);
      fetch(beg);
    }
    for (int p = beg; p < end; ++p) {
      pair16_to_lds<FULL, G, TB>(Kt, kv, L, lane);
      cposf = cposf_next;
      if (p + 1 < end) fetch(p + 1);
      __builtin_amdgcn_wave_barrier();

      f32x4 S[2][2], dP[2][2];
      float lse[2], dlt[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const F kA = lds_rowfrag<Fmt>(Kt, mt, lane);
        const F vA = lds_rowfrag<Fmt>(Vt, mt, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          S[mt][nt] = Fmt::mma(kA, qB[nt], f32x4{0.f, 0.f, 0.f, 0.f});
          dP[mt][nt] = Fmt::mma(vA, gB[nt], f32x4{0.f, 0.f, 0.f, 0.f});
        }
      }
      F sB[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        lse[nt] = column_softmax<FULL>(S[0][nt], S[1][nt], k.sc, 1.f, Fmt::kMasked, L, g);      // P^T; tile-1 regs 1..3 come out 0
        float part = S[1][nt][0] * dP[1][nt][0];
#pragma unroll
        for (int q = 0; q < 4; ++q) part = fmaf(S[0][nt][q], dP[0][nt][q], part);
        const float delta = groups_sum(part);
        dlt[nt] = delta;
#pragma unroll
        for (int q = 0; q < 4; ++q) S[0][nt][q] *= (dP[0][nt][q] - delta) * dsm;      // dS^T
        S[1][nt][0] *= (dP[1][nt][0] - delta) * dsm;
        if (!Fmt::kShadow) sB[nt] = Fmt::cd_frag(S[0][nt], S[1][nt]);
      }
      F kC[MC];
      if (Fmt::kShadow) TR_PRE_READ();
#pragma unroll
      for (int mc = 0; mc < MC; ++mc) kC[mc] = lds_colfrag<Fmt>(Kt, mc, lane);
      if (Fmt::kShadow) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) sB[nt] = Fmt::cd_frag(S[0][nt], S[1][nt]);
      }
      TR_FRAG_FENCE();
#pragma unroll
      for (int mc = 0; mc < MC; ++mc)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) dQT[mc][nt] = Fmt::mma(kC[mc], sB[nt], dQT[mc][nt]);
      if constexpr (STATS) {
        // every lane group holds the statistics of its column: lanes 0..15 have tokens 0..15 (tile 0), lanes 16..19
        // (group 1, columns 0..3) tokens 16..19 (tile 1): two 80-byte stores per edge and head
        float *st = a.stats + ((int64_t)__builtin_bit_cast(int, cposf) * a.H + h) * kStatsPerUnit;
        if (lane < L) {
          st[lane] = lane < 16 ? lse[0] : lse[1];
          st[kLmax + lane] = lane < 16 ? dlt[0] : dlt[1];
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    const bool hubp = a.hub.mode == 2;       // the hub pass leaves 1/sqrt(dh) to the combine pass
    const float m = Fmt::template store<HALF>(a.O, u.onode, h, dQT, Fmt::template dq_scale<HALF>(a, k, dsm, hubp), hubp, L, lane);
    Fmt::record_absmax(a, m);
  });
}

// ---- kernels[half][full] of one pass (and one value of STATS), and its launch
#define WAVE16_KERNELS(K) {{K<false, false>, K<true, false>}, {K<false, true>, K<true, true>}}
#define WAVE16_KERNELS_STATS(K, S) {{K<false, S, false>, K<true, S, false>}, {K<false, S, true>, K<true, S, true>}}
template <class Args>
int launch_wave16(void (*const (&kernels)[2][2])(Args), const Args &a, int L, bool half, hipStream_t stream) {
  return launch_wave_units(kernels[half][L == kLmax], a, kWavesPerBlock, stream);
}

}  // namespace wave16
