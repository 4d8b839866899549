// Workgroup-per-unit edge kernels for the shapes the one-wave-per-unit kernels do not take: L <= 64, even dh <= 64.  fp32
// storage (the reference's AMPGCN class defaults: L = 40, D = 100, H = 2 -> dh = 50, src/ampnet/module/amp_gcn.py:21-35)
// runs OFF the FP32 pipe: every fp32 tile is split into THREE bf16 planes on its way into LDS
//      x = h + m + l,   h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)        (24 significand bits, no scale needed:
//                                                                                 bf16 has fp32's exponent range)
// and every product is the fp32 sum of six v_mfma_f32_16x16x32_bf16 partial products
//      a b ~ a_l b_h + a_h b_l + a_m b_m + a_m b_h + a_h b_m + a_h b_h           (dropped: a_m b_l + a_l b_m + a_l b_l
//                                                                                 <= 2^-24 |a b|)
// -- 96 matrix-pipe cycles per 16 x 16 x 32 block instead of the 256 of eight v_mfma_f32_16x16x4_f32, and on the 16-bit
// matrix pipe, which runs beside the vector ALU instead of on it.  Softmax, delta and all sums stay fp32.  The source pass
// exists only with the softmax statistics the destination pass hands over (include/ampconv.h).  (The fp32-MFMA kernels
// that served these shapes up to round 5, edge_block.hip, were removed once these replaced them: see git history.)
//
// One WORKGROUP owns one (row, head) unit; wave w of its NT = ceil(L / 16) owns the unit's own tokens 16 w .. 16 w + 15
// (the COLUMNS of every score tile), all waves share the LDS images of the streamed pair of tiles.  Per plane an image
// is [16 NT token rows][64 channels] bf16 = 128-byte rows (dh <= 32: template KS = 1, one 32-channel k-step and two channel
// tiles instead of two and four; the upper half of every row is then neither staged nor read), 16-byte chunk c of row j stored at chunk c ^ 2 ((j >> 1) & 3):
// the ds_read_b128 of the channel-product fragments and the ds_read_b64_tr_b16 of the token-product fragments are both
// bank-conflict free (tools/lds_bank_check.py).
//
// Structure: each pass is written ONCE (fwd_body, bwd_dst_body, bwd_src_body) over an operand-format policy, and the
// nine __global__ kernels are named wrappers that carry their own launch bounds.  The three formats:
//      FmtX3   fp32 storage, three bf16 planes, six products                     fwd_x3 / bwd_dst_x3 / bwd_src_x3
//      FmtXH   fp32 storage, two fp16 planes of the scaled value, three products fwd_xh / bwd_dst_xh / bwd_src_xh
//      FmtXB   bf16 storage, the one plane as it lies in memory, one product     fwd_xb / bwd_dst_xb / bwd_src_xb
// A policy names the storage (element, staging registers, own-side registers, store), the plane count, `split` (two
// values -> their packed planes) and `mma`, the compile-time choices (channel tiles per group of transposed reads, the
// loop shape of the source pass) and the scale hooks: where this format multiplies which factor in.  Everything that
// follows from the plane count alone (fragment reads, staging stores, LDS sizes) is written over it.
// Reference arithmetic replaced: torch functional.py:6578-6594 per edge, the mean of amp_conv.py:11, and their autograd
// backward.
#include "plane16.h"

namespace {
using namespace plane16;      // conversions, plane_scale, split2, frag_sumsq, tr_half, TR_FRAG_FENCE / TR_WAR_GUARD

constexpr int kRowB = 128;                 // one plane of a token row: 64 bf16 channels
constexpr int kTileRowsB = 16 * kRowB;     // 16 token rows of one plane

#define MFMA_X3(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), (c), 0, 0, 0)
#define MFMA_XH(a, b, c) \
  __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), (c), 0, 0, 0)

// one MFMA operand in P planes, largest first
template <int P>
struct XFrag {
  i32x4 p[P];
};

__device__ __forceinline__ float bfl(int u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bfh(int u) { return __builtin_bit_cast(float, u & (int)0xFFFF0000u); }

// byte offset of 16-byte chunk `ch` (0..7) of token row j in a plane image
__device__ __forceinline__ int xoff(int j, int ch) { return j * kRowB + ((ch ^ (((j >> 1) & 3) << 1)) << 4); }

struct XArgs {
  ampconv_view_t Q, K, V, dO, O, dK, dV;     // O = forward output / dQ
  const int32_t *ptr, *idx, *qidx;
  const float *cinv;
  const int32_t *spos;
  float *stats;
  HubArgs hub;              // long-segment plan (hub.hip): mode 1 skips long rows, mode 2 = one unit per chunk
  int64_t n_units;
  int L, dh, H;
  float qscale, oscale;
  const float *bounds;      // scaled kernels: device {bound of |Q|K|V|, bound of |dObar|, recorded max |V|, recorded max |dObar|}
  float *absmax;            // scaled backward kernels, or null: atomic max of the finite magnitudes written
};

template <class E>
__device__ __forceinline__ const E *tile_of(const ampconv_view_t &v, int64_t n, int h) {
  return reinterpret_cast<const E *>(v.ptr) + n * v.node_stride + (int64_t)h * v.head_stride;
}

// ---- cooperative staging of two [L x dh] tiles (A then B): global -> registers -> (split ->) plane images.  Thread
// (r0 = tid / DVP, cv = tid % DVP) owns vector column cv (VEC elements) of rows r0 + i RS.
template <int VEC, int NT, int KS>
struct StageGeom {
  static constexpr int DVP = 32 * KS / VEC;                 // vector slots per padded row (KS k-steps of 32 channels)
  static constexpr int RS = 64 * NT / DVP;                  // rows per pass
  static constexpr int NP = (16 * NT + RS - 1) / RS;        // passes
};
template <int VEC, int NT, int KS>
struct StageX : StageGeom<VEC, NT, KS> {                    // fp32 storage
  float v[2][StageGeom<VEC, NT, KS>::NP][VEC];
};
template <int VEC, int NT, int KS>
struct StageB : StageGeom<VEC, NT, KS> {                    // bf16 storage: VEC = 2 or 4 elements = 1 or 2 words
  int v[2][StageGeom<VEC, NT, KS>::NP][VEC / 2];
};

// Loads: raw buffer loads off a per-tile resource (base = the (node, head) tile, uniform; num_records = the bytes of the
// tile that exist), ONE per-thread byte offset per tensor and a scalar offset per pass -- no per-lane address arithmetic,
// no predicates: token rows >= L lie beyond num_records and channels >= dh carry an out-of-range offset, both read as 0
// and are filed as the zero padding of the image.
struct StageSrc {
  unsigned voA, voB;        // byte offset of (row r0, channel c) in a tile of tensor A / B
  int stepA, stepB;         // bytes between two passes (RS token rows)
  int nrecA, nrecB;         // bytes from the tile's first element to the end of its last row
};
template <int ESIZE, int VEC, int NT, int KS>               // row strides sA, sB in elements of ESIZE bytes
__device__ __forceinline__ StageSrc stage_src(int sA, int sB, int L, int dh, int tid) {
  using S = StageGeom<VEC, NT, KS>;
  const int cv = tid % S::DVP, r0 = tid / S::DVP, c = cv * VEC;
  StageSrc q;
  q.voA = c < dh ? (unsigned)(r0 * sA + c) * (unsigned)ESIZE : 0x80000000u;
  q.voB = c < dh ? (unsigned)(r0 * sB + c) * (unsigned)ESIZE : 0x80000000u;
  q.stepA = S::RS * sA * ESIZE;
  q.stepB = S::RS * sB * ESIZE;
  q.nrecA = ((L - 1) * sA + dh) * ESIZE;
  q.nrecB = ((L - 1) * sB + dh) * ESIZE;
  return q;
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void *base, int nrec) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, nrec, 0x00020000);
}

template <int VEC, int NT, int KS>
__device__ __forceinline__ void stage_load(StageX<VEC, NT, KS> &s, const float *A, const float *B, const StageSrc &q, int L) {
  using S = StageX<VEC, NT, KS>;
  const __amdgpu_buffer_rsrc_t ra = tile_rsrc(A, q.nrecA), rb = tile_rsrc(B, q.nrecB);
#pragma unroll
  for (int i = 0; i < S::NP; ++i) {
    if (i * S::RS < L) {                                    // (uniform: whole passes beyond L are not issued)
      if constexpr (VEC == 4) {
        // (bit_cast of the builtin's result as a whole: element access on the returned vector type picks element 0 for
        // every index with this compiler)
        const f32x4 x = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, q.voA, i * q.stepA, 0));
        const f32x4 y = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, q.voB, i * q.stepB, 0));
        s.v[0][i][0] = x[0]; s.v[0][i][1] = x[1]; s.v[0][i][2] = x[2]; s.v[0][i][3] = x[3];
        s.v[1][i][0] = y[0]; s.v[1][i][1] = y[1]; s.v[1][i][2] = y[2]; s.v[1][i][3] = y[3];
      } else {
        const f32x2 x = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(ra, q.voA, i * q.stepA, 0));
        const f32x2 y = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rb, q.voB, i * q.stepB, 0));
        s.v[0][i][0] = x[0]; s.v[0][i][1] = x[1];
        s.v[1][i][0] = y[0]; s.v[1][i][1] = y[1];
      }
    }
  }
}
template <int VEC, int NT, int KS>
__device__ __forceinline__ void stage_load(StageB<VEC, NT, KS> &s, const unsigned short *A, const unsigned short *B,
                                           const StageSrc &q, int L) {
  using S = StageB<VEC, NT, KS>;
  const __amdgpu_buffer_rsrc_t ra = tile_rsrc(A, q.nrecA), rb = tile_rsrc(B, q.nrecB);
#pragma unroll
  for (int i = 0; i < S::NP; ++i) {
    if (i * S::RS < L) {
      if constexpr (VEC == 4) {
        const i32x2 x = __builtin_bit_cast(i32x2, __builtin_amdgcn_raw_buffer_load_b64(ra, q.voA, i * q.stepA, 0));
        const i32x2 y = __builtin_bit_cast(i32x2, __builtin_amdgcn_raw_buffer_load_b64(rb, q.voB, i * q.stepB, 0));
        s.v[0][i][0] = x[0]; s.v[0][i][1] = x[1];
        s.v[1][i][0] = y[0]; s.v[1][i][1] = y[1];
      } else {
        s.v[0][i][0] = (int)__builtin_amdgcn_raw_buffer_load_b32(ra, q.voA, i * q.stepA, 0);
        s.v[1][i][0] = (int)__builtin_amdgcn_raw_buffer_load_b32(rb, q.voB, i * q.stepB, 0);
      }
    }
  }
}

// LDS byte offsets of this thread's vector in the rows it stages (plane 0 of an image)
template <int VEC, int NT, int KS>
struct StageOffs {
  int v[StageGeom<VEC, NT, KS>::NP];
};
template <int VEC, int NT, int KS>
__device__ __forceinline__ void stage_offsets(StageOffs<VEC, NT, KS> &lo, int tid) {
  using S = StageGeom<VEC, NT, KS>;
  const int cv = tid % S::DVP, r0 = tid / S::DVP, c = cv * VEC;
#pragma unroll
  for (int i = 0; i < S::NP; ++i) lo.v[i] = xoff(r0 + i * S::RS, c >> 3) + (c & 7) * 2;
}

// fp32 storage: every pair of values times its tensor's factor, split, one store per plane
template <class Fmt, int VEC, int NT, int KS>
__device__ __forceinline__ void stage_store(char *imgA, char *imgB, const StageX<VEC, NT, KS> &s,
                                            const StageOffs<VEC, NT, KS> &lo, float mulA, float mulB, int L) {
  using S = StageX<VEC, NT, KS>;
  constexpr int P = Fmt::kPlanes, PB = 16 * NT * kRowB;
#pragma unroll
  for (int i = 0; i < S::NP; ++i) {
    if (i * S::RS < L) {                                    // (lanes beyond the tile hold zeros: the image's padding)
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        char *img = (x ? imgB : imgA) + lo.v[i];
        const float mul = x ? mulB : mulA;
        int w[VEC / 2][P];
#pragma unroll
        for (int k = 0; k < VEC / 2; ++k) Fmt::split(s.v[x][i][2 * k] * mul, s.v[x][i][2 * k + 1] * mul, w[k]);
#pragma unroll
        for (int pl = 0; pl < P; ++pl) {
          if constexpr (VEC == 4) *reinterpret_cast<i32x2 *>(img + pl * PB) = i32x2{w[0][pl], w[1][pl]};
          else *reinterpret_cast<int *>(img + pl * PB) = w[0][pl];
        }
      }
    }
  }
}
// bf16 storage: the words as they were loaded
template <class Fmt, int VEC, int NT, int KS>
__device__ __forceinline__ void stage_store(char *imgA, char *imgB, const StageB<VEC, NT, KS> &s,
                                            const StageOffs<VEC, NT, KS> &lo, float, float, int L) {
  using S = StageB<VEC, NT, KS>;
#pragma unroll
  for (int i = 0; i < S::NP; ++i) {
    if (i * S::RS < L) {
      if constexpr (VEC == 4) {
        *reinterpret_cast<i32x2 *>(imgA + lo.v[i]) = i32x2{s.v[0][i][0], s.v[0][i][1]};
        *reinterpret_cast<i32x2 *>(imgB + lo.v[i]) = i32x2{s.v[1][i][0], s.v[1][i][1]};
      } else {
        *reinterpret_cast<int *>(imgA + lo.v[i]) = s.v[0][i][0];
        *reinterpret_cast<int *>(imgB + lo.v[i]) = s.v[1][i][0];
      }
    }
  }
}

// the unit's own side as COLUMN fragments (B operand), once per unit from global memory: lane (n = lane & 15, kg) holds
// channels 32 ks + 8 kg .. + 7 of token 16 wave + n; token rows >= L and channels >= dh read as zero.  Two steps, so
// that the loads are in flight while the unit's first tiles are requested (own_load), and are only waited for behind
// that (own_split: fp32 storage scales and splits there, bf16 storage has its fragment already).
template <int KS>
struct OwnRaw {
  float2 x[KS][4];
};
template <int KS>
struct OwnB {
  i32x4 f[KS];
};
template <int KS>
__device__ __forceinline__ void own_load(OwnRaw<KS> &o, const float *base, int row_stride, int wave, int L, int dh, int lane) {
  const int n = lane & 15, kg = lane >> 4, j = 16 * wave + n;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 32 * ks + 8 * kg + 2 * u;
      o.x[ks][u] = make_float2(0.f, 0.f);
      if (j < L && c < dh) o.x[ks][u] = *reinterpret_cast<const float2 *>(base + j * row_stride + c);
    }
  }
}
template <int KS>
__device__ __forceinline__ void own_load(OwnB<KS> &o, const unsigned short *base, int row_stride, int wave, int L, int dh,
                                         int lane) {
  const int n = lane & 15, kg = lane >> 4, j = 16 * wave + n;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    int w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = 32 * ks + 8 * kg + 2 * u;
      w[u] = (j < L && c < dh) ? *reinterpret_cast<const int *>(base + j * row_stride + c) : 0;
    }
    o.f[ks] = i32x4{w[0], w[1], w[2], w[3]};
  }
}
template <class Fmt, int KS>
__device__ __forceinline__ void own_split(typename Fmt::Frag (&f)[KS], const OwnRaw<KS> &o, float mul) {
  constexpr int P = Fmt::kPlanes;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    int w[4][P];
#pragma unroll
    for (int u = 0; u < 4; ++u) Fmt::split(o.x[ks][u].x * mul, o.x[ks][u].y * mul, w[u]);
#pragma unroll
    for (int pl = 0; pl < P; ++pl) f[ks].p[pl] = i32x4{w[0][pl], w[1][pl], w[2][pl], w[3][pl]};
  }
}
template <class Fmt, int KS>
__device__ __forceinline__ void own_split(typename Fmt::Frag (&f)[KS], const OwnB<KS> &o, float) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) f[ks].p[0] = o.f[ks];
}

// channel-product fragment (A operand) of token tile t, k-step ks: `aks` = this lane's byte offset for that k-step
template <int P, int NT>
__device__ __forceinline__ XFrag<P> rowfrag(const char *img, int aks, int t) {
  const char *p = img + aks + t * kTileRowsB;
  XFrag<P> f;
#pragma unroll
  for (int pl = 0; pl < P; ++pl) f.p[pl] = *reinterpret_cast<const i32x4 *>(p + pl * (16 * NT * kRowB));
  return f;
}

// token-product fragment (A operand, rows = channels 16 mc .. + 15) over the token tiles (2 pair, 2 pair + 1): k-slots
// 0..3 = tokens 16 (2 pair) + 4 kg + 0..3, slots 4..7 = the same rows of the next tile (a last odd tile: its own values
// again -- finite -- against zeros in the other operand).  `trb` = this lane's byte offset for channel tile mc.
template <int P, int NT>
__device__ __forceinline__ XFrag<P> colfrag(const char *img, int trb, int pair) {
  constexpr int PB = 16 * NT * kRowB;
  const char *p = img + trb + 2 * pair * kTileRowsB;
  const bool two = 2 * pair + 1 < NT;
  i32x2 a[P], b[P];
#pragma unroll
  for (int pl = 0; pl < P; ++pl) a[pl] = tr_half(p + pl * PB);
#pragma unroll
  for (int pl = 0; pl < P; ++pl) b[pl] = two ? tr_half(p + kTileRowsB + pl * PB) : a[pl];
  XFrag<P> f;
#pragma unroll
  for (int pl = 0; pl < P; ++pl) f.p[pl] = i32x4{a[pl][0], a[pl][1], b[pl][0], b[pl][1]};
  return f;
}
// C/D tiles of a tile pair (lane (n, g), reg q of tile t = token 16 t + 4 g + q; already in the split's units) -> the B
// operand of the token product
template <class Fmt, int NT>
__device__ __forceinline__ typename Fmt::Frag cd_frag(const f32x4 (&T)[NT], int pair) {
  constexpr int P = Fmt::kPlanes;
  int w[4][P] = {};
  const f32x4 a = T[2 * pair];
  Fmt::split(a[0], a[1], w[0]);
  Fmt::split(a[2], a[3], w[1]);
  if (2 * pair + 1 < NT) {
    const f32x4 b = T[2 * pair + 1 < NT ? 2 * pair + 1 : 0];
    Fmt::split(b[0], b[1], w[2]);
    Fmt::split(b[2], b[3], w[3]);
  }
  typename Fmt::Frag f;
#pragma unroll
  for (int pl = 0; pl < P; ++pl) f.p[pl] = i32x4{w[0][pl], w[1][pl], w[2][pl], w[3][pl]};
  return f;
}

// per-lane address parts of the fragment reads
struct FragAddr {
  int a[2];       // channel-product fragments, k-steps 0 / 1
  int tr[4];      // token-product fragments, channel tiles 0..3
};
__device__ __forceinline__ FragAddr frag_addr(int lane) {
  FragAddr fa;
  const int m = lane & 15, kg = lane >> 4;
  fa.a[0] = xoff(m, kg);
  fa.a[1] = fa.a[0] ^ 64;                                   // chunk 4 + kg: the swizzle only touches bits 1..2
  const int q = (lane >> 2) & 3, pp = lane & 3, row = 4 * kg + q;
#pragma unroll
  for (int mc = 0; mc < 4; ++mc) fa.tr[mc] = xoff(row, 2 * mc + (pp >> 1)) + ((pp & 1) << 3);
  return fa;
}

// output: C/D tiles [channel tile mc] of this wave's token tile -> global fp32 rows (channels < dh, tokens < L).  Lane
// (token n = lane & 15, g), register r of tile mc = channel 16 mc + 4 g + r
template <int VEC, int MCT>
__device__ __forceinline__ float store_x3(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[MCT], float scale,
                                          int tile, int L, int dh, int lane) {
  const int i = (lane & 15) + 16 * tile, g = lane >> 4;
  float mx = 0.f;                      // largest finite magnitude stored (the scaled backward kernels record it)
  if (i >= L) return mx;
  float *row = reinterpret_cast<float *>(v.ptr) + node * v.node_stride + (int64_t)h * v.head_stride + (int64_t)i * v.row_stride;
#pragma unroll
  for (int mc = 0; mc < MCT; ++mc) {
    const int c = 16 * mc + 4 * g;
    const float x0 = T[mc][0] * scale, x1 = T[mc][1] * scale, x2 = T[mc][2] * scale, x3 = T[mc][3] * scale;
    if constexpr (VEC == 4) {
      if (c < dh) {
        *reinterpret_cast<float4 *>(row + c) = make_float4(x0, x1, x2, x3);
        mx = finite_abs_max(mx, make_float4(x0, x1, x2, x3));
      }
    } else {
      if (c < dh) {
        *reinterpret_cast<float2 *>(row + c) = make_float2(x0, x1);
        mx = fmaxf(mx, fmaxf(finite_abs(x0), finite_abs(x1)));
      }
      if (c + 2 < dh) {
        *reinterpret_cast<float2 *>(row + c + 2) = make_float2(x2, x3);
        mx = fmaxf(mx, fmaxf(finite_abs(x2), finite_abs(x3)));
      }
    }
  }
  return mx;
}
// bf16 storage: bf16 rows (main pass) or fp32 partial tiles (long-segment pass)
template <int VEC, int MCT>
__device__ __forceinline__ float store_xb(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[MCT], float scale, int tile,
                                          int L, int dh, int lane, bool partial) {
  if (partial) return store_x3<2, MCT>(v, node, h, T, scale, tile, L, dh, lane);
  const int i = (lane & 15) + 16 * tile, g = lane >> 4;
  if (i >= L) return 0.f;
  unsigned short *row = reinterpret_cast<unsigned short *>(v.ptr) + node * v.node_stride + (int64_t)h * v.head_stride +
                        (int64_t)i * v.row_stride;
#pragma unroll
  for (int mc = 0; mc < MCT; ++mc) {
    const int c = 16 * mc + 4 * g;
    const int p0 = cvt_pk_bf16(T[mc][0] * scale, T[mc][1] * scale), p1 = cvt_pk_bf16(T[mc][2] * scale, T[mc][3] * scale);
    if constexpr (VEC == 4) {
      if (c < dh) *reinterpret_cast<i32x2 *>(row + c) = i32x2{p0, p1};
    } else {
      if (c < dh) *reinterpret_cast<int *>(row + c) = p0;
      if (c + 2 < dh) *reinterpret_cast<int *>(row + c + 2) = p1;
    }
  }
  return 0.f;
}

// softmax over the source tokens (MFMA rows of every token tile) of one destination-token column; returns m + log2(sum)
template <int NT>
__device__ __forceinline__ float x3_column_softmax(f32x4 (&S)[NT], int L, int g) {
  float m = kNegBig;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (16 * t + 4 * g + q >= L) S[t][q] = kNegBig;
      m = fmaxf(m, S[t][q]);
    }
  }
  m = groups_max(m);
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      S[t][q] = fast_exp2(S[t][q] - m);
      l += S[t][q];
    }
  }
  l = groups_sum(l);
  const float inv = fast_rcp(l);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) S[t][q] *= inv;
  }
  return m + __builtin_amdgcn_logf(l);
}
// the same on RAW scores: `sc` = log2e / sqrt(dh) / (scale of the score product) is applied here, the weights leave
// multiplied by `mul`.  Returns m sc + log2(sum): P = exp2(S' sc - that).
constexpr float kMaskedX = -__builtin_inff();     // (scores meet their scale inside the exponential: a finite mask could be scaled back into range)
template <int NT>
__device__ __forceinline__ float xh_column_softmax(f32x4 (&S)[NT], float sc, float mul, int L, int g) {
  float m = kMaskedX;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (16 * t + 4 * g + q >= L) S[t][q] = kMaskedX;
      m = fmaxf(m, S[t][q]);
    }
  }
  m = groups_max(m);
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      S[t][q] = fast_exp2((S[t][q] - m) * sc);
      l += S[t][q];
    }
  }
  l = groups_sum(l);
  const float inv = fast_rcp(l) * mul;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int q = 0; q < 4; ++q) S[t][q] *= inv;
  }
  return fmaf(m, sc, __builtin_amdgcn_logf(l));
}

// the staging passes rewrite whole 64-channel rows (zeros in the padding) of every token row below RS ceil(L / RS); the
// rows above that, in all plane images, are zeroed once per unit
template <int VEC, int NT, int KS, int NPLANES>
__device__ __forceinline__ void lds_zero_tail(char *p, int L, int tid) {
  using S = StageGeom<VEC, NT, KS>;
  constexpr int PB = 16 * NT * kRowB;
  const int zr = ((L + S::RS - 1) / S::RS) * S::RS, nrow = 16 * NT - zr;      // rows zr .. 16 NT - 1
  for (int i = tid; i < NPLANES * nrow * (kRowB / 16); i += 64 * NT) {
    const int plane = i / (nrow * (kRowB / 16)), rem = i - plane * (nrow * (kRowB / 16));
    *reinterpret_cast<i32x4 *>(p + plane * PB + zr * kRowB + rem * 16) = i32x4{0, 0, 0, 0};
  }
}

// scale of a finished dQ / dK tile: partial tiles of a long segment leave unscaled, the combine pass applies it
__device__ __forceinline__ float part_or(const XArgs &a, float scale) { return a.hub.mode == 2 ? 1.f : scale; }

// =====================================================================================================================
// The operand formats.  Developer A/B switches: minimum waves per SIMD of each kernel (at its wrapper below); channel
// tiles per group of transposed reads; source pass one pair of destination-token tiles at a time.
#ifndef AMPCONV_X3_FWD_MCB
#define AMPCONV_X3_FWD_MCB 1
#endif
#ifndef AMPCONV_X3_DST_MCB
#define AMPCONV_X3_DST_MCB 2
#endif
#ifndef AMPCONV_X3_SRC_PAIRS
#define AMPCONV_X3_SRC_PAIRS 0
#endif
#ifndef AMPCONV_XH_FWD_MCB
#define AMPCONV_XH_FWD_MCB 1
#endif
#ifndef AMPCONV_XH_DST_MCB
#define AMPCONV_XH_DST_MCB 1
#endif
#ifndef AMPCONV_XH_SRC_PAIRS
#define AMPCONV_XH_SRC_PAIRS 1
#endif

// what fp32 storage gives the two split formats
struct Fp32Storage {
  using Elem = float;
  template <int VEC, int NT, int KS> using Stage = StageX<VEC, NT, KS>;
  template <int KS> using Own = OwnRaw<KS>;
  template <int VEC, int MCT>
  static __device__ __forceinline__ float store(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[MCT], float scale,
                                                int tile, int L, int dh, int lane, bool) {
    return store_x3<VEC, MCT>(v, node, h, T, scale, tile, L, dh, lane);
  }
};

// ---- three bf16 planes of the fp32 value.  Scales: log2e / sqrt(dh) is folded into Q (own side: when it is split;
// streamed side: in the staging pass), 1 / in-degree into dObar the same way; nothing else.
struct FmtX3 : Fp32Storage {
  static constexpr int kPlanes = 3;
  using Frag = XFrag<3>;
  static constexpr bool kQidx = true, kRecordMax = false, kSrcPairs = AMPCONV_X3_SRC_PAIRS;
  static constexpr float kPScale = 1.f;
  static constexpr int fwd_mcb(int) { return AMPCONV_X3_FWD_MCB; }
  static constexpr int dst_mcb(int) { return AMPCONV_X3_DST_MCB; }

  // (x0, x1) -> packed bf16 pairs of the three planes (the residuals are exact fp32 differences)
  static __device__ __forceinline__ void split(float x0, float x1, int (&w)[3]) {
    w[0] = cvt_pk_bf16(x0, x1);
    float r0 = x0 - bfl(w[0]), r1 = x1 - bfh(w[0]);
    w[1] = cvt_pk_bf16(r0, r1);
    r0 -= bfl(w[1]);
    r1 -= bfh(w[1]);
    w[2] = cvt_pk_bf16(r0, r1);
  }
  // the six partial products of one fp32-grade product, smallest first (planes h, m, l = p[0], p[1], p[2])
  static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) {
    c = MFMA_X3(a.p[2], b.p[0], c);
    c = MFMA_X3(a.p[0], b.p[2], c);
    c = MFMA_X3(a.p[1], b.p[1], c);
    c = MFMA_X3(a.p[1], b.p[0], c);
    c = MFMA_X3(a.p[0], b.p[1], c);
    return MFMA_X3(a.p[0], b.p[0], c);
  }

  __device__ __forceinline__ FmtX3(const XArgs &, bool) {}
  __device__ __forceinline__ float q_mul(const XArgs &a) const { return a.qscale; }      // Q, own or streamed
  __device__ __forceinline__ float g_mul(float inv) const { return inv; }                // dObar, own or streamed
  __device__ __forceinline__ float kv_mul() const { return 1.f; }                        // K and V, own or streamed
  template <int KS> __device__ __forceinline__ void dst_own(const Frag (&)[KS], const XArgs &) {}
  template <int KS> __device__ __forceinline__ void src_own(const Frag (&)[KS], const XArgs &) {}
  template <int NT>
  __device__ __forceinline__ float softmax(f32x4 (&S)[NT], float, int L, int g) const { return x3_column_softmax<NT>(S, L, g); }
  __device__ __forceinline__ float dst_ds(float x, float) const { return x; }            // x = dP - delta
  __device__ __forceinline__ void src_pds(float s, float lse, float dp, float delta, bool ok, float, float &P, float &dS) const {
    const float pr = ok ? fast_exp2(s - lse) : 0.f;
    P = pr;
    dS = pr * (dp - delta);
  }
  __device__ __forceinline__ float o_mul(float x) const { return x; }
  __device__ __forceinline__ float dq_mul(const XArgs &a) const { return part_or(a, a.oscale); }
  __device__ __forceinline__ float dk_mul(const XArgs &a) const { return part_or(a, a.oscale); }
  __device__ __forceinline__ float dv_mul() const { return 1.f; }
};

// ---- TWO fp16 planes of the power-of-two-SCALED value (entry points ampconv_*_edge_scaled): with a device-side bound
// of the operands' magnitudes -- the a-priori bound of the projection that produced them, as for the plane-format
// kernels of edge_mfma_f16x2.hip -- x 2^e = hi + lo with |x 2^e| < 2^15 needs two 16-bit planes instead
// of three and three partial products instead of six:
//      a b ~ a_lo b_hi + a_hi b_lo + a_hi b_hi        (dropped: a_lo b_lo <= 2^-22 |a b|)
// Half the matrix-pipe cycles, two thirds of the split's vector instructions and of the LDS traffic of the bf16 version.
// Scale and split are those of plane16.h, the scale bookkeeping is that of edge_mfma_f16x2.hip: scores meet their scale
// inside the exponential, P is split as
// P 2^14, dS with one power of two per WAVE from what the wave can see (Cauchy-Schwarz: its own side's largest token-row
// norm, sqrt(64) x the recorded maximum of the streamed tensor); dObar is divided by the in-degree here (own side: once
// per unit, streamed side: in the staging pass), the statistics hand-off carries delta in the units of dP' = dO' V'^T.
// (plane_scale, split2, frag_sumsq: plane16.h)
// largest token-row norm^2 of the wave's own 16 tokens (hi planes of its two k-step fragments): wave-uniform
template <int KS>
__device__ __forceinline__ float own_max_norm2(const XFrag<2> (&f)[KS]) {
  float q = frag_sumsq(f[0].p[0]);
  if constexpr (KS == 2) q += frag_sumsq(f[1].p[0]);
  const float t = groups_sum(q);
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, row16_max(t))));
}
// scale of dS for a wave whose own side has largest row norm^2 `own2` and whose streamed side is bounded by `other` per
// element (both in plane units, 64 channels): dS * scale < 2^15
__device__ __forceinline__ float ds_scale_x(float own2, float other) {
  return plane_scale(2.f * __builtin_sqrtf(own2) * (8.f * other));
}

struct FmtXH : Fp32Storage {
  static constexpr int kPlanes = 2;
  using Frag = XFrag<2>;
  // (no query subset: the scaled forward entry point has no such argument)
  static constexpr bool kQidx = false, kRecordMax = true, kSrcPairs = AMPCONV_XH_SRC_PAIRS;
  static constexpr float kPScale = 16384.f, kPUnscale = 1.f / 16384.f;      // P is split as P 2^14
  static constexpr int fwd_mcb(int) { return AMPCONV_XH_FWD_MCB; }
  static constexpr int dst_mcb(int) { return AMPCONV_XH_DST_MCB; }

  // (x0, x1), already scaled, |x| < 2^16 -> packed fp16 pairs of the two planes
  static __device__ __forceinline__ void split(float x0, float x1, int (&w)[2]) { split2(x0, x1, w[0], w[1]); }
  static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) {      // planes hi, lo = p[0], p[1]
    c = MFMA_XH(a.p[1], b.p[0], c);
    c = MFMA_XH(a.p[0], b.p[1], c);
    return MFMA_XH(a.p[0], b.p[0], c);
  }

  float sq, uq, sg, ug;     // plane scales of Q|K|V and of dObar with their inverses (powers of two: exact)
  float sc;                 // log2e / sqrt(dh) / (scale of Q' K'^T)
  float sd, usd;            // this wave's scale of dS
  // (the forward pass reads bounds[0] only: include/ampconv.h)
  __device__ __forceinline__ FmtXH(const XArgs &a, bool grad)
      : sq(plane_scale(a.bounds[0])), uq(1.f / sq), sg(grad ? plane_scale(a.bounds[1]) : 1.f), ug(1.f / sg),
        sc((a.qscale * uq) * uq), sd(1.f), usd(1.f) {}
  __device__ __forceinline__ float q_mul(const XArgs &) const { return sq; }
  __device__ __forceinline__ float g_mul(float inv) const { return inv * sg; }
  __device__ __forceinline__ float kv_mul() const { return sq; }
  // dS = P (dP' - delta'), |dP'_ij| <= |dO'_i| |V'_j|.  Destination pass: this wave's dO' rows, any V' row
  template <int KS>
  __device__ __forceinline__ void dst_own(const Frag (&gf)[KS], const XArgs &a) {
    sd = ds_scale_x(own_max_norm2(gf), a.bounds[2] * sq);
    usd = 1.f / sd;
  }
  // source pass: any dO' row (its elements are bounded by the recorded maximum), this wave's V' rows
  template <int KS>
  __device__ __forceinline__ void src_own(const Frag (&vf)[KS], const XArgs &a) {
    sd = ds_scale_x(own_max_norm2(vf), a.bounds[3] * sg);
    usd = 1.f / sd;
  }
  template <int NT>
  __device__ __forceinline__ float softmax(f32x4 (&S)[NT], float mul, int L, int g) const {
    return xh_column_softmax<NT>(S, sc, mul, L, g);
  }
  __device__ __forceinline__ float dst_ds(float x, float) const { return x * sd; }       // dS in the split's units
  __device__ __forceinline__ void src_pds(float s, float lse, float dp, float delta, bool ok, float, float &P, float &dS) const {
    const float pr = ok ? fast_exp2(fmaf(s, sc, -lse)) : 0.f;
    P = pr * kPScale;
    dS = (pr * sd) * (dp - delta);
  }
  __device__ __forceinline__ float o_mul(float x) const { return kPUnscale * uq * x; }
  // partial tiles of a long segment leave in the units the combine pass expects (it applies 1 / sqrt(dh))
  __device__ __forceinline__ float dq_mul(const XArgs &a) const { return part_or(a, a.oscale) * (((uq * uq) * ug) * usd); }
  __device__ __forceinline__ float dk_mul(const XArgs &a) const { return dq_mul(a); }
  __device__ __forceinline__ float dv_mul() const { return kPUnscale * ug; }
};

// ---- bf16 STORAGE (dtype AMPCONV_BF16): the rows are 16-bit already, so a tile is ONE plane copied into LDS as it
// stands and every product is one v_mfma_f32_16x16x32_bf16; softmax weights and dS are rounded to bf16 for their second
// product (the accuracy class of this storage mode: rtol 2e-2; edge_mfma_bf16.hip does the same),
// accumulators, softmax and delta stay fp32.  Nothing is pre-scaled (that would round the operands again): the scores meet
// log2e / sqrt(dh) inside the exponential, 1 / in-degree is applied to dS and to the weights that multiply dObar, and
// delta is handed over in the units of the raw dObar V^T product.  Views: strides in bf16 elements, bases and strides
// even (4-byte pieces) at least.  All channel tiles are read in one group.
struct FmtXB {
  using Elem = unsigned short;
  template <int VEC, int NT, int KS> using Stage = StageB<VEC, NT, KS>;
  template <int KS> using Own = OwnB<KS>;
  static constexpr int kPlanes = 1;
  using Frag = XFrag<1>;
  static constexpr bool kQidx = true, kRecordMax = false, kSrcPairs = true;
  static constexpr float kPScale = 1.f;
  static constexpr int fwd_mcb(int mct) { return mct; }
  static constexpr int dst_mcb(int mct) { return mct; }

  static __device__ __forceinline__ void split(float x0, float x1, int (&w)[1]) { w[0] = cvt_pk_bf16(x0, x1); }
  static __device__ __forceinline__ f32x4 mma(const Frag &a, const Frag &b, f32x4 c) { return MFMA_X3(a.p[0], b.p[0], c); }
  template <int VEC, int MCT>
  static __device__ __forceinline__ float store(const ampconv_view_t &v, int64_t node, int h, const f32x4 (&T)[MCT], float scale,
                                                int tile, int L, int dh, int lane, bool partial) {
    return store_xb<VEC, MCT>(v, node, h, T, scale, tile, L, dh, lane, partial);
  }

  float qscale;
  __device__ __forceinline__ FmtXB(const XArgs &a, bool) : qscale(a.qscale) {}
  __device__ __forceinline__ float q_mul(const XArgs &) const { return 1.f; }            // (the staging is a copy)
  __device__ __forceinline__ float g_mul(float) const { return 1.f; }
  __device__ __forceinline__ float kv_mul() const { return 1.f; }
  template <int KS> __device__ __forceinline__ void dst_own(const Frag (&)[KS], const XArgs &) {}
  template <int KS> __device__ __forceinline__ void src_own(const Frag (&)[KS], const XArgs &) {}
  template <int NT>
  __device__ __forceinline__ float softmax(f32x4 (&S)[NT], float mul, int L, int g) const {
    return xh_column_softmax<NT>(S, qscale, mul, L, g);
  }
  __device__ __forceinline__ float dst_ds(float x, float inv) const { return x * inv; }
  __device__ __forceinline__ void src_pds(float s, float lse, float dp, float delta, bool ok, float inv, float &P, float &dS) const {
    const float pr = ok ? fast_exp2(fmaf(s, qscale, -lse)) * inv : 0.f;      // P / in-degree
    P = pr;
    dS = pr * (dp - delta);
  }
  __device__ __forceinline__ float o_mul(float x) const { return x; }
  __device__ __forceinline__ float dq_mul(const XArgs &a) const { return part_or(a, a.oscale); }
  // (partial tiles of a long column: the combine pass of this family multiplies dK by ln 2 -- its fp32 kernels carry
  // log2e / sqrt(dh) in Q --, so they leave with log2e / sqrt(dh) here)
  __device__ __forceinline__ float dk_mul(const XArgs &a) const { return a.hub.mode == 2 ? a.oscale * kLog2e : a.oscale; }
  __device__ __forceinline__ float dv_mul() const { return 1.f; }
};

// =====================================================================================================================
// The three passes.
// ---------------------------------------------------------------- forward
template <class Fmt, int VEC, int NT, int KS>
__device__ __forceinline__ void fwd_body(const XArgs &a) {
  using Frag = typename Fmt::Frag;
  using Elem = typename Fmt::Elem;
  constexpr int MCT = 2 * KS;                 // 16-channel tiles
  constexpr int MCB = Fmt::fwd_mcb(MCT);      // channel tiles per group of transposed reads
  constexpr int P = Fmt::kPlanes, TB = P * 16 * NT * kRowB, NPAIR = (NT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int64_t r, onode;
  int h, beg, end, deg;
  const int64_t unit = xcd_unit(blockIdx.x, a.n_units, a.H);
  if (unit < 0 || !map_unit(a.hub, a.ptr, unit, a.n_units, a.H, r, onode, h, beg, end, deg)) return;
  const int L = a.L, dh = a.dh, g = lane >> 4;
  char *Kt = lds, *Vt = lds + TB;
  int64_t d = r;
  if constexpr (Fmt::kQidx) d = a.qidx ? a.qidx[r] : r;
  const Fmt f(a, false);

  IdxWindow win;
  if (beg < end) idxwin_load<false>(win, a.idx, nullptr, beg, end, lane);      // (first: everything else waits for it)
  typename Fmt::template Own<KS> qraw;
  own_load(qraw, tile_of<Elem>(a.Q, d, h), (int)a.Q.row_stride, wave, L, dh, lane);
  f32x4 OT[MCT];
#pragma unroll
  for (int mc = 0; mc < MCT; ++mc) OT[mc] = f32x4{0.f, 0.f, 0.f, 0.f};
  const FragAddr fa = frag_addr(lane);
  StageOffs<VEC, NT, KS> lo;
  stage_offsets<VEC, NT, KS>(lo, tid);

  typename Fmt::template Stage<VEC, NT, KS> st;
  const StageSrc sq = stage_src<sizeof(Elem), VEC, NT, KS>((int)a.K.row_stride, (int)a.V.row_stride, L, dh, tid);
  auto fetch = [&](int p) {
    const int64_t s = idxwin_get<false>(win, a.idx, nullptr, p, end, lane, nullptr);
    stage_load(st, tile_of<Elem>(a.K, s, h), tile_of<Elem>(a.V, s, h), sq, L);
  };
  if (beg < end) fetch(beg);
  lds_zero_tail<VEC, NT, KS, 2 * P>(lds, L, tid);
  Frag qf[KS];
  own_split<Fmt>(qf, qraw, f.q_mul(a));
  __syncthreads();
  for (int p = beg; p < end; ++p) {
    stage_store<Fmt>(Kt, Vt, st, lo, f.kv_mul(), f.kv_mul(), L);
#ifndef AMPCONV_X3_NOLOADS          // developer probe: the first edge's tiles again and again (what does the compute side cost?)
    if (p + 1 < end) fetch(p + 1);
#endif
    __syncthreads();

#ifdef AMPCONV_X3_NOCOMPUTE          // developer probe: staging, LDS images and barriers only (what does the memory side cost?)
    OT[0][0] += *reinterpret_cast<const float *>(Kt + 4 * tid) + *reinterpret_cast<const float *>(Vt + 4 * tid);
    __syncthreads();
    continue;
#endif
    f32x4 S[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      S[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) S[t] = Fmt::mma(rowfrag<P, NT>(Kt, fa.a[ks], t), qf[ks], S[t]);
    }
    f.template softmax<NT>(S, Fmt::kPScale, L, g);
    Frag pf[NPAIR];
#pragma unroll
    for (int mb = 0; mb < MCT / MCB; ++mb) {                  // MCB channel tiles per group of transposed reads
      TR_WAR_GUARD();
      Frag vc[MCB][NPAIR];
#pragma unroll
      for (int u = 0; u < MCB; ++u)
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) vc[u][i] = colfrag<P, NT>(Vt, fa.tr[MCB * mb + u], i);
      if (mb == 0) {
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) pf[i] = cd_frag<Fmt, NT>(S, i);      // (in the shadow of the reads)
      }
      TR_FRAG_FENCE();
#pragma unroll
      for (int u = 0; u < MCB; ++u)
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) OT[MCB * mb + u] = Fmt::mma(vc[u][i], pf[i], OT[MCB * mb + u]);
    }
    __syncthreads();
  }
  // hub pass: unnormalised partial tile, the combine pass applies 1/deg
  Fmt::template store<VEC, MCT>(a.O, onode, h, OT, f.o_mul(a.hub.mode == 2 ? 1.f : (deg > 0 ? 1.f / (float)deg : 0.f)), wave, L,
                                dh, lane, a.hub.mode == 2);
}

// ---------------------------------------------------------------- backward, destination pass
template <class Fmt, int VEC, bool STATS, int NT, int KS>
__device__ __forceinline__ void bwd_dst_body(const XArgs &a) {
  using Frag = typename Fmt::Frag;
  using Elem = typename Fmt::Elem;
  constexpr int MCT = 2 * KS;
  constexpr int MCB = Fmt::dst_mcb(MCT);
  constexpr int P = Fmt::kPlanes, TB = P * 16 * NT * kRowB, NPAIR = (NT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int64_t r, onode;
  int h, beg, end, deg;
  const int64_t unit = xcd_unit(blockIdx.x, a.n_units, a.H);
  if (unit < 0 || !map_unit(a.hub, a.ptr, unit, a.n_units, a.H, r, onode, h, beg, end, deg)) return;
  const int L = a.L, dh = a.dh, g = lane >> 4;
  char *Kt = lds, *Vt = lds + TB;
  const float inv = deg > 0 ? 1.f / (float)deg : 0.f;       // dO is the gradient of the MEAN
  Fmt f(a, true);       // (with the scale of dObar)

  IdxWindow win;
  const float *wts = reinterpret_cast<const float *>(a.spos);
  if (beg < end) idxwin_load<STATS>(win, a.idx, wts, beg, end, lane);
  typename Fmt::template Own<KS> qraw, graw;
  own_load(qraw, tile_of<Elem>(a.Q, r, h), (int)a.Q.row_stride, wave, L, dh, lane);
  own_load(graw, tile_of<Elem>(a.dO, r, h), (int)a.dO.row_stride, wave, L, dh, lane);
  f32x4 dQT[MCT];
#pragma unroll
  for (int mc = 0; mc < MCT; ++mc) dQT[mc] = f32x4{0.f, 0.f, 0.f, 0.f};
  const FragAddr fa = frag_addr(lane);
  StageOffs<VEC, NT, KS> lo;
  stage_offsets<VEC, NT, KS>(lo, tid);

  typename Fmt::template Stage<VEC, NT, KS> st;
  float pos_next = 0.f;                      // STATS: CSC position (int bits) in the window's weight slot
  const StageSrc sq = stage_src<sizeof(Elem), VEC, NT, KS>((int)a.K.row_stride, (int)a.V.row_stride, L, dh, tid);
  auto fetch = [&](int p) {
    const int64_t s = idxwin_get<STATS>(win, a.idx, wts, p, end, lane, &pos_next);
    stage_load(st, tile_of<Elem>(a.K, s, h), tile_of<Elem>(a.V, s, h), sq, L);
  };
  if (beg < end) fetch(beg);
  lds_zero_tail<VEC, NT, KS, 2 * P>(lds, L, tid);
  Frag qf[KS], gf[KS];
  own_split<Fmt>(qf, qraw, f.q_mul(a));
  own_split<Fmt>(gf, graw, f.g_mul(inv));
  f.dst_own(gf, a);
  __syncthreads();
  constexpr int LS = 16 * NT;
  for (int p = beg; p < end; ++p) {
    stage_store<Fmt>(Kt, Vt, st, lo, f.kv_mul(), f.kv_mul(), L);
    float *sb = nullptr;
    if (STATS) sb = a.stats + ((int64_t)__builtin_bit_cast(int, pos_next) * a.H + h) * (2 * LS);
    if (p + 1 < end) fetch(p + 1);
    __syncthreads();

    f32x4 S[NT], dP[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      S[t] = dP[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        S[t] = Fmt::mma(rowfrag<P, NT>(Kt, fa.a[ks], t), qf[ks], S[t]);
        dP[t] = Fmt::mma(rowfrag<P, NT>(Vt, fa.a[ks], t), gf[ks], dP[t]);
      }
    }
    const float lse = f.template softmax<NT>(S, 1.f, L, g);
    float part = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int q = 0; q < 4; ++q) part = fmaf(S[t][q], dP[t][q], part);
    }
    const float delta = groups_sum(part);    // (in the units of this format's dObar V^T product)
    if (STATS && g == 0) {                   // all LS columns: the source pass reads every one
      sb[(lane & 15) + 16 * wave] = lse;
      sb[LS + (lane & 15) + 16 * wave] = delta;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int q = 0; q < 4; ++q) S[t][q] *= f.dst_ds(dP[t][q] - delta, inv);       // dS
    }
    Frag sf[NPAIR];
#pragma unroll
    for (int mb = 0; mb < MCT / MCB; ++mb) {
      TR_WAR_GUARD();
      Frag kc[MCB][NPAIR];
#pragma unroll
      for (int u = 0; u < MCB; ++u)
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) kc[u][i] = colfrag<P, NT>(Kt, fa.tr[MCB * mb + u], i);
      if (mb == 0) {
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) sf[i] = cd_frag<Fmt, NT>(S, i);
      }
      TR_FRAG_FENCE();
#pragma unroll
      for (int u = 0; u < MCB; ++u)
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) dQT[MCB * mb + u] = Fmt::mma(kc[u][i], sf[i], dQT[MCB * mb + u]);
    }
    __syncthreads();
  }
  const float mx = Fmt::template store<VEC, MCT>(a.O, onode, h, dQT, f.dq_mul(a), wave, L, dh, lane, a.hub.mode == 2);
  if constexpr (Fmt::kRecordMax)
    if (a.absmax) wave_record_absmax(a.absmax, mx);
}

// ---------------------------------------------------------------- backward, source pass (needs the statistics)
template <class Fmt, int VEC, int NT, int KS>
__device__ __forceinline__ void bwd_src_body(const XArgs &a) {
  using Frag = typename Fmt::Frag;
  using Elem = typename Fmt::Elem;
  constexpr int MCT = 2 * KS;
  constexpr int P = Fmt::kPlanes, TB = P * 16 * NT * kRowB, NPAIR = (NT + 1) / 2;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int64_t s, onode;
  int h, beg, end, deg;
  const int64_t unit = xcd_unit(blockIdx.x, a.n_units, a.H);
  if (unit < 0 || !map_unit(a.hub, a.ptr, unit, a.n_units, a.H, s, onode, h, beg, end, deg)) return;
  const int L = a.L, dh = a.dh, g = lane >> 4, n = lane & 15;
  char *Qt = lds, *Gt = lds + TB;
  Fmt f(a, true);       // (with the scale of dObar)

  IdxWindow win;
  if (beg < end) idxwin_load<true>(win, a.idx, a.cinv, beg, end, lane);
  typename Fmt::template Own<KS> kraw, vraw;
  own_load(kraw, tile_of<Elem>(a.K, s, h), (int)a.K.row_stride, wave, L, dh, lane);
  own_load(vraw, tile_of<Elem>(a.V, s, h), (int)a.V.row_stride, wave, L, dh, lane);
  f32x4 dKT[MCT], dVT[MCT];
#pragma unroll
  for (int mc = 0; mc < MCT; ++mc) dKT[mc] = dVT[mc] = f32x4{0.f, 0.f, 0.f, 0.f};
  const FragAddr fa = frag_addr(lane);
  StageOffs<VEC, NT, KS> lo;
  stage_offsets<VEC, NT, KS>(lo, tid);

  typename Fmt::template Stage<VEC, NT, KS> st;
  float inv_next = 0.f;
  // the edge's softmax statistics (2 LS floats, written by the destination pass at this CSC position) travel with its
  // tiles: one float per thread, requested an edge ahead and handed to the waves through LDS
  constexpr int LS = 16 * NT;
  float *sl = reinterpret_cast<float *>(lds + 2 * TB);
  float stat_next = 0.f;
  const StageSrc sq = stage_src<sizeof(Elem), VEC, NT, KS>((int)a.Q.row_stride, (int)a.dO.row_stride, L, dh, tid);
  auto fetch = [&](int p) {
    const int64_t d = idxwin_get<true>(win, a.idx, a.cinv, p, end, lane, &inv_next);
    if (tid < 2 * LS) stat_next = a.stats[((int64_t)p * a.H + h) * (2 * LS) + tid];
    stage_load(st, tile_of<Elem>(a.Q, d, h), tile_of<Elem>(a.dO, d, h), sq, L);
  };
  if (beg < end) fetch(beg);
  lds_zero_tail<VEC, NT, KS, 2 * P>(lds, L, tid);
  Frag kf[KS], vf[KS];
  own_split<Fmt>(kf, kraw, f.kv_mul());
  own_split<Fmt>(vf, vraw, f.kv_mul());
  f.src_own(vf, a);
  __syncthreads();
  const bool colok = n + 16 * wave < L;      // this lane's source token exists
  for (int p = beg; p < end; ++p) {
    const float inv = inv_next;              // 1 / in-degree of THIS edge's destination (fetch overwrites inv_next)
    stage_store<Fmt>(Qt, Gt, st, lo, f.q_mul(a), f.g_mul(inv), L);
    if (tid < 2 * LS) sl[tid] = stat_next;
    if (p + 1 < end) fetch(p + 1);
    __syncthreads();

    // weights and dS of destination-token tile t (tokens 16 t + 4 g + q), in the split's units
    auto tile_pds = [&](int t, f32x4 &Pt, f32x4 &dSt) __attribute__((always_inline)) {
      const f32x4 l4 = *reinterpret_cast<const f32x4 *>(sl + 16 * t + 4 * g);
      const f32x4 d4 = *reinterpret_cast<const f32x4 *>(sl + LS + 16 * t + 4 * g);
      f32x4 S = f32x4{0.f, 0.f, 0.f, 0.f}, dP = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        S = Fmt::mma(rowfrag<P, NT>(Qt, fa.a[ks], t), kf[ks], S);
        dP = Fmt::mma(rowfrag<P, NT>(Gt, fa.a[ks], t), vf[ks], dP);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float pw, ds;
        f.src_pds(S[q], l4[q], dP[q], d4[q], colok, inv, pw, ds);
        Pt[q] = pw;
        dSt[q] = ds;
      }
    };
    if constexpr (Fmt::kSrcPairs) {
      // one pair of destination-token tiles at a time: scores, weights and their split live for one pair only (registers:
      // three waves per SIMD), at the price of a group of transposed reads per (pair, channel tile)
#pragma unroll
      for (int i = 0; i < NPAIR; ++i) {
        f32x4 Pw[2], dS[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          Pw[u] = dS[u] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (2 * i + u < NT) tile_pds(2 * i + u, Pw[u], dS[u]);
        }
        Frag pf, sf;
#pragma unroll
        for (int mc = 0; mc < MCT; ++mc) {
          TR_WAR_GUARD();
          const Frag gc = colfrag<P, NT>(Gt, fa.tr[mc], i), qc = colfrag<P, NT>(Qt, fa.tr[mc], i);
          if (mc == 0) {
            pf = cd_frag<Fmt, 2>(Pw, 0);
            sf = cd_frag<Fmt, 2>(dS, 0);
          }
          TR_FRAG_FENCE();
          dVT[mc] = Fmt::mma(gc, pf, dVT[mc]);
          dKT[mc] = Fmt::mma(qc, sf, dKT[mc]);
        }
      }
    } else {
      // all destination-token tiles at once: one group of transposed reads per channel tile
      f32x4 Pw[NT], dS[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) tile_pds(t, Pw[t], dS[t]);
      Frag pf[NPAIR], sf[NPAIR];
#pragma unroll
      for (int mc = 0; mc < MCT; ++mc) {
        TR_WAR_GUARD();
        Frag gc[NPAIR], qc[NPAIR];
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) {
          gc[i] = colfrag<P, NT>(Gt, fa.tr[mc], i);
          qc[i] = colfrag<P, NT>(Qt, fa.tr[mc], i);
        }
        if (mc == 0) {
#pragma unroll
          for (int i = 0; i < NPAIR; ++i) {
            pf[i] = cd_frag<Fmt, NT>(Pw, i);
            sf[i] = cd_frag<Fmt, NT>(dS, i);
          }
        }
        TR_FRAG_FENCE();
#pragma unroll
        for (int i = 0; i < NPAIR; ++i) {
          dVT[mc] = Fmt::mma(gc[i], pf[i], dVT[mc]);
          dKT[mc] = Fmt::mma(qc[i], sf[i], dKT[mc]);
        }
      }
    }
    __syncthreads();
  }
  const bool partial = a.hub.mode == 2;
  float mx = Fmt::template store<VEC, MCT>(a.dK, onode, h, dKT, f.dk_mul(a), wave, L, dh, lane, partial);
  mx = fmaxf(mx, Fmt::template store<VEC, MCT>(a.dV, onode, h, dVT, f.dv_mul(), wave, L, dh, lane, partial));
  if constexpr (Fmt::kRecordMax)
    if (a.absmax) wave_record_absmax(a.absmax, mx);
}

// =====================================================================================================================
// The nine kernels: names (profiles, tests/test_abi.py) and launch bounds (minimum waves per SIMD) of their own.
#ifndef AMPCONV_X3_FWD_WAVES
#define AMPCONV_X3_FWD_WAVES 3
#endif
#ifndef AMPCONV_X3_DST_WAVES
#define AMPCONV_X3_DST_WAVES 2
#endif
#ifndef AMPCONV_X3_SRC_WAVES
#define AMPCONV_X3_SRC_WAVES 2
#endif
#ifndef AMPCONV_XH_FWD_WAVES
#define AMPCONV_XH_FWD_WAVES 4
#endif
#ifndef AMPCONV_XH_DST_WAVES
#define AMPCONV_XH_DST_WAVES 3
#endif
#ifndef AMPCONV_XH_SRC_WAVES
#define AMPCONV_XH_SRC_WAVES 3
#endif
template <int VEC, int NT, int KS>
__global__ __launch_bounds__(64 * NT, AMPCONV_X3_FWD_WAVES) void fwd_x3(XArgs a) { fwd_body<FmtX3, VEC, NT, KS>(a); }
template <int VEC, bool STATS, int NT, int KS>
__global__ __launch_bounds__(64 * NT, AMPCONV_X3_DST_WAVES) void bwd_dst_x3(XArgs a) { bwd_dst_body<FmtX3, VEC, STATS, NT, KS>(a); }
template <int VEC, int NT, int KS>
__global__ __launch_bounds__(64 * NT, AMPCONV_X3_SRC_WAVES) void bwd_src_x3(XArgs a) { bwd_src_body<FmtX3, VEC, NT, KS>(a); }

template <int VEC, int NT, int KS>
__global__ __launch_bounds__(64 * NT, AMPCONV_XH_FWD_WAVES) void fwd_xh(XArgs a) { fwd_body<FmtXH, VEC, NT, KS>(a); }
template <int VEC, bool STATS, int NT, int KS>
__global__ __launch_bounds__(64 * NT, AMPCONV_XH_DST_WAVES) void bwd_dst_xh(XArgs a) { bwd_dst_body<FmtXH, VEC, STATS, NT, KS>(a); }
template <int VEC, int NT, int KS>
__global__ __launch_bounds__(64 * NT, AMPCONV_XH_SRC_WAVES) void bwd_src_xh(XArgs a) { bwd_src_body<FmtXH, VEC, NT, KS>(a); }

template <int EV, int NT, int KS>             // EV = bf16 elements per lane and load (2 or 4)
__global__ __launch_bounds__(64 * NT, 4) void fwd_xb(XArgs a) { fwd_body<FmtXB, EV, NT, KS>(a); }
template <int EV, bool STATS, int NT, int KS>
__global__ __launch_bounds__(64 * NT, 3) void bwd_dst_xb(XArgs a) { bwd_dst_body<FmtXB, EV, STATS, NT, KS>(a); }
template <int EV, int NT, int KS>
__global__ __launch_bounds__(64 * NT, 3) void bwd_src_xb(XArgs a) { bwd_src_body<FmtXB, EV, NT, KS>(a); }

// ---------------------------------------------------------------------------------------------------------------------
// Host side
typedef void (*X3Kernel)(XArgs);
enum XFmt { kX3, kXH, kXB };
struct XFmtInfo {
  int planes, esize;        // plane images per tile, bytes per stored element
};
template <class Fmt>
constexpr XFmtInfo fmt_info() { return {Fmt::kPlanes, (int)sizeof(typename Fmt::Elem)}; }
constexpr XFmtInfo kFmtInfo[3] = {fmt_info<FmtX3>(), fmt_info<FmtXH>(), fmt_info<FmtXB>()};      // by XFmt
enum XPass { kFwd, kDst, kDstStats, kSrc };

template <int VEC, int NT, int KS>
X3Kernel x3_kernel(XFmt fmt, XPass pass) {
  static const X3Kernel k[3][4] = {
      {fwd_x3<VEC, NT, KS>, bwd_dst_x3<VEC, false, NT, KS>, bwd_dst_x3<VEC, true, NT, KS>, bwd_src_x3<VEC, NT, KS>},
      {fwd_xh<VEC, NT, KS>, bwd_dst_xh<VEC, false, NT, KS>, bwd_dst_xh<VEC, true, NT, KS>, bwd_src_xh<VEC, NT, KS>},
      {fwd_xb<VEC, NT, KS>, bwd_dst_xb<VEC, false, NT, KS>, bwd_dst_xb<VEC, true, NT, KS>, bwd_src_xb<VEC, NT, KS>}};
  return k[fmt][pass];
}
template <int KS>
X3Kernel x3_pick_ks(XFmt fmt, XPass pass, int vec, int ntok) {
  switch (ntok) {
    case 1: return vec == 4 ? x3_kernel<4, 1, KS>(fmt, pass) : x3_kernel<2, 1, KS>(fmt, pass);
    case 2: return vec == 4 ? x3_kernel<4, 2, KS>(fmt, pass) : x3_kernel<2, 2, KS>(fmt, pass);
    case 3: return vec == 4 ? x3_kernel<4, 3, KS>(fmt, pass) : x3_kernel<2, 3, KS>(fmt, pass);
    default: return vec == 4 ? x3_kernel<4, 4, KS>(fmt, pass) : x3_kernel<2, 4, KS>(fmt, pass);
  }
}

// the widest vector (4 or 2 elements of esize bytes) that every view's base and strides allow
int vec_of(const ampconv_view_t *views, int n, int dh, int esize) {
  int vec = dh % 4 == 0 ? 4 : 2;
  for (int i = 0; i < n; ++i) {
    const ampconv_view_t &v = views[i];
    while (vec > 1 && (((uintptr_t)v.ptr % (esize * vec)) || v.node_stride % vec || v.row_stride % vec ||
                       v.head_stride % vec))
      vec >>= 1;
  }
  return vec;
}

// what a launch takes from the shape and the format: the kernel arguments that follow from them (the caller fills in
// its views and index arrays), the template parameters, the LDS bytes
struct XLaunch {
  XArgs a{};
  XFmt fmt;
  XLaunch(XFmt fmt, int64_t n_rows, int L, int D, int H) : fmt(fmt) {
    a.L = L; a.dh = D / H; a.H = H;
    a.n_units = n_rows * H;
    a.qscale = kLog2e / sqrtf((float)a.dh);
  }
  // `views`: every view the kernel touches (they decide the vector width)
  int run(XPass pass, const ampconv_view_t *views, int n, hipStream_t stream) const {
    const int64_t nb = xcd_grid(a.n_units, a.H);
    if (nb > INT32_MAX) return AMPCONV_E_BADARG;
    const int ntok = (a.L + 15) / 16, ks = a.dh > 32 ? 2 : 1;      // ks = k-steps of 32 channels
    const int vec = vec_of(views, n, a.dh, kFmtInfo[fmt].esize), planes = kFmtInfo[fmt].planes;
    const X3Kernel k = ks == 1 ? x3_pick_ks<1>(fmt, pass, vec, ntok) : x3_pick_ks<2>(fmt, pass, vec, ntok);
    // two tiles of `planes` images, and the source pass's statistics hand-off
    const size_t shmem = (size_t)2 * planes * 16 * ntok * kRowB + (pass == kSrc ? 2 * 16 * ntok * sizeof(float) : 0);
    hipLaunchKernelGGL(k, dim3((unsigned)nb), dim3(64 * ntok), shmem, stream, a);
    return ampconv_launch_status();
  }
};
}  // namespace

bool ampconv_block_supported(int L, int D, int H, const ampconv_view_t *views, int n, bool bf16) {
  const int dh = D / H;
  if (!(L >= 1 && L <= 64 && dh >= 2 && dh <= 64 && dh % 2 == 0)) return false;
  return vec_of(views, n, dh, kFmtInfo[bf16 ? kXB : kX3].esize) >= 2;
}

int ampconv_block_stats_floats(int L) { return 2 * 16 * ((L + 15) / 16); }

int ampconv_fwd_edge_block(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, const int32_t *rowptr,
                           const int32_t *col, const int32_t *qidx, int64_t n_rows, int L, int D, int H,
                           ampconv_view_t O, HubArgs hub, bool bf16, hipStream_t stream) {
  XLaunch x(bf16 ? kXB : kX3, n_rows, L, D, H);
  XArgs &a = x.a;
  a.hub = hub;
  a.Q = Q; a.K = K; a.V = V; a.O = O;
  a.ptr = rowptr; a.idx = col; a.qidx = qidx;
  const ampconv_view_t views[] = {Q, K, V, O};
  return x.run(kFwd, views, 4, stream);
}

int ampconv_bwd_edge_dst_block(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dO,
                               const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D, int H,
                               ampconv_view_t dQ, HubArgs hub, StatsArgs sa, bool bf16, hipStream_t stream) {
  XLaunch x(bf16 ? kXB : kX3, n_rows, L, D, H);
  XArgs &a = x.a;
  a.hub = hub;
  a.Q = Q; a.K = K; a.V = V; a.dO = dO; a.O = dQ;
  a.ptr = rowptr; a.idx = col; a.spos = sa.spos; a.stats = sa.stats;
  a.oscale = 1.f / sqrtf((float)a.dh);
  const ampconv_view_t views[] = {Q, K, V, dO, dQ};
  return x.run(sa.stats ? kDstStats : kDst, views, 5, stream);
}

int ampconv_bwd_edge_src_block(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dO,
                               const int32_t *cscptr, const int32_t *crow, const float *cinv, int64_t n_src,
                               int L, int D, int H, ampconv_view_t dK, ampconv_view_t dV, HubArgs hub,
                               const float *stats, bool bf16, hipStream_t stream) {
  if (!stats) return AMPCONV_E_BADARG;
  XLaunch x(bf16 ? kXB : kX3, n_src, L, D, H);
  XArgs &a = x.a;
  a.hub = hub;
  a.Q = Q; a.K = K; a.V = V; a.dO = dO; a.dK = dK; a.dV = dV;
  a.ptr = cscptr; a.idx = crow; a.cinv = cinv; a.stats = const_cast<float *>(stats);
  // fp32: dK = ln2 * sum dS^T (Q * log2e / sqrt(dh)); bf16: Q enters unscaled, dK = sum dS^T Q / sqrt(dh)
  a.oscale = bf16 ? 1.f / sqrtf((float)a.dh) : 0.6931471805599453f;
  const ampconv_view_t views[] = {Q, K, V, dO, dK, dV};
  return x.run(kSrc, views, 6, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// C-ABI of the scaled kernels (include/ampconv.h, "edge phase on fp32 views with operand bounds")
namespace {
int x3_check(int64_t n, int L, int D, int H, const float *bounds) {
  if (L <= 0 || D <= 0 || H <= 0 || D % H != 0 || n < 0 || !bounds) return AMPCONV_E_BADARG;
  if (!ampconv_scaled_supported(L, D, H)) return AMPCONV_E_DTYPE;
  return AMPCONV_OK;
}
// views of two-float vectors at least: rows, heads and nodes an even number of elements apart, 8-byte aligned base
bool x3_views_ok(const ampconv_view_t *views, int n, int dh) {
  for (int i = 0; i < n; ++i)
    if (!view_ok(views[i])) return false;
  return vec_of(views, n, dh, kFmtInfo[kXH].esize) >= 2;
}
}  // namespace

extern "C" int ampconv_scaled_supported(int L, int D, int H) {
  if (L < 1 || D < 1 || H < 1 || D % H != 0) return 0;
  const int dh = D / H;
  if (L <= 20 && (dh == 32 || dh == 16)) return 0;      // the one-wave-per-unit kernels' shapes (plane format / edge_mfma.hip)
  return L <= 64 && dh >= 2 && dh <= 64 && dh % 2 == 0;
}

extern "C" int ampconv_fwd_edge_scaled(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, const int32_t *rowptr,
                                       const int32_t *col, int64_t n_rows, int L, int D, int H, ampconv_view_t O,
                                       const void *hub_plan, int64_t hub_chunks, void *hub_ws, const float *bounds,
                                       void *stream) {
  if (int rc = x3_check(n_rows, L, D, H, bounds)) return rc;
  if (n_rows == 0) return AMPCONV_OK;
  const ampconv_view_t views[] = {Q, K, V, O};
  if (!x3_views_ok(views, 4, D / H) || !rowptr) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  XLaunch x(kXH, n_rows, L, D, H);
  XArgs &a = x.a;
  a.Q = Q; a.K = K; a.V = V;
  a.ptr = rowptr; a.idx = col; a.bounds = bounds;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *) {
    const ampconv_view_t v[] = {Q, K, V, o[0]};
    a.hub = hub; a.n_units = n * H; a.O = o[0];
    return x.run(kFwd, v, 4, st);
  };
  return run_edge_pass(run, n_rows, {O}, hub_plan, hub_chunks, hub_ws, L, D, H, rowptr, {1.f}, 0, nullptr, st);
}

extern "C" int ampconv_bwd_edge_dst_scaled(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                                           const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D, int H,
                                           ampconv_view_t dQ, const void *hub_plan, int64_t hub_chunks, void *hub_ws,
                                           const float *bounds, const int32_t *spos, float *stats, float *out_absmax,
                                           void *stream) {
  if (int rc = x3_check(n_rows, L, D, H, bounds)) return rc;
  if (stats && (!spos || (uintptr_t)stats % 16 != 0)) return AMPCONV_E_BADARG;
  if (n_rows == 0) return AMPCONV_OK;
  const ampconv_view_t views[] = {Q, K, V, dObar, dQ};
  if (!x3_views_ok(views, 5, D / H) || !rowptr) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  XLaunch x(kXH, n_rows, L, D, H);
  XArgs &a = x.a;
  a.Q = Q; a.K = K; a.V = V; a.dO = dObar;
  a.ptr = rowptr; a.idx = col; a.bounds = bounds;
  a.spos = spos; a.stats = stats;
  a.oscale = 1.f / sqrtf((float)a.dh);
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *absmax) {
    const ampconv_view_t v[] = {Q, K, V, dObar, o[0]};
    a.hub = hub; a.n_units = n * H; a.O = o[0]; a.absmax = absmax;
    return x.run(stats ? kDstStats : kDst, v, 5, st);
  };
  return run_edge_pass(run, n_rows, {dQ}, hub_plan, hub_chunks, hub_ws, L, D, H, nullptr, {a.oscale}, 0, out_absmax,
                       st);
}

extern "C" int ampconv_bwd_edge_src_scaled(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                                           const int32_t *cscptr, const int32_t *crow, const float *cinv, int64_t n_src,
                                           int L, int D, int H, ampconv_view_t dK, ampconv_view_t dV, const void *hub_plan,
                                           int64_t hub_chunks, void *hub_ws, const float *bounds, const float *stats,
                                           float *out_absmax, void *stream) {
  if (int rc = x3_check(n_src, L, D, H, bounds)) return rc;
  if (!stats || (uintptr_t)stats % 16 != 0 || !cinv) return AMPCONV_E_BADARG;      // this pass exists only with the hand-off
  if (n_src == 0) return AMPCONV_OK;
  const ampconv_view_t views[] = {Q, K, V, dObar, dK, dV};
  if (!x3_views_ok(views, 6, D / H) || !cscptr) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  XLaunch x(kXH, n_src, L, D, H);
  XArgs &a = x.a;
  a.Q = Q; a.K = K; a.V = V; a.dO = dObar;
  a.ptr = cscptr; a.idx = crow; a.cinv = cinv; a.bounds = bounds;
  a.stats = const_cast<float *>(stats);
  a.oscale = 1.f / sqrtf((float)a.dh);
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *absmax) {
    const ampconv_view_t v[] = {Q, K, V, dObar, o[0], o[1]};
    a.hub = hub; a.n_units = n * H; a.dK = o[0]; a.dV = o[1]; a.absmax = absmax;
    return x.run(kSrc, v, 6, st);
  };
  return run_edge_pass(run, n_src, {dK, dV}, hub_plan, hub_chunks, hub_ws, L, D, H, nullptr, {a.oscale, 1.f}, 0,
                       out_absmax, st);
}
