// The 16-bit plane format, once: how fp32 tensors travel between the projections (proj_gemm*.hip) and the edge kernels
// (edge_mfma_bf16.hip, edge_mfma_f16x2.hip, edge_block_x3.hip) as bf16 / fp16 planes, how a plane image lies in LDS and
// how MFMA fragments are read back from it -- with the fences those reads need.
#pragma once
#include "mfma_tile.h"

namespace plane16 {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr float kLog2e = 1.4426950408889634f;

__device__ __forceinline__ int cvt_pk_bf16(float a, float b) {      // v_cvt_pk_bf16_f32 (RNE)
  f32x2 v = {a, b};
  return __builtin_bit_cast(int, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ int cvt_pk_f16(float a, float b) {       // v_cvt_pk_f16_f32 (RNE)
  f32x2 v = {a, b};
  return __builtin_bit_cast(int, __builtin_convertvector(v, f16x2));
}

// scale of a tensor whose magnitudes are bounded by `bound` (its largest finite magnitude, ampconv_absmax, or an a-priori
// bound, ampconv_proj_out_bound): 2^(14 - floor(log2 bound)), so that the scaled maximum lies in [2^14, 2^15) (fp16: finite
// below 2^16); exponent field clamped to [15, 254] (zero / subnormal bounds take 2^126, a non-finite one -- never produced
// by ampconv_absmax -- 2^-113).  Both sides of a hand-off must derive the same power of two: the projection that writes
// planes and the edge kernel that reads them, the weight image and the kernel that undoes its scale, all call THIS.
__device__ __forceinline__ float plane_scale(float bound) {
  int e = (int)((__builtin_bit_cast(unsigned, bound) >> 23) & 0xFFu);
  e = e < 15 ? 15 : (e > 254 ? 254 : e);
  return __builtin_bit_cast(float, (unsigned)(268 - e) << 23);
}
__device__ __forceinline__ float plane_unscale(float bound) { return 1.f / plane_scale(bound); }     // exact: a power of two

// the two-plane fp16 split of (x0, x1), already scaled, |x| < 2^16: h = the packed hi pair, l = the packed lo pair of the
// remainder (x ~ hi + lo to 2^-22 |x|; the remainder is an exact fp32 difference)
__device__ __forceinline__ void split2(float x0, float x1, int &h, int &l) {
  h = cvt_pk_f16(x0, x1);
  const f16x2 hv = __builtin_bit_cast(f16x2, h);
  l = cvt_pk_f16(x0 - (float)hv[0], x1 - (float)hv[1]);
}

// sum of squares of the 8 fp16 values of a fragment register quadruple (v_dot2_f32_f16)
__device__ __forceinline__ float frag_sumsq(const i32x4 &f) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const f16x2 v = __builtin_bit_cast(f16x2, f[k]);
    s = __builtin_amdgcn_fdot2(v, v, s, false);
  }
  return s;
}

// ds_read_b64_tr_b16: one transposing 8-byte LDS read (4 rows x 16 columns of a row-major 16-bit image per 16 lanes,
// delivered column-major); two of them = one MFMA operand fragment whose 8 consecutive k per lane are ROWS of the image
__device__ __forceinline__ i32x2 tr_half(const char *p) {
  return __builtin_bit_cast(i32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)p));
}
__device__ __forceinline__ i32x4 tr_frag(const char *p0, const char *p1) {
  const i32x2 ai = tr_half(p0), bi = tr_half(p1);
  return i32x4{ai[0], ai[1], bi[0], bi[1]};
}

// The fences of the transposed reads.  Every transposed fragment of a product group is in its registers before the
// group's first MFMA issues, and no transposed read is scheduled in among the MFMAs: the interleaved schedule hipcc picks
// by itself -- an MFMA's operand register redefined by the next ds_read_b64_tr_b16 right behind it, consumed right behind
// the wait -- gave WRONG weight-gradient sums in 7-100 % of the launches of the masked product (one 16-bit element of a
// fragment stale), with the fence 0 of 1 600.  The edge kernels never showed it (thousands of bitwise
// identical repeated steps); at 4-6 waves per SIMD the wait costs nothing measurable, so they carry the fence too.
// tests/test_abi.py scans the shipped ISA for both patterns (tools/scan_tr_hazard.py --gate).
#define TR_FRAG_FENCE()                                    \
  do {                                                     \
    __builtin_amdgcn_sched_barrier(0);                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     \
    __builtin_amdgcn_sched_barrier(0);                     \
  } while (0)
// ... the weight-gradient kernels' form: + 16 idle cycles behind the wait
#define TR_FRAG_FENCE_IDLE()                                                          \
  do {                                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                \
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 7\n\ts_nop 7" ::: "memory");          \
    __builtin_amdgcn_sched_barrier(0);                                                \
  } while (0)
// behind a group of MFMAs whose fragment registers the next group's transposed reads may take over: the last MFMA has
// fetched its operands before a read redefines them (8 idle cycles; gate rule WAR)
#define TR_WAR_GUARD()                         \
  do {                                         \
    __builtin_amdgcn_sched_barrier(0);         \
    asm volatile("s_nop 7" ::: "memory");      \
    __builtin_amdgcn_sched_barrier(0);         \
  } while (0)
// in front of a group of transposed reads that follows MFMAs of another phase (their fragment registers may be taken
// over): eight idle cycles and a compiler barrier for memory operations only -- the vector work around it still moves
#define TR_PRE_READ() asm volatile("s_nop 7" ::: "memory")

// ---- the swizzled LDS image of one plane of a 20-token tile with 64-byte token rows (32 channels of 16 bits; the
// one-wave-per-unit kernels of edge_mfma_bf16.hip and, per plane, edge_mfma_f16x2.hip): conflict-free ds_write_b128,
// ds_read_b128 and transposed reads
constexpr int kPlaneRowBytes = 64;
// byte offset of 16-byte chunk `ch` (0..3) of token row `j`
__device__ __forceinline__ int plane_off(int j, int ch) {
  const int f = (4 - (j >> 2)) & 3;
  return j * kPlaneRowBytes + ((ch ^ f) << 4);
}
// channel-product fragment of row tile mt.  Tile 1 uses the quarter map of mfma_tile.h: MFMA row m <-> token
// 16 + (m >> 2), so in C/D layout lane group g holds token 16 + g in reg 0
__device__ __forceinline__ i32x4 rowfrag(const char *img, int mt, int lane) {
  const int m = lane & 15, kg = lane >> 4;
  const int j = mt == 0 ? m : 16 + (m >> 2);
  return *reinterpret_cast<const i32x4 *>(img + plane_off(j, kg));
}
// token-product fragment of channel tile mc: k-slots 0..3 = tokens 4 kg .. 4 kg + 3, slot 4 = token 16 + kg (slots 5..7
// repeat it; the other operand holds zeros there)
__device__ __forceinline__ i32x4 colfrag(const char *img, int mc, int lane) {
  const int q = (lane >> 2) & 3, pp = lane & 3, kg = lane >> 4;
  const int ch = 2 * mc + (pp >> 1), half = (pp & 1) << 3;
  return tr_frag(img + plane_off(4 * kg + q, ch) + half, img + plane_off(16 + kg, ch) + half);
}

}  // namespace plane16
