// Shared pieces of the node-phase projection kernels (proj_gemm.hip: fp32 storage, proj_gemm_bf16.hip: bf16 storage).
// The plane format itself (conversions, scale, split, transposed-read fragments and their fences): plane16.h.
#pragma once
#include "plane16.h"

namespace proj {
using namespace plane16;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) char lds_char;

constexpr int kFrag = 1024;          // one MFMA operand fragment: 64 lanes x 8 bf16
constexpr int kXcd = 8;

__device__ __forceinline__ float lo_as_f32(unsigned h) { return __builtin_bit_cast(float, h << 16); }
__device__ __forceinline__ float hi_as_f32(unsigned h) { return __builtin_bit_cast(float, h & 0xFFFF0000u); }

#define MFMA32H(a, b, c)                                                                                         \
  __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(proj::f16x8, a), __builtin_bit_cast(proj::f16x8, b), \
                                         (c), 0, 0, 0)

#define MFMA32(a, b, c)                                                                                          \
  __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(proj::bf16x8, a), __builtin_bit_cast(proj::bf16x8, b), \
                                          (c), 0, 0, 0)

// LDS-DMA of 16 bytes per lane: LDS destination = wave-uniform `lds_dst` + 16 * lane, source per lane.
// Inline assembly on purpose: behind the builtin hipcc orders every later LDS read after the DMA with
// `s_waitcnt vmcnt(0)` (the whole memory latency); the kernels wait for their DMAs themselves.
__device__ __forceinline__ void dma16(const void *gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
               "s_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}

inline int cu_count() {
  static const int n_cu = [] {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n;
  }();
  return n_cu;
}

// ---- the second step of both weight-gradient products: out[e] = sum over the slices of part[s][e]; e < n_dw goes to dW,
// the rest to colsum.  256 threads = 32 float4 elements x 8 slice phases: phase g adds slices g, g + 8, ... in order (four
// loads in flight), the eight phase sums meet in LDS and are added in a fixed order -- bitwise reproducible, and S / 8
// dependent load rounds instead of S.  `Out` is the epilogue: where four sums of dW / of the column sums go, and as what.
struct ReduceF32 {      // fp32 out; scaled mode (amax_a / amax_b non-null): the dW part leaves through the two exact inverse scales
  float *dW, *colsum;
  const float *amax_a, *amax_b;
  __device__ __forceinline__ void dw(float4 acc, size_t o) const {
    if (amax_a) {
      const float ua = plane_unscale(*amax_a), ub = plane_unscale(*amax_b);
      acc.x = acc.x * ua * ub; acc.y = acc.y * ua * ub; acc.z = acc.z * ua * ub; acc.w = acc.w * ua * ub;
    }
    *reinterpret_cast<float4 *>(dW + o) = acc;
  }
  __device__ __forceinline__ void cs(float4 acc, size_t o) const { *reinterpret_cast<float4 *>(colsum + o) = acc; }
};
struct ReduceBf16 {     // one rounding to bf16 on the way out
  unsigned short *dW, *colsum;
  static __device__ __forceinline__ i32x2 pack(float4 acc) { return i32x2{cvt_pk_bf16(acc.x, acc.y), cvt_pk_bf16(acc.z, acc.w)}; }
  __device__ __forceinline__ void dw(float4 acc, size_t o) const { *reinterpret_cast<i32x2 *>(dW + o) = pack(acc); }
  __device__ __forceinline__ void cs(float4 acc, size_t o) const { *reinterpret_cast<i32x2 *>(colsum + o) = pack(acc); }
};
template <class Out>
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ part, int S, int Na, int Nb, int Nap,
                                                           int Nbp, Out out) {
  __shared__ float4 red[8][32];
  const int el = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int64_t n_dw = (int64_t)Nap * Nbp, n_all = n_dw + Nap;        // the slabs cover the padded shape
  const int64_t e = ((int64_t)blockIdx.x * 32 + el) * 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e < n_all) {
    float4 a1 = acc;
    int s = g;
    for (; s + 8 < S; s += 16) {
      const float4 v0 = *reinterpret_cast<const float4 *>(part + (size_t)s * n_all + e);
      const float4 v1 = *reinterpret_cast<const float4 *>(part + (size_t)(s + 8) * n_all + e);
      acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
      a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
    }
    if (s < S) {
      const float4 v0 = *reinterpret_cast<const float4 *>(part + (size_t)s * n_all + e);
      acc.x += v0.x; acc.y += v0.y; acc.z += v0.z; acc.w += v0.w;
    }
    acc.x += a1.x; acc.y += a1.y; acc.z += a1.z; acc.w += a1.w;
  }
  red[g][el] = acc;
  __syncthreads();
  if (g == 0 && e < n_all) {
#pragma unroll
    for (int k = 1; k < 8; ++k) {
      const float4 v = red[k][el];
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    if (e < n_dw) {
      const int i = (int)(e / Nbp), j = (int)(e - (int64_t)i * Nbp);
      if (i < Na && j < Nb) out.dw(acc, (size_t)i * Nb + j);
    } else if (out.colsum && e - n_dw < Na) {
      out.cs(acc, (size_t)(e - n_dw));
    }
  }
}

// ---- the first step's shape: tile of dW and row slices, for `rows_per_stage` rows per pipeline stage (kRS / kRSB)
struct WgradPlan {
  int S;
  int64_t rows_per_slice;      // a multiple of rows_per_stage
  int ti, tj;
};
// padded shape (multiples of 128).  256 x 256: eight waves, one workgroup per CU; the others: four waves, two per CU.
// `square`: the kernel has T x T tiles only (bf16 storage), else 128 x 256 exists too (Na an odd multiple of 128)
inline WgradPlan wgrad_plan(int64_t M, int Nap, int Nbp, int rows_per_stage, bool square) {
  WgradPlan p;
  p.tj = Nbp % 256 == 0 ? 256 : 128;
  p.ti = (Nap % 256 == 0 && p.tj == 256) ? 256 : 128;
  if (square) p.tj = p.ti;
  const int64_t ntiles = (int64_t)(Nap / p.ti) * (Nbp / p.tj);
  const int64_t nstages = (M + rows_per_stage - 1) / rows_per_stage;
  // one round of workgroups: slices are dealt to the 8 XCDs in turn (round-robin dispatch) and every slice brings
  // `ntiles` workgroups, so an XCD's 32 CUs (x 2 for the 4-wave shapes) hold floor(32 / ntiles) slices each --
  // one slice more on some XCDs would run as a second round and double the time
  const int per_xcd = (p.ti == 256 ? 1 : 2) * 32;
  int64_t S = (int64_t)kXcd * (per_xcd / ntiles > 0 ? per_xcd / ntiles : 1);
  if (S > nstages) S = nstages > 0 ? nstages : 1;
  p.rows_per_slice = ((nstages + S - 1) / S) * rows_per_stage;
  p.S = (int)((M + p.rows_per_slice - 1) / p.rows_per_slice);
  if (p.S < 1) p.S = 1;
  return p;
}

}  // namespace proj

// ---- bf16-storage entry points (proj_gemm_bf16.hip), dispatched by the C ABI in proj_gemm.hip
size_t ampconv_proj_weight_image_bytes_bf16(int N, int K);
bool ampconv_proj_supported_bf16(int N, int K);
int ampconv_proj_weight_images_bf16(int count, const ampconv_weight_image_t *jobs, hipStream_t stream);
int ampconv_proj_rows_bf16(const void *A, int64_t lda, int64_t M, int K, const void *wimage, int N, const void *bias,
                           const int32_t *rowptr, int L, void *out, int64_t ldc, const int32_t *nodes, int64_t n_nodes,
                           hipStream_t stream);
size_t ampconv_proj_wgrad_workspace_bytes_bf16(int64_t M, int Na, int Nb);
int ampconv_proj_wgrad_bf16(const void *A, int64_t lda, const void *B, int64_t ldb, int64_t M, int Na, int Nb,
                            const int32_t *rowptr, int L, void *dW, void *colsum, void *workspace,
                            size_t workspace_bytes, const int32_t *nodes, int64_t n_nodes, hipStream_t stream);
