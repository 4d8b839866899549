// Operand-range helpers of the scaled (two fp16 plane) mode, around the projections of proj_gemm.hip: what a tensor is
// scaled by (plane16.h: plane_scale) is derived from its largest finite magnitude or from an a-priori bound, both computed
// on the device by the small kernels here; planes_to_f32 is the way back from plane slots to plain fp32.
//   ampconv_proj_out_bound   bound of |A W^T + bias| from the largest |A|, before the product runs
//   ampconv_planes_to_f32    plane slots -> fp32
//   ampconv_absmax           largest finite magnitude of a tensor (fp32 or bf16)
//   ampconv_absmax_stats     ... with the range statistic that tells when one scale per tensor is too coarse
#include "proj_common.h"

using namespace proj;

// bound of the magnitudes of out = A W^T + bias from the largest magnitude of A: a_absmax * max_n sum_k |W[n][k]| +
// max_n |bias[n]| (W[n][k] at W[n * stride_n + k * stride_k]) -- what the plane output of proj_rows scales by, known
// BEFORE the product runs.  One workgroup: the weights are a few hundred KB.
namespace {
__global__ __launch_bounds__(1024) void out_bound_kernel(const float *__restrict__ W, int64_t sn, int64_t sk, int N, int K,
                                                         const float *__restrict__ bias, const float *__restrict__ amax,
                                                         float *__restrict__ out) {
  __shared__ float red[2][16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float l1 = 0.f, bm = 0.f;
  for (int n = w; n < N; n += 16) {
    float sum = 0.f;
    for (int k = lane; k < K; k += 64) sum += finite_abs(W[(int64_t)n * sn + (int64_t)k * sk]);
    l1 = fmaxf(l1, wave_sum(sum));
  }
  if (bias)
    for (int n = threadIdx.x; n < N; n += 1024) bm = fmaxf(bm, finite_abs(bias[n]));
  bm = wave_max(bm);
  if (lane == 0) { red[0][w] = l1; red[1][w] = bm; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 16; ++i) { l1 = fmaxf(l1, red[0][i]); bm = fmaxf(bm, red[1][i]); }
    out[0] = *amax * l1 + bm;
  }
}
}  // namespace

extern "C" int ampconv_proj_out_bound(const void *W, int64_t stride_n, int64_t stride_k, int N, int K, const void *bias,
                                      const float *a_absmax, float *out, void *stream) {
  if (!W || !a_absmax || !out || N <= 0 || K <= 0) return AMPCONV_E_BADARG;
  out_bound_kernel<<<1, 1024, 0, (hipStream_t)stream>>>((const float *)W, stride_n, stride_k, N, K, (const float *)bias,
                                                        a_absmax, out);
  return ampconv_launch_status();
}

// plane slots -> fp32, in place layout (the reverse of the PLANES epilogue; the lazily served side outputs and the
// fall-back paths read the projection buffer as fp32): X[M, K] with K a multiple of 32, rows ld floats apart
namespace {
__global__ __launch_bounds__(256) void planes_to_f32_kernel(const char *__restrict__ X, int64_t ld, int64_t M, int K8, int dh,
                                                            const float *__restrict__ bound, float *__restrict__ out,
                                                            int64_t ldo) {
  const float u = 1.f / plane_scale(*bound);
  const int pps = dh / 8;                                  // 8-channel pieces per slot
  const int64_t total = M * K8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / K8;
    const int r = (int)(i - row * K8), slot = r / pps, c = r - slot * pps;
    const char *src = X + (row * ld + (int64_t)slot * dh) * 4 + 16 * c;
    const uint4 h = *reinterpret_cast<const uint4 *>(src), l = *reinterpret_cast<const uint4 *>(src + 2 * dh);
    const unsigned hu[4] = {h.x, h.y, h.z, h.w}, lu[4] = {l.x, l.y, l.z, l.w};
    float v[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f16x2 hv = __builtin_bit_cast(f16x2, hu[k]), lv = __builtin_bit_cast(f16x2, lu[k]);
      v[2 * k] = ((float)hv[0] + (float)lv[0]) * u;
      v[2 * k + 1] = ((float)hv[1] + (float)lv[1]) * u;
    }
    float *o = out + row * ldo + slot * dh + 8 * c;
    *reinterpret_cast<float4 *>(o) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4 *>(o + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
}
}  // namespace

extern "C" int ampconv_planes_to_f32(const void *X, int64_t ld, int64_t M, int K, int plane_dh, const float *bound, void *out,
                                     int64_t ldo, void *stream) {
  if (M < 0 || K <= 0 || (plane_dh != 32 && plane_dh != 16) || K % plane_dh || ld < K || ldo < K || ld % 4 || ldo % 4 || !bound)
    return AMPCONV_E_BADARG;
  if (M == 0) return AMPCONV_OK;
  if (!X || !out || (uintptr_t)X % 16 || (uintptr_t)out % 16) return AMPCONV_E_BADARG;
  const int64_t pieces = M * (K / 8);
  int64_t grid = (pieces + 255) / 256;
  const int64_t cap = (int64_t)cu_count() * 16;
  if (grid > cap) grid = cap;
  planes_to_f32_kernel<<<(unsigned)grid, 256, 0, (hipStream_t)stream>>>((const char *)X, ld, M, K / 8, plane_dh, bound,
                                                                        (float *)out, ldo);
  return ampconv_launch_status();
}

// largest finite magnitude of X[M, K] (row stride ld), merged into *out by an atomic max: zero it first (reset != 0
// does) or let several calls accumulate.  NaN and infinities are skipped: they propagate through the products by
// themselves, in the rows they sit in.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void absmax_kernel(const T *__restrict__ X, int64_t ld, int64_t M, int K4,
                                                     float *__restrict__ out) {
  // K4 = 16-byte pieces per row; a workgroup walks pieces blockIdx.x * 256 + t, + gridDim.x * 256, ...
  constexpr int EPP = 16 / sizeof(T);
  const int64_t total = M * K4;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / K4;
    const int c = (int)(i - row * K4);
    const uint4 raw = *reinterpret_cast<const uint4 *>(X + row * ld + (int64_t)c * EPP);
    if constexpr (sizeof(T) == 4) {
      m = fmaxf(m, fmaxf(fmaxf(finite_abs(__builtin_bit_cast(float, raw.x)), finite_abs(__builtin_bit_cast(float, raw.y))),
                         fmaxf(finite_abs(__builtin_bit_cast(float, raw.z)), finite_abs(__builtin_bit_cast(float, raw.w)))));
    } else {
      const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        m = fmaxf(m, fmaxf(finite_abs(lo_as_f32(u[k])), finite_abs(hi_as_f32(u[k]))));
    }
  }
  __shared__ float red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    atomicMax(reinterpret_cast<unsigned *>(out), __builtin_bit_cast(unsigned, m));
  }
}
}  // namespace

extern "C" int ampconv_absmax(const void *X, int64_t ld, int64_t M, int K, int dtype, float *out, int reset,
                              void *stream) {
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  const int epp = dtype == AMPCONV_F32 ? 4 : 8;
  if (!out || M < 0 || K < 0 || K % epp || ld < K || ld % epp) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (reset) {
    const hipError_t e = hipMemsetAsync(out, 0, sizeof(float), st);
    if (e != hipSuccess) return (int)e;
  }
  if (M == 0 || K == 0) return AMPCONV_OK;
  if (!X || (uintptr_t)X % 16) return AMPCONV_E_BADARG;
  const int64_t pieces = M * (K / epp);
  int64_t grid = (pieces + 255) / 256;
  const int64_t cap = (int64_t)cu_count() * 16;         // eight loads per thread and more: the atomics stay few
  if (grid > cap) grid = cap;
  if (dtype == AMPCONV_F32)
    absmax_kernel<float><<<(unsigned)grid, 256, 0, st>>>((const float *)X, ld, M, K / epp, out);
  else
    absmax_kernel<unsigned short><<<(unsigned)grid, 256, 0, st>>>((const unsigned short *)X, ld, M, K / epp, out);
  return ampconv_launch_status();
}

// the same pass with a RANGE statistic beside the maximum (fp32): out[0] = largest finite magnitude, out[1] = the smallest
// non-zero maximum of any group of 8 consecutive 16-byte pieces (32 channels: one head slot of a row where K % 32 == 0).
// out[1] far below out[0] means whole rows / heads live binades under the tensor's maximum -- the data on which ONE scale
// per tensor costs the small rows their low plane (include/ampconv.h "SCALED MODE"); the caller then takes the exact
// kernels.  Single elements near zero do not count (absolute error is what a sum feels), all-zero groups neither.
namespace {
__global__ void absmax_stats_init_kernel(float *out) {
  out[0] = 0.f;
  out[1] = __builtin_inff();
}
template <int CTRL>
__device__ __forceinline__ float dpp_get(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
__global__ __launch_bounds__(256) void absmax_stats_kernel(const float *__restrict__ X, int64_t ld, int64_t M, int K4,
                                                           float *__restrict__ out) {
  const int64_t total = M * K4;
  float m = 0.f, smin = __builtin_inff();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / K4;
    const int c = (int)(i - row * K4);
    const float4 v = *reinterpret_cast<const float4 *>(X + row * ld + (int64_t)c * 4);
    const float m4 = finite_abs_max(0.f, v);
    m = fmaxf(m, m4);
    float g = fmaxf(m4, dpp_get<0xB1>(m4));     // quad_perm [1,0,3,2]
    g = fmaxf(g, dpp_get<0x4E>(g));             // quad_perm [2,3,0,1]
    g = fmaxf(g, dpp_get<0x141>(g));            // row_half_mirror: the 8 lanes of a half row (masked lanes read as 0)
    if (g > 0.f) smin = fminf(smin, g);
  }
  __shared__ float red[2][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    m = fmaxf(m, __shfl_xor(m, o));
    smin = fminf(smin, __shfl_xor(smin, o));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = m;
    red[1][threadIdx.x >> 6] = smin;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    smin = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
    atomicMax(reinterpret_cast<unsigned *>(out), __builtin_bit_cast(unsigned, m));          // non-negative floats order
    atomicMin(reinterpret_cast<unsigned *>(out + 1), __builtin_bit_cast(unsigned, smin));   // as their bits
  }
}
}  // namespace

extern "C" int ampconv_absmax_stats(const void *X, int64_t ld, int64_t M, int K, float *out, void *stream) {
  if (!out || M < 0 || K < 0 || K % 4 || ld < K || ld % 4) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  absmax_stats_init_kernel<<<1, 1, 0, st>>>(out);
  if (M == 0 || K == 0) return ampconv_launch_status();
  if (!X || (uintptr_t)X % 16) return AMPCONV_E_BADARG;
  const int64_t pieces = M * (K / 4);
  int64_t grid = (pieces + 255) / 256;
  const int64_t cap = (int64_t)cu_count() * 16;
  if (grid > cap) grid = cap;
  absmax_stats_kernel<<<(unsigned)grid, 256, 0, st>>>((const float *)X, ld, M, K / 4, out);
  return ampconv_launch_status();
}
