// The optimizer step behind the backward pass: a multi-tensor Adam / AdamW update and the global gradient norm that
// clips it, each as ONE launch over a whole parameter group (include/ampconv.h, "optimizer step").
// Reference: every training script runs torch.optim.Adam with L2 weight decay, most under CosineAnnealingWarmRestarts
//   experiments/cora_benchmark_graphsaint.py:84-85   Adam(model.parameters(), lr=0.1, weight_decay=1e-4)
//   src/ampnet/module/amp_gcn.py:278-405             gradient histograms: what a device-side gradient norm replaces
// REGIME.  AMPGCN's parameter set is ~0.23 M fp32 elements at the class defaults (142 k of them the embedding table) in
// 11-15 tensors: p, g, m and v together are a few MB, which the chip moves in about a microsecond.  The step is
// LAUNCH-bound, not bandwidth-bound: what counts is the number of launches and that nothing is copied or synchronised
// around them, not the bytes per lane.
// MAPPING.  The host cuts every tensor into chunks of kChunk = 1024 elements -- 256 lanes x one 16-byte piece per stream,
// so the class-default set is ~240 workgroups: one launch that covers the 256 CUs once.  Up to AMPCONV_ADAM_MAX_TENSORS
// descriptors and the prefix counts of their chunks travel BY VALUE as kernel arguments: no device table, no copy.  A
// workgroup finds its (tensor, chunk) by scanning those prefix counts; a chunk never straddles tensors.  Lane j of a
// chunk owns elements 4 j .. 4 j + 3 of it: one 16-byte piece per stream where all the tensor's pointers are 16-byte
// aligned and the piece lies inside the tensor, element by element otherwise (unaligned tensors, the tail).
// NORM.  The same mapping over g: a lane's squares in ascending order, an xor butterfly over the wave, the 4 waves in
// wave order through LDS into the workgroup's slot, then adam_norm_finish adds the slots in ascending order (256
// consecutive runs, then the run sums) and writes the square root: no floating-point atomics, the same bits on every
// launch, and the same bits whether a tensor is aligned or not.
#include "site_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = AMPCONV_ADAM_CHUNK;      // elements per workgroup: one 16-byte piece per lane and stream
constexpr int kMax = AMPCONV_ADAM_MAX_TENSORS;
static_assert(kChunk == kThreads * 4, "a chunk is one fp32 piece per lane");

struct Launch {                                 // the kernel-argument block of one launch
  ampconv_adam_tensor_t t[kMax];
  int32_t first[kMax];                          // first[i]: workgroups of the launch before tensor i (non-decreasing)
};

struct Hyper {
  float lr, beta2, omb1, omb2, eps, weight_decay, grad_scale, max_grad_norm;      // omb = 1 - beta, rounded from double
  int decoupled;
};

// the tensor that owns workgroup b: the last one whose first chunk is at or before b (empty tensors share the `first`
// of their successor and are stepped over)
__device__ __forceinline__ int tensor_of(const Launch &L, int b) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < kMax; ++k) i += L.first[k] <= b;
  return i;
}

__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const Hyper &h, float c, float step_size,
                                         float inv_bc2_sqrt) {
  g = g * h.grad_scale * c;
  if (h.decoupled) p *= 1.f - h.lr * h.weight_decay;
  else g += h.weight_decay * p;
  m = m + h.omb1 * (g - m);
  v = h.beta2 * v + h.omb2 * g * g;
  p = p - step_size * m / (sqrtf(v) * inv_bc2_sqrt + h.eps);
}

__global__ __launch_bounds__(kThreads) void adam_step_chunks(const Launch L, const Hyper h,
                                                             const float *__restrict__ norm) {
  const int ti = tensor_of(L, (int)blockIdx.x);
  const ampconv_adam_tensor_t d = L.t[ti];
  const int64_t i0 = (int64_t)((int)blockIdx.x - L.first[ti]) * kChunk + threadIdx.x * 4;
  if (i0 >= d.numel) return;
  const float c = norm ? fminf(1.f, h.max_grad_norm / (*norm + 1e-6f)) : 1.f;
  const bool vec = (((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.m | (uintptr_t)d.v) & 15) == 0;
  if (vec && i0 + 4 <= d.numel) {
    typedef Piece<float> P4;
    P4 p = *(const P4 *)(d.p + i0), m = *(const P4 *)(d.m + i0), v = *(const P4 *)(d.v + i0);
    const P4 g = *(const P4 *)(d.g + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) adam_one(p.e[e], g.e[e], m.e[e], v.e[e], h, c, d.step_size, d.inv_bc2_sqrt);
    *(P4 *)(d.p + i0) = p;
    *(P4 *)(d.m + i0) = m;
    *(P4 *)(d.v + i0) = v;
  } else {
    const int64_t i1 = i0 + 4 < d.numel ? i0 + 4 : d.numel;
    for (int64_t i = i0; i < i1; ++i) {
      float p = d.p[i], m = d.m[i], v = d.v[i];
      adam_one(p, d.g[i], m, v, h, c, d.step_size, d.inv_bc2_sqrt);
      d.p[i] = p;
      d.m[i] = m;
      d.v[i] = v;
    }
  }
}

// slots[blockIdx.x] = the chunk's sum of (g * grad_scale)^2
__global__ __launch_bounds__(kThreads) void adam_norm_chunks(const Launch L, float grad_scale, float *__restrict__ slots) {
  __shared__ float red[kThreads / 64];
  const int ti = tensor_of(L, (int)blockIdx.x);
  const float *g = L.t[ti].g;
  const int64_t numel = L.t[ti].numel;
  const int64_t i0 = (int64_t)((int)blockIdx.x - L.first[ti]) * kChunk + threadIdx.x * 4;
  float x[4] = {0.f, 0.f, 0.f, 0.f};
  if (((uintptr_t)g & 15) == 0 && i0 + 4 <= numel) {
    const Piece<float> q = *(const Piece<float> *)(g + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = q.e[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < numel) x[e] = g[i0 + e];
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = x[e] * grad_scale;
    s += y * y;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) t += red[w];
    slots[blockIdx.x] = t;
  }
}

// *norm = sqrt(sum of the n slots in ascending order): kThreads consecutive runs of slots, each an ascending chain, then
// the run sums in ascending order.  n == 0 writes 0.
__global__ __launch_bounds__(kThreads) void adam_norm_finish(const float *__restrict__ slots, int64_t n,
                                                             float *__restrict__ norm) {
  __shared__ float part[kThreads];
  const int64_t per = (n + kThreads - 1) / kThreads;
  const int64_t b0 = threadIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
  float s = 0.f;
  for (int64_t b = b0; b < b1; ++b) s += slots[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int r = 0; r < kThreads; ++r) t += part[r];
    *norm = sqrtf(t);
  }
}

inline int64_t chunks_of(int64_t numel) { return (numel + kChunk - 1) / kChunk; }

// the descriptors of a call: pointers and sizes; total = chunks of all n tensors
inline bool tensors_ok(const ampconv_adam_tensor_t *t, int n, int64_t *total) {
  if (n < 0 || (n > 0 && !t)) return false;
  int64_t sum = 0;
  for (int i = 0; i < n; ++i) {
    if (t[i].numel < 0 || t[i].numel > INT64_MAX - kChunk) return false;
    if (t[i].numel > 0 && !(t[i].p && t[i].g && t[i].m && t[i].v)) return false;
    sum += chunks_of(t[i].numel);
    if (sum > INT32_MAX) return false;                    // a launch's grid, and the slot index, are 32-bit
  }
  *total = sum;
  return true;
}

// f(launch block, its workgroups, workgroups of the launches before it) for each of the ceil(n / kMax) launches
template <typename F>
int for_each_launch(const ampconv_adam_tensor_t *t, int n, const F &f) {
  int64_t before = 0;
  for (int base = 0; base < n; base += kMax) {
    const int cnt = n - base < kMax ? n - base : kMax;
    Launch L = {};
    int32_t blocks = 0;
    for (int i = 0; i < kMax; ++i) {
      L.first[i] = blocks;
      if (i < cnt) {
        L.t[i] = t[base + i];
        blocks += (int32_t)chunks_of(t[base + i].numel);
      }
    }
    if (blocks == 0) continue;
    if (int rc = f(L, blocks, before)) return rc;
    before += blocks;
  }
  return AMPCONV_OK;
}

}  // namespace

extern "C" size_t ampconv_adam_workspace_bytes(const ampconv_adam_tensor_t *t, int n) {
  int64_t total = 0;
  if (!tensors_ok(t, n, &total)) return 0;
  return (size_t)total * sizeof(float);                   // a slot per chunk
}

extern "C" int ampconv_adam_grad_norm(const ampconv_adam_tensor_t *t, int n, float grad_scale, float *norm,
                                      void *workspace, size_t workspace_bytes, void *stream) {
  int64_t total = 0;
  if (!tensors_ok(t, n, &total) || !norm) return AMPCONV_E_BADARG;
  if (total > 0 && (!workspace || workspace_bytes < (size_t)total * sizeof(float))) return AMPCONV_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float *slots = (float *)workspace;
  if (int rc = for_each_launch(t, n, [&](const Launch &L, int32_t blocks, int64_t before) -> int {
        adam_norm_chunks<<<blocks, kThreads, 0, s>>>(L, grad_scale, slots + before);
        return ampconv_launch_status();
      }))
    return rc;
  adam_norm_finish<<<1, kThreads, 0, s>>>(slots, total, norm);
  return ampconv_launch_status();
}

extern "C" int ampconv_adam_step(const ampconv_adam_tensor_t *t, int n, float lr, double beta1, double beta2, float eps,
                                 float weight_decay, int decoupled, float grad_scale, const float *norm,
                                 float max_grad_norm, void *stream) {
  int64_t total = 0;
  if (!tensors_ok(t, n, &total) || !(lr >= 0.f) || !(eps > 0.f) || !(beta1 >= 0. && beta1 < 1.) ||
      !(beta2 >= 0. && beta2 < 1.) || !(weight_decay >= 0.f) || (norm && !(max_grad_norm > 0.f)))
    return AMPCONV_E_BADARG;
  // 1 - beta in double, then rounded: 1.f - 0.999f is 0.00099998713, 1.3e-5 off the 0.001 that scales every g * g
  const Hyper h = {lr, (float)beta2, (float)(1. - beta1), (float)(1. - beta2), eps, weight_decay, grad_scale, max_grad_norm,
                   decoupled != 0};
  return for_each_launch(t, n, [&](const Launch &L, int32_t blocks, int64_t) -> int {
    adam_step_chunks<<<blocks, kThreads, 0, (hipStream_t)stream>>>(L, h, norm);
    return ampconv_launch_status();
  });
}

// ---- mixed precision: bf16 parameters behind an fp32 master copy, gradients of either dtype ---------------------------
// The same grid, the same chunk and the same four elements per lane as above.  A piece is four elements of its own stream:
// 16 bytes on fp32 streams, 8 bytes on bf16 ones.  The dtype pair is uniform per workgroup (it belongs to the tensor).
// ROUNDING.  adam_one leaves the contraction of its multiply-adds to the compiler, and the object code of adam_step_chunks
// settled on the sequence that adam_one_pinned writes out -- with ONE difference between its two paths: the 16-byte
// pieces form the denominator as fma(sqrt(v), inv_bc2_sqrt, eps), the element-wise path as sqrt(v) * inv_bc2_sqrt + eps
// (two roundings; they differ where eps is not negligible beside sqrt(v)).  A second compilation of adam_one contracts
// differently again, so the mixed kernel pins every rounding, and it picks the denominator BY POSITION: an element
// whose group 4 j .. 4 j + 3 lies inside the tensor gets the piece's, the up to three elements behind the last whole
// group the element-wise one -- whatever the alignment.  So: a bf16 gradient gives the bits of its widened copy; alignment
// changes no bit; all-fp32 descriptors give the bits of adam_step_chunks on every tensor that kernel walks in pieces
// (all pointers 16-byte aligned: every tensor torch allocates).  On an fp32 tensor that is NOT 16-byte aligned
// adam_step_chunks takes the element-wise denominator for every element and the mixed kernel does not follow it: the two
// properties exclude each other there.
namespace {

template <typename T>
struct alignas(4 * sizeof(T)) Quad {
  T e[4];
};

struct MixedLaunch {                            // 24 x 64 + 24 x 4 bytes of kernel arguments
  ampconv_adam_mixed_tensor_t t[kMax];
  int32_t first[kMax];
};
static_assert(sizeof(ampconv_adam_mixed_tensor_t) == 64, "the descriptor of include/ampconv.h");

__device__ __forceinline__ int mixed_tensor_of(const MixedLaunch &L, int b) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < kMax; ++k) i += L.first[k] <= b;
  return i;
}

template <typename T>
__device__ __forceinline__ bool piece_aligned(const T *p) {
  return ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0;
}

// adam_one with every rounding written out (see ROUNDING above); decay = fma(-lr, weight_decay, 1).  WHOLE: the element's
// group of four lies inside the tensor.
template <bool WHOLE>
__device__ __forceinline__ void adam_one_pinned(float &p, float g, float &m, float &v, const Hyper &h, float c, float decay,
                                                float step_size, float inv_bc2_sqrt) {
#pragma clang fp contract(off)
  const float gs = g * h.grad_scale;
  const float l2 = h.decoupled ? -0.f : h.weight_decay * p;
  if (h.decoupled) p = p * decay;
  g = __builtin_fmaf(c, gs, l2);
  const float og = h.omb2 * g;
  v = __builtin_fmaf(g, og, h.beta2 * v);
  m = __builtin_fmaf(h.omb1, g - m, m);
  const float r = sqrtf(v);
  const float den = WHOLE ? __builtin_fmaf(r, inv_bc2_sqrt, h.eps) : r * inv_bc2_sqrt + h.eps;
  p = p - (step_size * m) / den;
}

// w: the fp32 value of the parameter (master for a bf16 p, p itself for an fp32 one); p16: the bf16 parameter or NULL
template <typename TG>
__device__ __forceinline__ void mixed_step_chunk(const ampconv_adam_mixed_tensor_t &d, float *__restrict__ w,
                                                 __bf16 *__restrict__ p16, int64_t i0, const Hyper &h, float c) {
  const TG *__restrict__ g = (const TG *)d.g;
  const bool vec = piece_aligned(w) && piece_aligned(g) && piece_aligned(d.m) && piece_aligned(d.v) &&
                   (!p16 || piece_aligned(p16));
  const bool whole = i0 + 4 <= d.numel;
  const float decay = __builtin_fmaf(-h.lr, h.weight_decay, 1.f);
  if (vec && whole) {
    typedef Quad<float> F4;
    F4 p = *(const F4 *)(w + i0), m = *(const F4 *)(d.m + i0), v = *(const F4 *)(d.v + i0);
    const Quad<TG> q = *(const Quad<TG> *)(g + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      adam_one_pinned<true>(p.e[e], (float)q.e[e], m.e[e], v.e[e], h, c, decay, d.step_size, d.inv_bc2_sqrt);
    *(F4 *)(w + i0) = p;
    *(F4 *)(d.m + i0) = m;
    *(F4 *)(d.v + i0) = v;
    if (p16) {
      Quad<__bf16> r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r.e[e] = (__bf16)p.e[e];          // round to nearest even
      *(Quad<__bf16> *)(p16 + i0) = r;
    }
  } else {
    const int64_t i1 = i0 + 4 < d.numel ? i0 + 4 : d.numel;
    for (int64_t i = i0; i < i1; ++i) {
      float p = w[i], m = d.m[i], v = d.v[i];
      if (whole) adam_one_pinned<true>(p, (float)g[i], m, v, h, c, decay, d.step_size, d.inv_bc2_sqrt);
      else adam_one_pinned<false>(p, (float)g[i], m, v, h, c, decay, d.step_size, d.inv_bc2_sqrt);
      w[i] = p;
      d.m[i] = m;
      d.v[i] = v;
      if (p16) p16[i] = (__bf16)p;
    }
  }
}

__global__ __launch_bounds__(kThreads) void adam_mixed_step_chunks(const MixedLaunch L, const Hyper h,
                                                                   const float *__restrict__ norm) {
  const int ti = mixed_tensor_of(L, (int)blockIdx.x);
  const ampconv_adam_mixed_tensor_t d = L.t[ti];
  const int64_t i0 = (int64_t)((int)blockIdx.x - L.first[ti]) * kChunk + threadIdx.x * 4;
  if (i0 >= d.numel) return;
  const float c = norm ? fminf(1.f, h.max_grad_norm / (*norm + 1e-6f)) : 1.f;
  const bool p_bf16 = d.p_dtype == AMPCONV_BF16;
  float *w = p_bf16 ? d.master : (float *)d.p;
  __bf16 *p16 = p_bf16 ? (__bf16 *)d.p : nullptr;
  if (d.g_dtype == AMPCONV_BF16) mixed_step_chunk<__bf16>(d, w, p16, i0, h, c);
  else mixed_step_chunk<float>(d, w, p16, i0, h, c);
}

template <typename TG>
__device__ __forceinline__ void load_grad4(const TG *__restrict__ g, int64_t i0, int64_t numel, float (&x)[4]) {
  if (piece_aligned(g) && i0 + 4 <= numel) {
    const Quad<TG> q = *(const Quad<TG> *)(g + i0);
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = (float)q.e[e];
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (i0 + e < numel) x[e] = (float)g[i0 + e];
  }
}

// slots[blockIdx.x] = the chunk's sum of (g * grad_scale)^2: the reduction of adam_norm_chunks on the widened gradient
__global__ __launch_bounds__(kThreads) void adam_mixed_norm_chunks(const MixedLaunch L, float grad_scale,
                                                                   float *__restrict__ slots) {
  __shared__ float red[kThreads / 64];
  const int ti = mixed_tensor_of(L, (int)blockIdx.x);
  const int64_t numel = L.t[ti].numel;
  const int64_t i0 = (int64_t)((int)blockIdx.x - L.first[ti]) * kChunk + threadIdx.x * 4;
  float x[4] = {0.f, 0.f, 0.f, 0.f};
  if (L.t[ti].g_dtype == AMPCONV_BF16) load_grad4((const __bf16 *)L.t[ti].g, i0, numel, x);
  else load_grad4((const float *)L.t[ti].g, i0, numel, x);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float y = x[e] * grad_scale;
    s += y * y;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = red[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) t += red[w];
    slots[blockIdx.x] = t;
  }
}

inline bool dtype_ok(int32_t d) { return d == AMPCONV_F32 || d == AMPCONV_BF16; }

inline bool mixed_tensors_ok(const ampconv_adam_mixed_tensor_t *t, int n, int64_t *total) {
  if (n < 0 || (n > 0 && !t)) return false;
  int64_t sum = 0;
  for (int i = 0; i < n; ++i) {
    if (!dtype_ok(t[i].p_dtype) || !dtype_ok(t[i].g_dtype)) return false;
    if (t[i].p_dtype == AMPCONV_F32 && t[i].master) return false;      // an fp32 parameter is its own master
    if (t[i].numel < 0 || t[i].numel > INT64_MAX - kChunk) return false;
    if (t[i].numel > 0 && !(t[i].p && t[i].g && t[i].m && t[i].v)) return false;
    if (t[i].numel > 0 && t[i].p_dtype == AMPCONV_BF16 && !t[i].master) return false;
    sum += chunks_of(t[i].numel);
    if (sum > INT32_MAX) return false;
  }
  *total = sum;
  return true;
}

template <typename F>
int for_each_mixed_launch(const ampconv_adam_mixed_tensor_t *t, int n, const F &f) {
  int64_t before = 0;
  for (int base = 0; base < n; base += kMax) {
    const int cnt = n - base < kMax ? n - base : kMax;
    MixedLaunch L = {};
    int32_t blocks = 0;
    for (int i = 0; i < kMax; ++i) {
      L.first[i] = blocks;
      if (i < cnt) {
        L.t[i] = t[base + i];
        blocks += (int32_t)chunks_of(t[base + i].numel);
      }
    }
    if (blocks == 0) continue;
    if (int rc = f(L, blocks, before)) return rc;
    before += blocks;
  }
  return AMPCONV_OK;
}

}  // namespace

extern "C" size_t ampconv_adam_mixed_workspace_bytes(const ampconv_adam_mixed_tensor_t *t, int n) {
  int64_t total = 0;
  if (!mixed_tensors_ok(t, n, &total)) return 0;
  return (size_t)total * sizeof(float);
}

extern "C" int ampconv_adam_mixed_grad_norm(const ampconv_adam_mixed_tensor_t *t, int n, float grad_scale, float *norm,
                                            void *workspace, size_t workspace_bytes, void *stream) {
  int64_t total = 0;
  if (!mixed_tensors_ok(t, n, &total) || !norm) return AMPCONV_E_BADARG;
  if (total > 0 && (!workspace || workspace_bytes < (size_t)total * sizeof(float))) return AMPCONV_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  float *slots = (float *)workspace;
  if (int rc = for_each_mixed_launch(t, n, [&](const MixedLaunch &L, int32_t blocks, int64_t before) -> int {
        adam_mixed_norm_chunks<<<blocks, kThreads, 0, s>>>(L, grad_scale, slots + before);
        return ampconv_launch_status();
      }))
    return rc;
  adam_norm_finish<<<1, kThreads, 0, s>>>(slots, total, norm);
  return ampconv_launch_status();
}

extern "C" int ampconv_adam_mixed_step(const ampconv_adam_mixed_tensor_t *t, int n, float lr, double beta1, double beta2,
                                       float eps, float weight_decay, int decoupled, float grad_scale, const float *norm,
                                       float max_grad_norm, void *stream) {
  int64_t total = 0;
  if (!mixed_tensors_ok(t, n, &total) || !(lr >= 0.f) || !(eps > 0.f) || !(beta1 >= 0. && beta1 < 1.) ||
      !(beta2 >= 0. && beta2 < 1.) || !(weight_decay >= 0.f) || (norm && !(max_grad_norm > 0.f)))
    return AMPCONV_E_BADARG;
  const Hyper h = {lr, (float)beta2, (float)(1. - beta1), (float)(1. - beta2), eps, weight_decay, grad_scale, max_grad_norm,
                   decoupled != 0};
  return for_each_mixed_launch(t, n, [&](const MixedLaunch &L, int32_t blocks, int64_t) -> int {
    adam_mixed_step_chunks<<<blocks, kThreads, 0, (hipStream_t)stream>>>(L, h, norm);
    return ampconv_launch_status();
  });
}
