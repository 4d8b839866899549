// Rows of a node matrix read through index arrays, for the kernels that keep 16 rows of a FIXED side in registers and
// walk a STREAMED side in 32-row LDS tiles (pair_loss.hip, knn.hip): the id clamp, the row loaders and the split of the
// streamed side over blockIdx.y.  The loaders take any argument block `A` with the fields
//   const void *Z; int64_t ldz; int D, bf16, vec;
// (vec: D % 4 == 0, ldz % 4 == 0 and a base aligned to four elements).
#pragma once
#include <algorithm>
#include <type_traits>
#include "mfma_tile.h"

constexpr int kTS = 32;            // streamed rows per LDS tile

__device__ __forceinline__ int64_t clamp_id(int64_t v, int64_t N) { return v < 0 ? 0 : (v >= N ? N - 1 : v); }
__device__ __forceinline__ float bf16_f32(unsigned h) { return __uint_as_float(h << 16); }

template <typename A>
__device__ __forceinline__ float load1(const A &a, int64_t row, int c) {
  if (c >= a.D) return 0.f;
  if (a.bf16) return bf16_f32(reinterpret_cast<const uint16_t *>(a.Z)[row * a.ldz + c]);
  return reinterpret_cast<const float *>(a.Z)[row * a.ldz + c];
}
// channels c .. c + 3 of a row (c % 4 == 0), zero from D on
template <typename A>
__device__ __forceinline__ float4 load4(const A &a, int64_t row, int c) {
  if (a.vec) {                     // D % 4 == 0, ldz % 4 == 0 and an aligned base: the four channels are one load
    const int cc = c < a.D ? c : 0;                   // a padding chunk loads chunk 0 and drops it: no branch around a load
    float4 v;
    if (a.bf16) {
      const uint2 u = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(a.Z) + row * a.ldz + cc);
      v = make_float4(bf16_f32(u.x & 0xFFFFu), bf16_f32(u.x >> 16), bf16_f32(u.y & 0xFFFFu), bf16_f32(u.y >> 16));
    } else {
      v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(a.Z) + row * a.ldz + cc);
    }
    return c < a.D ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (c >= a.D) return make_float4(0.f, 0.f, 0.f, 0.f);
  return make_float4(load1(a, row, c), load1(a, row, c + 1), load1(a, row, c + 2), load1(a, row, c + 3));
}

// The same four channels as they come from memory, and their conversion apart from it: a streamed tile is asked for one
// tile ahead and must not be looked at -- not even by a select -- before it goes to LDS, or the wave waits for it at once.
// PATH 0: fp32, one 16-byte load; 1: bf16, one 8-byte load; 2: fp32, 3: bf16, element by element.  Channels from D on are
// read from channel 0 instead (a valid address, no branch) and zeroed by cook4.
template <int PATH, typename A>
__device__ __forceinline__ uint4 raw4(const A &a, int64_t row, int c) {
  if (PATH == 0) return *reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(a.Z) + row * a.ldz + (c < a.D ? c : 0));
  if (PATH == 1) {
    const uint2 u = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(a.Z) + row * a.ldz + (c < a.D ? c : 0));
    return make_uint4(u.x, u.y, 0u, 0u);
  }
  unsigned v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t at = row * a.ldz + (c + e < a.D ? c + e : 0);
    v[e] = PATH == 2 ? reinterpret_cast<const unsigned *>(a.Z)[at] : (unsigned)reinterpret_cast<const uint16_t *>(a.Z)[at];
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}
template <int PATH, typename A>
__device__ __forceinline__ float4 cook4(const A &a, uint4 u, int c, bool row_ok) {
  float4 v;
  if (PATH == 0 || PATH == 2) v = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
  else if (PATH == 1) v = make_float4(bf16_f32(u.x & 0xFFFFu), bf16_f32(u.x >> 16), bf16_f32(u.y & 0xFFFFu), bf16_f32(u.y >> 16));
  else v = make_float4(bf16_f32(u.x), bf16_f32(u.y), bf16_f32(u.z), bf16_f32(u.w));
  v.x = row_ok && c < a.D ? v.x : 0.f;
  v.y = row_ok && c + 1 < a.D ? v.y : 0.f;
  v.z = row_ok && c + 2 < a.D ? v.z : 0.f;
  v.w = row_ok && c + 3 < a.D ? v.w : 0.f;
  return v;
}
template <typename A, typename F>
__device__ __forceinline__ void by_path(const A &a, F &&f) {     // workgroup-uniform
  if (a.vec) {
    if (!a.bf16) f(std::integral_constant<int, 0>()); else f(std::integral_constant<int, 1>());
  } else {
    if (!a.bf16) f(std::integral_constant<int, 2>()); else f(std::integral_constant<int, 3>());
  }
}

// ---- host side
constexpr size_t kPartialCap = (size_t)4 << 20;

struct Split { int tiles, per, n; };
// splits of the streamed side: enough waves to fill the card, at most 64, and (row_bytes > 0: partials of that many bytes
// per fixed row and split) from the third split on only while the partials stay under 4 MiB
static inline Split stream_split(int64_t nfixed, int64_t nstream, size_t row_bytes) {
  Split s;
  s.tiles = (int)((nstream + kTS - 1) / kTS);
  const int64_t waves = (nfixed + 15) / 16;
  int64_t n = waves > 0 ? (2048 + waves - 1) / waves : 1;
  n = std::min<int64_t>(std::min<int64_t>(n, s.tiles), 64);
  n = std::max<int64_t>(n, 1);
  while (n > 2 && (size_t)n * (size_t)nfixed * row_bytes > kPartialCap) --n;
  s.per = (int)((s.tiles + n - 1) / n);
  if (s.per < 1) s.per = 1;
  s.n = std::max(1, (s.tiles + s.per - 1) / s.per);
  return s;
}
