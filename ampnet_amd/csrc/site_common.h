// What the element-wise sites around the layers share (glue.hip, norm.hip): the 16-byte piece, the activations, THE MASK
// of include/ampconv.h and the (dtype, activation) dispatch.
#pragma once
#include <type_traits>

#include "common.h"

namespace {

template <typename T>
struct alignas(16) Piece {
  static constexpr int N = 16 / sizeof(T);
  T e[N];
};

template <int ACT>
__device__ __forceinline__ float act_value(float x) {
  if constexpr (ACT == AMPCONV_ACT_RELU) return x > 0.f ? x : 0.f;
  if constexpr (ACT == AMPCONV_ACT_ELU) return x > 0.f ? x : expm1f(x);
  return x;
}
// act'(x) from a = act(x): what the element-wise backward has (it is handed the saved OUTPUT)
template <int ACT>
__device__ __forceinline__ float act_slope_of_value(float a) {
  if constexpr (ACT == AMPCONV_ACT_RELU) return a > 0.f ? 1.f : 0.f;
  if constexpr (ACT == AMPCONV_ACT_ELU) return a > 0.f ? 1.f : a + 1.f;
  return 1.f;
}
// act'(x) from x: what the pooling backward has (the layer output is alive anyway)
template <int ACT>
__device__ __forceinline__ float act_slope_of_input(float x) {
  if constexpr (ACT == AMPCONV_ACT_RELU) return x > 0.f ? 1.f : 0.f;
  if constexpr (ACT == AMPCONV_ACT_ELU) return x > 0.f ? 1.f : expf(x);
  return 1.f;
}

// THE MASK (include/ampconv.h): bit k of the result = element 4 g0 + k is kept, for the NP / 4 groups of one piece.
// thr == 0 keeps everything and costs no hash (wave-uniform branch).
template <int NP>
__device__ __forceinline__ uint32_t keep_bits(uint64_t seed, uint32_t thr, uint64_t g0) {
  if (thr == 0) return 0xFFFFFFFFu;
  uint32_t bits = 0;
#pragma unroll
  for (int j = 0; j < NP / 4; ++j) {
    const uint64_t h = splitmix64(seed ^ splitmix64(g0 + j));
#pragma unroll
    for (int k = 0; k < 4; ++k) bits |= (uint32_t)(((uint32_t)(h >> (16 * k)) & 0xFFFFu) >= thr) << (4 * j + k);
  }
  return bits;
}
__device__ __forceinline__ bool keep_one(uint64_t seed, uint32_t thr, uint64_t i) {
  if (thr == 0) return true;
  const uint64_t h = splitmix64(seed ^ splitmix64(i >> 2));
  return ((uint32_t)(h >> (16 * (i & 3))) & 0xFFFFu) >= thr;
}

// f(T{}, integral_constant<int, ACT>{}) for the (dtype, activation) of a call
template <typename F>
int with_type_and_act(int dtype, int act, const F &f) {
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  if (act < AMPCONV_ACT_IDENTITY || act > AMPCONV_ACT_ELU) return AMPCONV_E_BADARG;
  auto by_act = [&](auto t) {
    if (act == AMPCONV_ACT_RELU) return f(t, std::integral_constant<int, AMPCONV_ACT_RELU>{});
    if (act == AMPCONV_ACT_ELU) return f(t, std::integral_constant<int, AMPCONV_ACT_ELU>{});
    return f(t, std::integral_constant<int, AMPCONV_ACT_IDENTITY>{});
  };
  return dtype == AMPCONV_BF16 ? by_act(__bf16{}) : by_act(float{});
}

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline bool mask_args_ok(uint32_t thr, float scale) { return thr <= 65535u && scale > 0.f; }

}  // namespace
