// Tensor statistics where the tensors lie: counts, extrema and fp64 moments in one pass, a histogram and exact order
// statistics in a few more (include/ampconv.h, "tensor statistics").
// Reference: src/ampnet/module/amp_gcn.py:278-405 copies every weight gradient and five [N, L*D] activations to the host
// for seaborn histograms and mean / median / std / abs().mean() / abs().max() titles; a plot needs a few dozen numbers.
// MAPPING.  Descriptors and the prefix counts of their workgroups travel BY VALUE as kernel arguments (optim.hip's
// scheme).  A tensor is cut into chunks of kChunk = 4096 elements and gets min(chunks, kMaxBlocks) workgroups; workgroup
// w walks chunks w, w + workgroups, ...: every pass is a pure read stream, 64 bytes (fp32) or 32 (bf16) per lane in
// flight.  Lane j owns the 16-byte pieces j, j + 256, ... of a chunk whether they are read as pieces (16-byte aligned base,
// whole chunk inside the tensor) or element by element: alignment changes no result bit.
// BITS.  The library is built with -fno-honor-nans: every element arrives as its bit pattern (bf16 shifted into the upper
// half of an fp32 pattern), is classified from it, and a non-finite one is replaced by the pattern of +0 with its `finite`
// flag off before anything converts it to a floating-point value.  min / max / the selection compare the unsigned key of
// the bits, absmax the bits without the sign.
// MOMENTS.  No floating-point atomics: lane sums in ascending element order, an xor butterfly over the wave, the four waves
// in wave order into the workgroup's slot, then stats_moments_finish adds a tensor's slots in ascending order (256
// consecutive runs, then the run sums).  The grid depends on the numels only, so the bits repeat from call to call.
// COUNTS.  stats_count is ONE kernel body for the value histogram and for a digit pass of the radix select; the binning
// policy says which table entry an element goes to.  A workgroup counts in LDS with 32-bit atomics and flushes the non-zero
// entries into the 64-bit global counts with integer atomics at its end and every kFlushEvery chunks (2^31 elements, before
// an entry can wrap).  A ReLU output sends most elements to one entry: lds_add first counts the lanes of the wave that
// share the first active lane's entry and lets that lane add them at once (-DAMPCONV_STATS_NO_AGG: one atomic per lane).
#include "site_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = AMPCONV_STATS_CHUNK;
constexpr int kPerLane = kChunk / kThreads;          // 16 elements of a chunk per lane
constexpr int kMax = AMPCONV_STATS_MAX_TENSORS;
constexpr int kMaxBlocks = 1024;                     // workgroups per tensor: 4 per CU, 16 MB (fp32) in flight chip-wide
constexpr int kMaxBins = AMPCONV_STATS_MAX_BINS;
constexpr int kRanks = AMPCONV_STATS_MAX_RANKS;
constexpr int kDigits = 2048;                        // entries of a digit table (11 bits)
constexpr int kFlushEvery = (1 << 19);               // chunks between two flushes of a workgroup: 2^31 elements
constexpr int64_t kMaxNumel = (int64_t)1 << 44;
static_assert(kPerLane == 16 && kChunk == kThreads * kPerLane, "a lane holds 16 elements of a chunk");

struct Launch {                                      // the kernel-argument block of one launch
  ampconv_stats_tensor_t t[kMax];
  int32_t first[kMax + 1];                           // first[i]: workgroups before tensor i; first[kMax]: all of them
  int32_t count;                                     // descriptors in use
};

struct Partial {                                     // a workgroup's slot of the moments pass
  double sum, sum_abs, sum_sq;
  uint64_t finite, nan, inf, zero, negative;
  uint32_t kmin, kmax, amax, pad;                    // keys of min and max, bits of absmax
};

struct SelState {                                    // per (tensor, rank) between the digit passes
  uint64_t k;                                        // rank among the elements under `prefix`
  uint32_t prefix, pad;                              // the key's digits chosen so far
};

__device__ __forceinline__ int tensor_of(const Launch &L, int b) {
  int i = 0;
#pragma unroll
  for (int k = 1; k < kMax; ++k) i += L.first[k] <= b;
  return i;
}

// ---- bit patterns
__device__ __forceinline__ bool finite_bits(uint32_t u) { return (u & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ uint32_t key_of(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
// the pattern whose key starts with `k`'s digits above `shift` (the digits below are the pattern's zeros)
__device__ __forceinline__ uint32_t bits_of_key(uint32_t k, int shift) {
  const uint32_t low = shift ? ((1u << shift) - 1u) : 0u;
  return (k & 0x80000000u) ? (k & 0x7FFFFFFFu & ~low) : (~k & ~low);
}
__device__ __forceinline__ uint32_t widen(uint32_t v) { return v; }
__device__ __forceinline__ uint32_t widen(uint16_t v) { return (uint32_t)v << 16; }

// A lane's 16 elements of chunk c as fp32 bit patterns, -0 rewritten to +0; returns the mask of those inside the tensor
// (the others read as +0).  U: uint32_t (fp32) or uint16_t (bf16).
template <typename U>
__device__ __forceinline__ uint32_t load_chunk(const U *__restrict__ x, int64_t numel, int64_t c, bool aligned,
                                               uint32_t (&u)[kPerLane]) {
  constexpr int EP = Piece<U>::N, SUB = kPerLane / EP;
  const int64_t base = c * kChunk;
  uint32_t valid = 0;
  if (aligned && base + kChunk <= numel) {
    Piece<U> p[SUB];
#pragma unroll
    for (int s = 0; s < SUB; ++s) p[s] = *(const Piece<U> *)(x + base + ((int64_t)s * kThreads + threadIdx.x) * EP);
#pragma unroll
    for (int s = 0; s < SUB; ++s)
#pragma unroll
      for (int e = 0; e < EP; ++e) u[s * EP + e] = widen(p[s].e[e]);
    valid = 0xFFFFu;
  } else {
#pragma unroll
    for (int s = 0; s < SUB; ++s) {
      const int64_t i0 = base + ((int64_t)s * kThreads + threadIdx.x) * EP;
#pragma unroll
      for (int e = 0; e < EP; ++e) {
        const bool in = i0 + e < numel;
        u[s * EP + e] = in ? widen(x[i0 + e]) : 0u;
        valid |= (uint32_t)in << (s * EP + e);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < kPerLane; ++e) u[e] = u[e] == 0x80000000u ? 0u : u[e];
  return valid;
}
__device__ __forceinline__ uint32_t load_chunk(const ampconv_stats_tensor_t &d, int64_t c, uint32_t (&u)[kPerLane]) {
  const bool aligned = ((uintptr_t)d.x & 15) == 0;
  return d.dtype == AMPCONV_BF16 ? load_chunk((const uint16_t *)d.x, d.numel, c, aligned, u)
                                 : load_chunk((const uint32_t *)d.x, d.numel, c, aligned, u);
}

// ---- wave butterflies (every lane ends with the result; wave_sum_f64 is common.h's)
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, o, 64);
  return x;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, o, 64);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t y = (uint32_t)__shfl_xor((int)x, o, 64);
    x = y > x ? y : x;
  }
  return x;
}

// ---- moments
__device__ __forceinline__ void combine(Partial &a, const Partial &b) {
  a.sum += b.sum;
  a.sum_abs += b.sum_abs;
  a.sum_sq += b.sum_sq;
  a.finite += b.finite;
  a.nan += b.nan;
  a.inf += b.inf;
  a.zero += b.zero;
  a.negative += b.negative;
  a.kmin = b.kmin < a.kmin ? b.kmin : a.kmin;
  a.kmax = b.kmax > a.kmax ? b.kmax : a.kmax;
  a.amax = b.amax > a.amax ? b.amax : a.amax;
}
__device__ __forceinline__ Partial empty_partial() { return Partial{0., 0., 0., 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0u, 0u, 0u}; }

// slots[blockIdx.x] = the workgroup's share of its tensor
__global__ __launch_bounds__(kThreads) void stats_moments_chunks(const Launch L, Partial *__restrict__ slots) {
  __shared__ Partial red[kThreads / 64];
  const int ti = tensor_of(L, (int)blockIdx.x);
  const ampconv_stats_tensor_t d = L.t[ti];
  const int nwg = L.first[ti + 1] - L.first[ti];
  const int64_t nchunks = (d.numel + kChunk - 1) / kChunk;
  double s = 0., sa = 0., sq = 0.;
  uint32_t nfin = 0, nnan = 0, ninf = 0, nzero = 0, nneg = 0, kmin = 0xFFFFFFFFu, kmax = 0u, amax = 0u;
  for (int64_t c = (int)blockIdx.x - L.first[ti]; c < nchunks; c += nwg) {
    uint32_t u[kPerLane];
    const uint32_t valid = load_chunk(d, c, u);
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
      const bool in = (valid >> e) & 1u, fin = in && finite_bits(u[e]);
      const bool frac = (u[e] & 0x007FFFFFu) != 0;
      nfin += fin;
      nnan += in && !fin && frac;
      ninf += in && !fin && !frac;
      const uint32_t f = fin ? u[e] : 0u;                     // from here on: a finite pattern
      nzero += fin && f == 0u;
      nneg += f >> 31;
      const uint32_t k = key_of(f), a = f & 0x7FFFFFFFu;
      kmin = fin && k < kmin ? k : kmin;
      kmax = fin && k > kmax ? k : kmax;
      amax = a > amax ? a : amax;
      const double x = (double)__builtin_bit_cast(float, f);
      s += x;
      sa += (double)__builtin_bit_cast(float, a);
      sq += x * x;                                            // the square of an fp32 value is exact in fp64
    }
  }
  Partial p;
  p.sum = wave_sum_f64(s);
  p.sum_abs = wave_sum_f64(sa);
  p.sum_sq = wave_sum_f64(sq);
  p.finite = wave_sum_u64(nfin);
  p.nan = wave_sum_u64(nnan);
  p.inf = wave_sum_u64(ninf);
  p.zero = wave_sum_u64(nzero);
  p.negative = wave_sum_u64(nneg);
  p.kmin = wave_min_u32(kmin);
  p.kmax = wave_max_u32(kmax);
  p.amax = wave_max_u32(amax);
  p.pad = 0;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial t = red[0];
#pragma unroll
    for (int w = 1; w < kThreads / 64; ++w) combine(t, red[w]);
    slots[blockIdx.x] = t;
  }
}

// records[blockIdx.x] from the slots of tensor blockIdx.x in ascending order: kThreads consecutive runs, then the run sums
__global__ __launch_bounds__(kThreads) void stats_moments_finish(const Launch L, const Partial *__restrict__ slots,
                                                                 ampconv_stats_record_t *__restrict__ records) {
  __shared__ Partial part[kThreads];
  const int ti = (int)blockIdx.x;
  if (ti >= L.count) return;
  const int n = L.first[ti + 1] - L.first[ti];
  const Partial *mine = slots + L.first[ti];
  const int per = (n + kThreads - 1) / kThreads;
  const int b0 = (int)threadIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
  Partial p = empty_partial();
  for (int b = b0; b < b1; ++b) combine(p, mine[b]);
  part[threadIdx.x] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    Partial t = empty_partial();
    for (int r = 0; r < kThreads; ++r) combine(t, part[r]);
    ampconv_stats_record_t rec;
    rec.numel = L.t[ti].numel;
    rec.finite = (int64_t)t.finite;
    rec.nan = (int64_t)t.nan;
    rec.inf = (int64_t)t.inf;
    rec.zero = (int64_t)t.zero;
    rec.negative = (int64_t)t.negative;
    rec.sum = t.sum;
    rec.sum_abs = t.sum_abs;
    rec.sum_sq = t.sum_sq;
    const uint32_t none = 0x7FC00000u;                        // NaN: no finite element
    rec.min = __builtin_bit_cast(float, t.finite ? bits_of_key(t.kmin, 0) : none);
    rec.max = __builtin_bit_cast(float, t.finite ? bits_of_key(t.kmax, 0) : none);
    rec.absmax = __builtin_bit_cast(float, t.finite ? t.amax : none);
    rec.reserved = 0.f;
    records[ti] = rec;
  }
}

// ---- counting: LDS tables, two binning policies
// table[idx] += 1 for every lane with `on`; the lanes that share the first such lane's entry are counted by a ballot and
// added by that lane at once.  Called by all lanes of a wave together.
__device__ __forceinline__ void lds_add(uint32_t *table, int idx, bool on) {
#ifdef AMPCONV_STATS_NO_AGG
  if (on) atomicAdd(&table[idx], 1u);
#else
  const uint64_t any = __ballot(on);
  if (any == 0) return;                                       // wave-uniform
  const int leader = __ffsll((unsigned long long)any) - 1;
  const int lead_idx = __shfl(idx, leader, 64);
  const bool same = on && idx == lead_idx;
  const uint64_t mates = __ballot(same);
  if ((int)(threadIdx.x & 63) == leader) atomicAdd(&table[lead_idx], (uint32_t)__popcll((unsigned long long)mates));
  else if (on && !same) atomicAdd(&table[idx], 1u);
#endif
}

// the value histogram: entries 0 .. bins - 1 the bins, `bins` below lo, bins + 1 above hi (include/ampconv.h, THE BIN RULE)
struct ValueBins {
  static constexpr int kTable = kMaxBins + 2;
  int bins;
  const float *range;                                         // per tensor (lo, hi), or nullptr: the record's min, max
  const ampconv_stats_record_t *records;
  struct Ctx {
    float lo, hi, scale;
    int bins;
  };
  __device__ __forceinline__ Ctx setup(int ti, int) const {
    Ctx c;
    c.lo = range ? range[2 * ti] : records[ti].min;
    c.hi = range ? range[2 * ti + 1] : records[ti].max;
    c.scale = c.hi == c.lo ? 0.f : __fdiv_rn((float)bins, __fsub_rn(c.hi, c.lo));
    c.bins = bins;
    return c;
  }
  __device__ __forceinline__ int used(const Ctx &c) const { return c.bins + 2; }
  __device__ __forceinline__ int64_t offset(int ti) const { return (int64_t)ti * (bins + 2); }
  __device__ __forceinline__ void add(const Ctx &c, uint32_t *table, uint32_t f, bool fin) const {
    const float x = __builtin_bit_cast(float, f);             // f is a finite pattern (+0 for what is not counted)
    const float top = (float)(c.bins - 1);                    // clamped as a float first: the conversion cannot overflow
    int b = (int)floorf(fmaxf(fminf(__fmul_rn(__fsub_rn(x, c.lo), c.scale), top), 0.f));
    b = b < 0 ? 0 : b;
    b = b > c.bins - 1 ? c.bins - 1 : b;                      // integer clamps: in bounds whatever the range was
    const int idx = x < c.lo ? c.bins : (x > c.hi ? c.bins + 1 : b);
    lds_add(table, idx, fin);
  }
};

// a digit pass of the radix select: for every rank r, entry r * kDigits + digit for the elements whose key has the digits
// chosen so far for r; ranks with equal prefixes share the table of the first of them
struct DigitBins {
  static constexpr int kTable = kRanks * kDigits;
  int nq, pass;
  const SelState *state;
  struct Ctx {
    uint32_t prefix[kRanks];
    bool own[kRanks];                                         // rank r has a table of its own
    int prev, shift, nq;
    uint32_t mask;
  };
  // digit pass p of a dtype: the key's bits [shift, prev); false if the dtype has no such pass
  __host__ __device__ static bool plan(int dtype, int pass, int &prev, int &shift) {
    const int f32[4] = {32, 21, 10, 0}, b16[3] = {32, 21, 16};
    if (pass < 0 || pass >= (dtype == AMPCONV_BF16 ? 2 : 3)) return false;
    prev = dtype == AMPCONV_BF16 ? b16[pass] : f32[pass];
    shift = dtype == AMPCONV_BF16 ? b16[pass + 1] : f32[pass + 1];
    return true;
  }
  __device__ __forceinline__ Ctx setup(int ti, int dtype) const {
    Ctx c;
    plan(dtype, pass, c.prev, c.shift);
    c.mask = (1u << (c.prev - c.shift)) - 1u;
    c.nq = nq;
#pragma unroll
    for (int r = 0; r < kRanks; ++r) {
      c.prefix[r] = (pass > 0 && r < nq) ? state[ti * kRanks + r].prefix : 0u;
      c.own[r] = r < nq;
#pragma unroll
      for (int q = 0; q < r; ++q) c.own[r] = c.own[r] && c.prefix[q] != c.prefix[r];
    }
    return c;
  }
  __device__ __forceinline__ int used(const Ctx &c) const { return c.nq * kDigits; }
  __device__ __forceinline__ int64_t offset(int ti) const { return (int64_t)ti * kTable; }
  __device__ __forceinline__ void add(const Ctx &c, uint32_t *table, uint32_t f, bool fin) const {
    const uint32_t k = key_of(f);
    const uint32_t head = c.prev >= 32 ? 0u : k >> c.prev;
    const int digit = (int)((k >> c.shift) & c.mask);
#pragma unroll
    for (int r = 0; r < kRanks; ++r)
      if (c.own[r]) lds_add(table + r * kDigits, digit, fin && head == c.prefix[r]);      // own[]: workgroup-uniform
  }
};

template <typename P>
__global__ __launch_bounds__(kThreads) void stats_count(const Launch L, const P pol, unsigned long long *__restrict__ counts) {
  __shared__ uint32_t table[P::kTable];
  const int ti = tensor_of(L, (int)blockIdx.x);
  const ampconv_stats_tensor_t d = L.t[ti];
  const int nwg = L.first[ti + 1] - L.first[ti];
  const int64_t nchunks = (d.numel + kChunk - 1) / kChunk;
  const typename P::Ctx ctx = pol.setup(ti, d.dtype);
  const int used = pol.used(ctx);
  unsigned long long *out = counts + pol.offset(ti);
  for (int i = threadIdx.x; i < used; i += kThreads) table[i] = 0u;
  __syncthreads();
  auto flush = [&]() {
    __syncthreads();
    for (int i = threadIdx.x; i < used; i += kThreads) {
      const uint32_t v = table[i];
      if (v) {
        atomicAdd(out + i, (unsigned long long)v);
        table[i] = 0u;
      }
    }
    __syncthreads();
  };
  int since = 0;
  for (int64_t c = (int)blockIdx.x - L.first[ti]; c < nchunks; c += nwg) {
    uint32_t u[kPerLane];
    const uint32_t valid = load_chunk(d, c, u);
#pragma unroll
    for (int e = 0; e < kPerLane; ++e) {
      const bool fin = ((valid >> e) & 1u) && finite_bits(u[e]);
      pol.add(ctx, table, fin ? u[e] : 0u, fin);
    }
    if (++since == kFlushEvery) {                             // workgroup-uniform
      flush();
      since = 0;
    }
  }
  flush();
}

// After digit pass `pass`: for every rank of tensor blockIdx.x, the digit under which its rank falls; the last pass of a
// dtype writes the element.  Leaves the tensor's tables zeroed for the next pass.
__global__ __launch_bounds__(kThreads) void stats_select_pick(const Launch L, int pass, int nq, double q0, double q1, double q2,
                                                              double q3, const ampconv_stats_record_t *__restrict__ records,
                                                              SelState *__restrict__ state,
                                                              unsigned long long *__restrict__ counts,
                                                              float *__restrict__ out) {
  __shared__ unsigned long long part[kThreads];
  const int ti = (int)blockIdx.x;
  if (ti >= L.count) return;
  int prev, shift;
  if (!DigitBins::plan(L.t[ti].dtype, pass, prev, shift)) return;
  int nprev, nshift;
  const bool last = !DigitBins::plan(L.t[ti].dtype, pass + 1, nprev, nshift);
  const int bits = prev - shift, entries = 1 << bits;
  const int64_t finite = records[ti].finite;
  const double q[kRanks] = {q0, q1, q2, q3};
  unsigned long long *tables = counts + (int64_t)ti * DigitBins::kTable;
  uint32_t prefix[kRanks];
  for (int r = 0; r < kRanks; ++r) prefix[r] = (pass > 0 && r < nq) ? state[ti * kRanks + r].prefix : 0u;
  __syncthreads();                                            // every lane has the prefixes before lane 0 rewrites them
  for (int r = 0; r < nq; ++r) {
    int a = r;                                                // the table that rank r's elements were counted in
    for (int p = r - 1; p >= 0; --p) a = prefix[p] == prefix[r] ? p : a;
    const unsigned long long *T = tables + a * kDigits;
    constexpr int kRun = kDigits / kThreads;                  // 8 consecutive entries per lane
    unsigned long long s = 0;
    for (int j = 0; j < kRun; ++j) {
      const int i = (int)threadIdx.x * kRun + j;
      s += i < entries ? T[i] : 0ull;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long k = 0;
      if (pass == 0) k = finite > 0 ? (unsigned long long)floor(__dmul_rn(q[r], (double)(finite - 1))) : 0ull;
      else k = state[ti * kRanks + r].k;
      unsigned long long before = 0;
      int run = 0;
      for (; run < kThreads - 1 && before + part[run] <= k; ++run) before += part[run];
      int dgt = run * kRun;
      const int end = dgt + kRun - 1 < entries - 1 ? dgt + kRun - 1 : entries - 1;
      dgt = dgt < entries - 1 ? dgt : entries - 1;
      for (; dgt < end && before + T[dgt] <= k; ++dgt) before += T[dgt];
      const uint32_t chosen = (bits >= 32 ? 0u : prefix[r] << bits) | (uint32_t)dgt;
      state[ti * kRanks + r] = SelState{k >= before ? k - before : 0ull, chosen, 0u};
      if (last) {
        const uint32_t v = finite > 0 ? bits_of_key(chosen << shift, shift) : 0x7FC00000u;
        out[(int64_t)ti * nq + r] = __builtin_bit_cast(float, v);
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < nq * kDigits; i += kThreads) tables[i] = 0ull;
}

// ---- host
inline int64_t blocks_of(int64_t numel) {
  const int64_t chunks = (numel + kChunk - 1) / kChunk;
  return chunks < kMaxBlocks ? chunks : kMaxBlocks;
}

inline int tensors_ok(const ampconv_stats_tensor_t *t, int n) {
  if (n < 0 || (n > 0 && !t)) return AMPCONV_E_BADARG;
  for (int i = 0; i < n; ++i) {
    if (t[i].numel < 0 || t[i].numel > kMaxNumel || (t[i].numel > 0 && !t[i].x)) return AMPCONV_E_BADARG;
    if (t[i].dtype != AMPCONV_F32 && t[i].dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  }
  return AMPCONV_OK;
}

// the launch block of up to kMax descriptors; `takes(tensor)` says whether a tensor gets workgroups in this pass
template <typename Takes>
Launch make_launch(const ampconv_stats_tensor_t *t, int cnt, const Takes &takes) {
  Launch L = {};
  int32_t blocks = 0;
  for (int i = 0; i < kMax; ++i) {
    L.first[i] = blocks;
    if (i < cnt) {
      L.t[i] = t[i];
      if (takes(t[i])) blocks += (int32_t)blocks_of(t[i].numel);
    }
  }
  L.first[kMax] = blocks;
  L.count = cnt;
  return L;
}
inline bool every_tensor(const ampconv_stats_tensor_t &) { return true; }

// f(launch block, its workgroups, index of its first tensor, workgroups of the batches before it) for each batch of up to
// kMax descriptors.  A batch without workgroups is still handed over (blocks == 0): its finishing kernel has records to
// write.
template <typename F>
int for_each_batch(const ampconv_stats_tensor_t *t, int n, const F &f) {
  int64_t before = 0;
  for (int base = 0; base < n; base += kMax) {
    const Launch L = make_launch(t + base, n - base < kMax ? n - base : kMax, every_tensor);
    if (int rc = f(L, L.first[kMax], base, before)) return rc;
    before += L.first[kMax];
  }
  return AMPCONV_OK;
}

inline size_t moments_bytes(const ampconv_stats_tensor_t *t, int n) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += blocks_of(t[i].numel);
  return (size_t)total * sizeof(Partial);
}
inline size_t select_state_bytes(int n) { return (size_t)(n < kMax ? n : kMax) * kRanks * sizeof(SelState); }
inline size_t select_table_bytes(int n) { return (size_t)(n < kMax ? n : kMax) * DigitBins::kTable * sizeof(uint64_t); }

}  // namespace

extern "C" size_t ampconv_stats_workspace_bytes(const ampconv_stats_tensor_t *t, int n) {
  if (tensors_ok(t, n) != AMPCONV_OK || n == 0) return 0;
  const size_t a = moments_bytes(t, n), b = select_state_bytes(n) + select_table_bytes(n);
  return a > b ? a : b;
}

extern "C" int ampconv_stats_moments(const ampconv_stats_tensor_t *t, int n, ampconv_stats_record_t *records,
                                     void *workspace, size_t workspace_bytes, void *stream) {
  if (int rc = tensors_ok(t, n)) return rc;
  if (n == 0) return AMPCONV_OK;
  if (!records) return AMPCONV_E_BADARG;
  const size_t need = moments_bytes(t, n);
  if (need > 0 && (!workspace || workspace_bytes < need)) return AMPCONV_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  Partial *slots = (Partial *)workspace;
  return for_each_batch(t, n, [&](const Launch &L, int32_t blocks, int base, int64_t before) -> int {
                          if (blocks > 0) {
                            stats_moments_chunks<<<blocks, kThreads, 0, s>>>(L, slots + before);
                            if (int rc = ampconv_launch_status()) return rc;
                          }
                          stats_moments_finish<<<kMax, kThreads, 0, s>>>(L, slots + before, records + base);
                          return ampconv_launch_status();
                        });
}

extern "C" int ampconv_stats_histogram(const ampconv_stats_tensor_t *t, int n, int bins, const float *range,
                                       const ampconv_stats_record_t *records, uint64_t *counts, void *stream) {
  if (int rc = tensors_ok(t, n)) return rc;
  if (bins < 1 || bins > kMaxBins) return AMPCONV_E_BADARG;
  if (n == 0) return AMPCONV_OK;
  if (!counts || (!range && !records)) return AMPCONV_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  return for_each_batch(t, n, [&](const Launch &L, int32_t blocks, int base, int64_t) -> int {
                          if (blocks == 0) return AMPCONV_OK;
                          const ValueBins pol = {bins, range ? range + 2 * (int64_t)base : nullptr,
                                                 records ? records + base : nullptr};
                          stats_count<ValueBins><<<blocks, kThreads, 0, s>>>(
                              L, pol, (unsigned long long *)counts + (int64_t)base * (bins + 2));
                          return ampconv_launch_status();
                        });
}

extern "C" int ampconv_stats_select(const ampconv_stats_tensor_t *t, int n, const double *q, int nq,
                                    const ampconv_stats_record_t *records, float *out, void *workspace,
                                    size_t workspace_bytes, void *stream) {
  if (int rc = tensors_ok(t, n)) return rc;
  if (nq < 1 || nq > kRanks || !q) return AMPCONV_E_BADARG;
  double qs[kRanks] = {0., 0., 0., 0.};
  for (int r = 0; r < nq; ++r) {
    if (!(q[r] >= 0. && q[r] <= 1.)) return AMPCONV_E_BADARG;
    qs[r] = q[r];
  }
  if (n == 0) return AMPCONV_OK;
  if (!records || !out) return AMPCONV_E_BADARG;
  const size_t state_bytes = select_state_bytes(n), table_bytes = select_table_bytes(n);
  if (!workspace || workspace_bytes < state_bytes + table_bytes) return AMPCONV_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  SelState *state = (SelState *)workspace;
  unsigned long long *tables = (unsigned long long *)((char *)workspace + state_bytes);
  if (hipError_t e = hipMemsetAsync(tables, 0, table_bytes, s)) return (int)e;
  // batch by batch (the batches share the workspace), the digit passes of a batch one after the other; the pick kernel
  // leaves the tables zeroed for whatever comes next
  for (int base = 0; base < n; base += kMax) {
    const int cnt = n - base < kMax ? n - base : kMax;
    for (int pass = 0; pass < 3; ++pass) {
      const Launch L = make_launch(t + base, cnt, [pass](const ampconv_stats_tensor_t &d) {
        int prev, shift;
        return DigitBins::plan(d.dtype, pass, prev, shift);
      });
      bool any = false;
      for (int i = 0; i < cnt; ++i) {
        int prev, shift;
        any = any || DigitBins::plan(t[base + i].dtype, pass, prev, shift);
      }
      if (!any) break;
      if (L.first[kMax] > 0) {
        const DigitBins pol = {nq, pass, state};
        stats_count<DigitBins><<<L.first[kMax], kThreads, 0, s>>>(L, pol, tables);
        if (int rc = ampconv_launch_status()) return rc;
      }
      stats_select_pick<<<kMax, kThreads, 0, s>>>(L, pass, nq, qs[0], qs[1], qs[2], qs[3], records + base, state, tables,
                                                   out + (int64_t)base * nq);
      if (int rc = ampconv_launch_status()) return rc;
    }
  }
  return AMPCONV_OK;
}
