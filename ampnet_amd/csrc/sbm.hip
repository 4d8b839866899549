// Stochastic block model graphs drawn on the GPU (include/ampconv.h, "THE BLOCK MODEL"): the graph of the reference's
// create_xor_data (synthetic_benchmark/synthetic_xor.py:104-165: two nested Python loops over an [N, N] matrix) and of
// its Random_Partition_Graph (synthetic_rpg.py:39-121).  A unit (u, b) -- node u against block b -- walks the candidate
// range with geometric skips, so the work is proportional to the edges, not to the N^2 pairs.  Two passes over the same
// chains: count, the caller's exclusive scan, fill.  No atomics: every position is written by exactly one lane.
#include "common.h"

namespace {

constexpr int kSbmWaves = 4;      // waves per workgroup, one (64-node tile, block) pair each

struct SbmArgs {
  int64_t start[AMPCONV_SBM_MAX_K + 1];
  const double *P, *lq;
  int64_t *count, *mcount;        // count pass
  const int64_t *off, *moff;      // fill pass
  int64_t *row, *col;
  int64_t mirror_base, E;
  int64_t n_tiles;                // ceil(N / 64)
  uint64_t seed;
  int K, directed, selfloops;
};

// the block that holds node u: the largest b with start[b] <= u (empty blocks share their start with the next one)
__device__ __forceinline__ int sbm_block_of(const SbmArgs &a, int64_t u) {
  int lo = 0, hi = a.K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.start[mid] <= u) lo = mid; else hi = mid;
  }
  return lo;
}

// The chain of unit (u, b).  emit(v) is called for every edge (u, v) in ascending v; returns their number.  With
// kCount the p >= 1 units return their closed form without a call of emit, and `self` tells whether (u, u) is among
// the unit's edges.
template <bool kCount, typename Emit>
__device__ __forceinline__ int64_t sbm_walk(const SbmArgs &a, int64_t u, int b, bool &self, const Emit &emit) {
  const int bu = sbm_block_of(a, u);
  const double p = a.P[(int64_t)bu * a.K + b];
  int64_t lo = a.start[b];
  const int64_t hi = a.start[b + 1];
  bool hole = false;                  // directed, no self loops, u in block b: the candidates skip u
  if (a.directed) {
    hole = !a.selfloops && bu == b;
  } else {
    const int64_t first = u + (a.selfloops ? 0 : 1);
    lo = lo > first ? lo : first;
  }
  const int64_t m = hi - lo - (hole ? 1 : 0);
  self = false;
  if (m <= 0 || !(p > 0.0)) return 0;
  const bool has_u = a.selfloops && bu == b;      // u is a candidate (the first one of an undirected unit)
  if (p >= 1.0) {
    self = has_u;
    if (!kCount)
      for (int64_t j = 0; j < m; ++j) emit(lo + j + (hole && lo + j >= u ? 1 : 0));
    return m;
  }
  const double lq = a.lq[(int64_t)bu * a.K + b];
  const uint64_t unit = (uint64_t)u * (uint64_t)a.K + (uint64_t)b;
  int64_t j = -1, n = 0;
  for (uint64_t t = 0;; ++t) {
    const uint64_t r = draw(a.seed, unit, t);
    const double U = (double)((r >> 11) + 1) * 0x1p-53;
    const double q = log(U) / lq;
    if (!(q < (double)(m - 1 - j))) break;       // in fp64: q is unbounded, its integer part need not fit
    j += 1 + (int64_t)floor(q);
    const int64_t v = lo + j + (hole && lo + j >= u ? 1 : 0);
    self |= has_u && v == u;
    emit(v);
    ++n;
  }
  return n;
}

// wave -> (tile of 64 consecutive nodes, block b), b fastest: the K waves of a tile share block(u) and the P row
__device__ __forceinline__ bool sbm_unit(const SbmArgs &a, int64_t &u, int &b) {
  const int64_t w = (int64_t)blockIdx.x * kSbmWaves + (threadIdx.x >> 6);
  const int64_t tile = w / a.K;
  b = (int)(w - tile * a.K);
  u = tile * 64 + (threadIdx.x & 63);
  return tile < a.n_tiles && u < a.start[a.K];
}

__global__ __launch_bounds__(64 * kSbmWaves) void sbm_count_kernel(const SbmArgs a) {
  int64_t u;
  int b;
  if (!sbm_unit(a, u, b)) return;
  bool self;
  const int64_t n = sbm_walk<true>(a, u, b, self, [](int64_t) {});
  a.count[u * a.K + b] = n;
  if (a.mcount) a.mcount[u * a.K + b] = n - (self ? 1 : 0);
}

__global__ __launch_bounds__(64 * kSbmWaves) void sbm_fill_kernel(const SbmArgs a) {
  int64_t u;
  int b;
  if (!sbm_unit(a, u, b)) return;
  int64_t pos = a.off[u * a.K + b];
  int64_t mpos = a.moff ? a.mirror_base + a.moff[u * a.K + b] : -1;
  bool self;
  sbm_walk<false>(a, u, b, self, [&](int64_t v) {
    if (pos >= 0 && pos < a.E) {
      a.row[pos] = u;
      a.col[pos] = v;
    }
    ++pos;
    if (a.moff && v != u) {
      if (mpos >= 0 && mpos < a.E) {
        a.row[mpos] = v;
        a.col[mpos] = u;
      }
      ++mpos;
    }
  });
}

// the arguments both passes share; false: refused
bool sbm_args(const int64_t *sizes, int K, const double *P, const double *lq, int directed, int selfloops, uint64_t seed,
              SbmArgs &a) {
  if (!sizes || K < 1 || K > AMPCONV_SBM_MAX_K || !aligned8(P) || !aligned8(lq)) return false;
  a.start[0] = 0;
  for (int b = 0; b < K; ++b) {
    if (sizes[b] < 0 || sizes[b] > INT32_MAX) return false;
    a.start[b + 1] = a.start[b] + sizes[b];
    if (a.start[b + 1] > INT32_MAX) return false;
  }
  for (int b = K + 1; b <= AMPCONV_SBM_MAX_K; ++b) a.start[b] = a.start[K];
  a.P = P;
  a.lq = lq;
  a.count = a.mcount = nullptr;
  a.off = a.moff = nullptr;
  a.row = a.col = nullptr;
  a.mirror_base = a.E = 0;
  a.n_tiles = (a.start[K] + 63) / 64;
  a.seed = seed;
  a.K = K;
  a.directed = directed != 0;
  a.selfloops = selfloops != 0;
  return true;
}

int sbm_launch(void (*kernel)(const SbmArgs), const SbmArgs &a, void *stream) {
  if (a.n_tiles == 0) return AMPCONV_OK;
  const int64_t blocks = (a.n_tiles * a.K + kSbmWaves - 1) / kSbmWaves;
  if (blocks > INT32_MAX) return AMPCONV_E_BADARG;
  kernel<<<dim3((unsigned)blocks), dim3(64 * kSbmWaves), 0, (hipStream_t)stream>>>(a);
  return ampconv_launch_status();
}

}  // namespace

extern "C" int ampconv_sbm_count(const int64_t *sizes, int K, const double *P, const double *lq, int directed,
                                 int selfloops, uint64_t seed, int64_t *count, int64_t *mcount, void *stream) {
  SbmArgs a;
  if (!sbm_args(sizes, K, P, lq, directed, selfloops, seed, a) || !aligned8(count) || (mcount && !aligned8(mcount)))
    return AMPCONV_E_BADARG;
  a.count = count;
  a.mcount = mcount;
  return sbm_launch(sbm_count_kernel, a, stream);
}

extern "C" int ampconv_sbm_fill(const int64_t *sizes, int K, const double *P, const double *lq, int directed, int selfloops,
                                uint64_t seed, const int64_t *off, const int64_t *moff, int64_t mirror_base, int64_t *row,
                                int64_t *col, int64_t E, void *stream) {
  SbmArgs a;
  if (!sbm_args(sizes, K, P, lq, directed, selfloops, seed, a) || !aligned8(off) || (moff && !aligned8(moff)) ||
      !aligned8(row) || !aligned8(col) || E < 0 || mirror_base < 0)
    return AMPCONV_E_BADARG;
  a.off = off;
  a.moff = moff;
  a.row = row;
  a.col = col;
  a.mirror_base = mirror_base;
  a.E = E;
  return sbm_launch(sbm_fill_kernel, a, stream);
}
