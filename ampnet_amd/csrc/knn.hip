// k nearest neighbours over node embeddings (include/ampconv.h, "nearest neighbours"): the [Q, S] scores tiled on chip,
// the best k of every query kept in LDS, [Q, k] written.
//
// The scores are pair_loss.hip's forward product: a wave keeps 16 QUERY rows in registers and walks the KEY rows in 32-row
// LDS tiles that the four waves of a workgroup share (ids two tiles ahead, rows one, nothing looked at before it is in
// LDS), v_mfma_f32_16x16x4_f32 on K zero-padded to 16 KQ4 channels: C/D lane (r, g), reg q = <query r, key 4 g + q>.
// COSINE and L2 take a per-node term (1 / norm, squared norm) that a pre-pass writes to the workspace.
//
// Selection.  A pair's goodness g and its key POSITION s fold into one 64-bit key -- high word: the order-preserving
// unsigned image of g (-0 as +0), low word: ~s -- so "better" in the order (g descending, s ascending) is one unsigned
// compare and 0 is free for "no candidate" (the image of -inf is 0x007FFFFF).  Every query row owns a list of k keys in
// LDS, sorted best first; its last entry is the row's threshold, held in registers by the row's four lanes.  After a
// sub-tile a lane tests its four keys against the threshold and a wave-wide ballot skips everything else when no lane has
// a survivor.  Survivors are placed one at a time by the whole wave (list_place: lane j writes the new entry j, one LDS
// round trip whatever k is); then the row's lanes re-read the threshold.  The order is strict, so the list a row ends with
// does not depend on the order its candidates arrived in.
// The key range is split over blockIdx.y where Q alone does not fill the card: every split writes its lists as keys
// [split][Q][k] and knn_merge_kernel takes the best k of a row's partials.  No atomics anywhere.
#include "row_stream.h"

namespace {

constexpr int kThreads = 256;      // four waves = 64 query rows per workgroup

struct KnnArgs {
  const void *Z;
  int64_t ldz, N;
  int D, bf16, vec;
  const int64_t *qid, *kid;          // node ids, or nullptr: the position is the node
  int64_t nq, ns;
  int tiles, tiles_per_split, k, metric, exclude;
  const float *aux;                  // per node: 1 / norm (COSINE), squared norm (L2); nullptr for DOT
  unsigned long long *part;          // [split][nq][k] keys, or nullptr: one split, decoded at once
  int64_t *idx;
  float *score;
  int32_t *oob;
};

__device__ __forceinline__ unsigned float_image(unsigned u) {      // bits of a non-NaN float -> unsigned, same order
  u = u == 0x80000000u ? 0u : u;                                   // -0 counts as +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float image_float(unsigned h) {
  return __uint_as_float((h & 0x80000000u) ? (h & 0x7FFFFFFFu) : ~h);
}

// slot `at` of the output from a key: node id and score, or the empty slot
__device__ __forceinline__ void emit(const KnnArgs &a, int64_t at, unsigned long long key) {
  const bool l2 = a.metric == AMPCONV_KNN_L2;
  if (key == 0ull) {
    a.idx[at] = -1;
    a.score[at] = l2 ? __builtin_inff() : -__builtin_inff();
    return;
  }
  int64_t s = (int64_t)(~(unsigned)key);
  s = s < a.ns ? s : a.ns - 1;                                     // a key is built from s < ns: bounded again by construction
  const float g = image_float((unsigned)(key >> 32));
  a.idx[at] = a.kid ? clamp_id(a.kid[s], a.N) : s;
  a.score[at] = l2 ? 0.f - g : g;
}

// the key of lane `src` (wave-uniform) in every lane
__device__ __forceinline__ unsigned long long lane_key(unsigned long long v, int src) {
  const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, src), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), src);
  return ((unsigned long long)hi << 32) | lo;
}

// One list (sorted best first, k <= 64 entries), the whole wave: the key takes its place and the last entry falls out.
// Lane j < k writes the new entry j: the old one while that beats the key, else the key where the entry in front still beats
// it, else the entry in front.  A key that does not beat the last entry leaves the list as it is.  Both reads of every
// lane are issued in front of the store, and a wave's LDS operations complete in order.
__device__ __forceinline__ void list_place(unsigned long long *R, int k, int lane, unsigned long long key) {
  unsigned long long cur = 0ull, prv = ~0ull;
  if (lane < k) {
    cur = R[lane];
    if (lane > 0) prv = R[lane - 1];
  }
  __builtin_amdgcn_wave_barrier();
  if (lane < k) R[lane] = cur > key ? cur : (prv > key ? key : prv);
}

template <int KQ4>
__global__ __launch_bounds__(kThreads) void knn_kernel(const KnnArgs a) {
  constexpr int KQ = 4 * KQ4, DP = 16 * KQ4, LDR = DP + 4, CH = DP / 4;
  constexpr int XCH = KQ4 < 8 ? KQ4 : 8;               // row-operand chunks in flight
  constexpr int NL = (kTS * CH + kThreads - 1) / kThreads;
  // all LDS is the dynamic region (knn_lds_bytes): the key tile, its ids and per-key terms, then the 64 lists of k keys --
  // what a workgroup holds follows k, not AMPCONV_KNN_MAX_K.  Every carve offset is a multiple of 16 bytes.
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
  float *tile = reinterpret_cast<float *>(knn_lds);
  int *s_id = reinterpret_cast<int *>(knn_lds + sizeof(float) * kTS * LDR);
  float *s_aux = reinterpret_cast<float *>(s_id + kTS);
  unsigned long long *s_list = reinterpret_cast<unsigned long long *>(s_aux + kTS);   // row (wave, r) at (16 wave + r) k

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int64_t fr = ((int64_t)blockIdx.x * (kThreads / 64) + wave) * 16 + r;
  const bool valid_f = fr < a.nq;
  const int sp = blockIdx.y;
  const int64_t fr0 = valid_f ? fr : 0;
  const int64_t fidc = clamp_id(a.qid ? a.qid[fr0] : fr0, a.N);
  const int k = a.k;

  float fx[KQ];
#pragma unroll
  for (int j = 0; j < KQ4; ++j) {
    const float4 v = load4(a, fidc, g * KQ + 4 * j);
    fx[4 * j] = v.x; fx[4 * j + 1] = v.y; fx[4 * j + 2] = v.z; fx[4 * j + 3] = v.w;
  }
  const float aux_f = a.aux ? a.aux[fidc] : 0.f;

  unsigned long long *L = s_list + (16 * wave + r) * k;
  for (int i = lane; i < 16 * k; i += 64) s_list[16 * wave * k + i] = 0ull;
  unsigned long long thr = 0ull;                        // the list's last entry: what a key has to beat

  const int t0 = sp * a.tiles_per_split, t1 = min(t0 + a.tiles_per_split, a.tiles);

  // as in pair_kernel: rows one tile ahead in registers, their ids two; nothing asked for is looked at before the next
  // iteration
  uint4 pf[NL];
  int64_t rid[NL];
  int64_t nx_id = 0;
  int pf_id = -1;
  float pf_aux = 0.f;
  auto load_ids = [&](int t) {
#pragma unroll
    for (int kk = 0; kk < NL; ++kk) {
      const int i = tid + kThreads * kk, row = i / CH;
      const int64_t s = (int64_t)t * kTS + row, s0 = row < kTS && s < a.ns ? s : 0;
      rid[kk] = a.kid ? a.kid[s0] : s0;
    }
    if (tid < kTS) {
      const int64_t s = (int64_t)t * kTS + tid, s0 = s < a.ns ? s : 0;
      nx_id = a.kid ? a.kid[s0] : s0;
    }
  };
  auto load_rows = [&](int t) {
    by_path(a, [&](auto path) {
#pragma unroll
      for (int kk = 0; kk < NL; ++kk) {
        const int i = tid + kThreads * kk, row = i / CH, ch = i - row * CH;
        pf[kk] = raw4<decltype(path)::value>(a, clamp_id(rid[kk], a.N), 4 * ch);
      }
    });
    if (tid < kTS) {
      const int64_t s = (int64_t)t * kTS + tid, idc = clamp_id(nx_id, a.N);
      pf_id = s < a.ns ? (int)idc : -1;
      if (a.aux) pf_aux = a.aux[idc];
    }
  };

  if (t0 < t1) {                                        // S == 0: no tile, and no id to read
    load_ids(t0);
    load_rows(t0);
    load_ids(t0 + 1);
  }
  for (int t = t0; t < t1; ++t) {
    __syncthreads();
    by_path(a, [&](auto path) {
#pragma unroll
      for (int kk = 0; kk < NL; ++kk) {
        const int i = tid + kThreads * kk, row = i / CH, ch = i - row * CH;
        if (row < kTS)
          *reinterpret_cast<float4 *>(tile + row * LDR + 4 * ch) =
              cook4<decltype(path)::value>(a, pf[kk], 4 * ch, (int64_t)t * kTS + row < a.ns);
      }
    });
    if (tid < kTS) {
      s_id[tid] = pf_id;
      s_aux[tid] = pf_aux;
    }
    __syncthreads();
    if (t + 1 < t1) {
      load_rows(t + 1);
      load_ids(t + 2);
    }

    const int cnt = (int)min((int64_t)kTS, a.ns - (int64_t)t * kTS);
#pragma unroll
    for (int sub = 0; sub < kTS / 16; ++sub) {
      if (sub * 16 >= cnt) break;                       // workgroup-uniform
      const float *rowp = tile + (sub * 16 + r) * LDR + g * KQ;
      f32x4 lg = {0.f, 0.f, 0.f, 0.f}, lg1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j0 = 0; j0 < KQ4; j0 += XCH) {
        float4 xs[XCH];
#pragma unroll
        for (int j = 0; j < XCH; ++j)
          if (j0 + j < KQ4) xs[j] = *reinterpret_cast<const float4 *>(rowp + 4 * (j0 + j));
#pragma unroll
        for (int j = 0; j < XCH; ++j) {
          if (j0 + j >= KQ4) continue;
          lg = MFMA16(xs[j].x, fx[4 * (j0 + j)], lg);         // two chains: a dependent MFMA issues 8 cycles late
          lg1 = MFMA16(xs[j].y, fx[4 * (j0 + j) + 1], lg1);
          lg = MFMA16(xs[j].z, fx[4 * (j0 + j) + 2], lg);
          lg1 = MFMA16(xs[j].w, fx[4 * (j0 + j) + 3], lg1);
        }
      }
      lg += lg1;

      unsigned long long key[4];
      bool any = false;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int srow = sub * 16 + 4 * g + q;
        const int id = s_id[srow];                      // -1 behind the end of the key list
        float v = lg[q];                                // what is tested for NaN, then g
        if (a.metric == AMPCONV_KNN_COSINE) v = v * aux_f * s_aux[srow];
        else if (a.metric == AMPCONV_KNN_L2) v = fmaf(-2.f, v, aux_f + s_aux[srow]);
        unsigned u = __float_as_uint(v);
        asm volatile("" : "+v"(u));                     // the NaN test is on the bits: the build assumes NaN-free arithmetic
        const bool nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
        if (a.metric == AMPCONV_KNN_L2) u = __float_as_uint(-fmaxf(__uint_as_float(u), 0.f));
        const unsigned s = (unsigned)t * kTS + srow;    // < 2^31
        const bool cand = id >= 0 && valid_f && !nan && !(a.exclude && id == (int)fidc);
        key[q] = cand ? ((unsigned long long)float_image(u) << 32) | (unsigned)~s : 0ull;
        any |= key[q] > thr;
      }
      if (__ballot(any) != 0ull) {                      // after the first tiles: rarely
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          unsigned long long todo = __ballot(key[q] > thr);
          while (todo) {                                // wave-uniform: one survivor at a time, placed by the whole wave
            const int src = __ffsll(todo) - 1;
            todo &= todo - 1;
            list_place(s_list + (16 * wave + (src & 15)) * k, k, lane, lane_key(key[q], src));
          }
          thr = L[k - 1];
        }
      }
    }
  }

  __builtin_amdgcn_wave_barrier();
  if (valid_f) {
    for (int j = g; j < k; j += 4) {
      const unsigned long long key = L[j];
      if (a.part) a.part[((int64_t)sp * a.nq + fr) * k + j] = key;
      else emit(a, fr * k + j, key);
    }
  }
}

// the best k of a row's `splits` partial lists: one wave per query, one pass over the partials per output slot
__global__ __launch_bounds__(256) void knn_merge_kernel(const KnnArgs a, int splits) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= a.nq) return;                                // wave-uniform
  const int k = a.k, total = splits * k;
  unsigned long long prev = ~0ull;
  for (int j = 0; j < k; ++j) {
    unsigned long long best = 0ull;
    for (int i = lane; i < total; i += 64) {
      const int sp = i / k, jj = i - sp * k;
      const unsigned long long v = a.part[((int64_t)sp * a.nq + q) * k + jj];
      if (v < prev && v > best) best = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
    }
    if (lane == 0) emit(a, q * k + j, best);
    prev = best;                                        // 0: nothing is left, every later slot is empty
  }
}

// bounds flag of the id lists; per node 1 / max(norm, 1e-12) (COSINE) or the squared norm (L2): 16 lanes per row, lane l
// sums the channels l, l + 16, ... in order, then the lanes pairwise -- one fixed order per row
__global__ __launch_bounds__(256) void knn_prep_kernel(const KnnArgs a, float *aux) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  bool bad = false;
  if (a.qid)
    for (int64_t i = gid; i < a.nq; i += stride) bad |= a.qid[i] < 0 || a.qid[i] >= a.N;
  if (a.kid)
    for (int64_t i = gid; i < a.ns; i += stride) bad |= a.kid[i] < 0 || a.kid[i] >= a.N;
  if (bad) *a.oob = 1;
  if (a.metric == AMPCONV_KNN_DOT) return;
  const int l = (int)(gid & 15);
  for (int64_t row = gid >> 4; row < a.N; row += stride >> 4) {       // the 16 lanes of a row stay in the loop together
    float ss = 0.f;
    for (int c = l; c < a.D; c += 16) {
      const float x = a.bf16 ? bf16_f32(reinterpret_cast<const uint16_t *>(a.Z)[row * a.ldz + c])
                             : reinterpret_cast<const float *>(a.Z)[row * a.ldz + c];
      ss = fmaf(x, x, ss);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    if (l == 0) aux[row] = a.metric == AMPCONV_KNN_COSINE ? 1.f / fmaxf(sqrtf(ss), 1e-12f) : ss;
  }
}

// ---- host side
constexpr int64_t kMaxCount = INT32_MAX;

// rows of k keys the partial lists can take: splits * Q <= min(64, tiles) * Q and <= 32768 + Q (stream_split: at most
// ceil(2048 / waves) splits with Q <= 16 waves); either bound grows with Q and with S
int64_t part_rows(int64_t Q, int64_t S) {
  const int64_t tiles = (S + kTS - 1) / kTS;
  return std::min<int64_t>(std::min<int64_t>(tiles, 64) * Q, 32768 + Q);
}

constexpr size_t kLdsOptIn = 48 * 1024;             // a larger dynamic region is asked for per kernel

template <int KQ4>
int launch_kq(const KnnArgs &a, dim3 grid, hipStream_t stream) {
  // the kernel's carve: tile [kTS][16 KQ4 + 4] floats, kTS ids, kTS per-key terms, 64 lists of k keys
  const size_t lds = sizeof(float) * kTS * (16 * KQ4 + 4) + 2 * sizeof(float) * kTS + sizeof(unsigned long long) * 64 * a.k;
  if (lds > kLdsOptIn) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(knn_kernel<KQ4>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  knn_kernel<KQ4><<<grid, dim3(kThreads), lds, stream>>>(a);
  return ampconv_launch_status();
}

}  // namespace

extern "C" size_t ampconv_knn_workspace_bytes(int64_t Q, int64_t S, int64_t N, int D, int k) {
  if (Q <= 0 || S < 0 || N < 0 || D < 1 || D > AMPCONV_KNN_MAX_D || k < 1 || k > AMPCONV_KNN_MAX_K) return 0;
  if (Q > kMaxCount || S > kMaxCount || N > kMaxCount) return 0;
  return pad256((size_t)N * sizeof(float)) + pad256((size_t)part_rows(Q, S) * (size_t)k * sizeof(unsigned long long));
}

extern "C" int ampconv_knn(const void *X, int64_t N, int D, int64_t ldx, const int64_t *query, int64_t Q,
                           const int64_t *key, int64_t S, int k, int metric, int exclude_self, int64_t *idx,
                           float *score, int32_t *oob, void *workspace, size_t workspace_bytes, int dtype,
                           void *stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (Q < 0 || S < 0 || N < 0 || Q > kMaxCount || S > kMaxCount || N > kMaxCount) return AMPCONV_E_BADARG;
  if (D < 1 || D > AMPCONV_KNN_MAX_D || k < 1 || k > AMPCONV_KNN_MAX_K || ldx < D) return AMPCONV_E_BADARG;
  if (metric != AMPCONV_KNN_DOT && metric != AMPCONV_KNN_COSINE && metric != AMPCONV_KNN_L2) return AMPCONV_E_BADARG;
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_BADARG;
  if ((!query && Q != N && Q != 0) || (!key && S != N && S != 0)) return AMPCONV_E_BADARG;
  if (Q > 0 && (N < 1 || !X || !idx || !score || !oob)) return AMPCONV_E_BADARG;
  if (Q == 0) {
    if (oob) hipMemsetAsync(oob, 0, sizeof(int32_t), stream);
    return ampconv_launch_status();
  }
  if (!workspace || workspace_bytes < ampconv_knn_workspace_bytes(Q, S, N, D, k)) return AMPCONV_E_WORKSPACE;

  const Split sp = stream_split(Q, S, 0);
  KnnArgs a = {};
  a.Z = X; a.ldz = ldx; a.N = N; a.D = D;
  a.bf16 = dtype == AMPCONV_BF16;
  const size_t el = a.bf16 ? 2 : 4;
  a.vec = D % 4 == 0 && ldx % 4 == 0 && (uintptr_t)X % (4 * el) == 0;
  a.qid = query; a.kid = key; a.nq = Q; a.ns = S;
  a.tiles = sp.tiles; a.tiles_per_split = sp.per; a.k = k; a.metric = metric; a.exclude = exclude_self != 0;
  float *aux = (float *)workspace;
  a.aux = metric == AMPCONV_KNN_DOT ? nullptr : aux;
  a.part = sp.n > 1 ? (unsigned long long *)((char *)workspace + pad256((size_t)N * sizeof(float))) : nullptr;
  a.idx = idx; a.score = score; a.oob = oob;

  hipMemsetAsync(oob, 0, sizeof(int32_t), stream);
  if (metric != AMPCONV_KNN_DOT || query || key) {
    const int64_t work = std::max<int64_t>(metric != AMPCONV_KNN_DOT ? N * 16 : 0, std::max(query ? Q : 0, key ? S : 0));
    const int64_t blocks = std::min<int64_t>(std::max<int64_t>((work + 255) / 256, 1), 1 << 16);
    knn_prep_kernel<<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(a, aux);
    if (int rc = ampconv_launch_status()) return rc;
  }

  const dim3 grid((unsigned)((Q + 63) / 64), (unsigned)sp.n);
  const int kq4 = (D + 15) / 16;
  if (int rc = kq4 <= 1 ? launch_kq<1>(a, grid, stream) : kq4 <= 2 ? launch_kq<2>(a, grid, stream)
             : kq4 <= 4 ? launch_kq<4>(a, grid, stream) : kq4 <= 7 ? launch_kq<7>(a, grid, stream)
             : kq4 <= 8 ? launch_kq<8>(a, grid, stream) : launch_kq<16>(a, grid, stream))
    return rc;
  if (sp.n > 1) {
    knn_merge_kernel<<<dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, stream>>>(a, sp.n);
    return ampconv_launch_status();
  }
  return AMPCONV_OK;
}
