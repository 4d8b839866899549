// One-query-token edge family (include/ampconv.h, "edge phase, ONE query token"): the three edge passes of a layer whose
// output is read at a single token per node -- AMPGCN(average_pooling_flag=False) reads token 0 of conv2 and drops the
// rest (reference src/ampnet/module/amp_gcn.py:266-271).  Q, dObar, O and dQ hold ONE row of dh channels per (node,
// head); K, V, dK, dV hold L rows as everywhere else.
//
// The products are 1 x dh . dh x L: nothing for the matrix cores.  The passes are bound by the gather of the source's
// K and V tiles (forward, destination pass) or by nothing much (source pass: two dh-wide rows per edge), so the lane
// mapping is chosen for loads in flight and plain VALU arithmetic:
//   * one wave per (row, head) unit, map_unit's three modes (no plan / main pass / long-segment chunks) as in the
//     other families; no atomics, every output row has one owner, sums run in CSR / CSC order;
//   * forward / destination pass: per in-edge the K and V tiles go global -> registers -> LDS in the widest pieces
//     base and strides allow (16, 8, 4 or 2 bytes), 8 pieces per lane in flight; lane j then owns score j (its dot
//     products walk LDS rows of an odd stride: no bank conflict), the softmax is two wave reductions, and lane
//     (g, c) sums p_j V[j][c] (ds_j K[j][c]) over the rows j = g, g + G, ... of its group, G = 64 / (dh rounded up to
//     a power of two); the groups meet in a fixed xor tree once per row;
//   * source pass: K[s] and V[s] of the unit's OWN node are loaded once and stay in LDS; per out-edge the wave reads
//     the destination's q and dObar rows (one element per lane, coalesced), recomputes the length-L softmax and
//     sum p.dp from them -- no statistics hand-off -- and lane (g, c) keeps dK[j][c], dV[j][c] of its rows in
//     registers until the segment ends.
// fp32 softmax and accumulation; bf16 storage is widened on the way into LDS and rounded once on the way out.
#include "common.h"

namespace {

struct TokArgs {
  ampconv_view_t Q, K, V, dO, O, O2;      // O: O / dQ / dK, O2: dV
  const int32_t *ptr, *idx;               // rowptr, col (forward, destination pass) or cscptr, crow (source pass)
  const float *cinv;                      // source pass: 1 / in-degree of the destination of every CSC edge
  HubArgs hub;
  int64_t n_units;
  int L, dh, dhp, H;
  int gw, gshift;                         // lanes per group (dh rounded up to a power of two) and its log2
  int vec;                                // elements per K / V load piece
  int out_f32;                            // the outputs are fp32 whatever T says (partial tiles of the hub pass)
  float scale;                            // 1 / sqrt(dh)
};

__device__ __forceinline__ float to_f(float x) { return x; }
__device__ __forceinline__ float to_f(__bf16 x) { return (float)x; }

template <typename T>
__device__ __forceinline__ void store_out(void *base, int64_t off, float v, int out_f32) {
  if (out_f32)
    reinterpret_cast<float *>(base)[off] = v;
  else
    reinterpret_cast<T *>(base)[off] = (T)v;
}

template <typename T, int EPV>
struct Piece {
  typedef T type __attribute__((ext_vector_type(EPV)));
};
template <typename T>
struct Piece<T, 1> {
  typedef T type;
};
template <typename T, int EPV>
__device__ __forceinline__ float piece_at(const typename Piece<T, EPV>::type &v, int e) {
  if constexpr (EPV == 1)
    return to_f(v);
  else
    return to_f(v[e]);
}

// K and V tiles of one (node, head), L rows of dh channels, into LDS rows of dhp floats.  Pieces of EPV elements; the
// loads of U pieces of each tile are issued before the first is stored.  Every lane loads a valid address (the
// index is clamped, the store is predicated): a branch around a load would make the wave wait for each load in turn.
template <typename T, int EPV, int U>
__device__ __forceinline__ void load_kv_batches(float *Ks, float *Vs, const T *kp, const T *vp, int n, int cpr, int dhp,
                                                int64_t krs, int64_t vrs, int lane) {
  typedef typename Piece<T, EPV>::type P;
  const unsigned rcp = ((1u << 20) + cpr - 1) / cpr;        // i / cpr == (i * rcp) >> 20 for i < 4096, cpr <= 64
  for (int base = 0; base < n; base += 64 * U) {
    P kv[U], vv[U];
    int at[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * 64 + lane, ii = i < n ? i : n - 1;
      const int j = (int)(((unsigned)ii * rcp) >> 20), c = (ii - j * cpr) * EPV;
      kv[u] = *reinterpret_cast<const P *>(kp + (int64_t)j * krs + c);
      vv[u] = *reinterpret_cast<const P *>(vp + (int64_t)j * vrs + c);
      at[u] = i < n ? j * dhp + c : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (at[u] >= 0) {
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          Ks[at[u] + e] = piece_at<T, EPV>(kv[u], e);
          Vs[at[u] + e] = piece_at<T, EPV>(vv[u], e);
        }
      }
    }
  }
}

// batches of 4 pieces per tile and lane: 8 loads in flight.  (Batches of 8 cost the row kernels 140 registers, i.e. their
// occupancy: BASELINE config 3's layer shape ran 5 ms slower per call with them, profiles/token_query.md.)
template <typename T, int EPV>
__device__ __forceinline__ void load_kv_pieces(float *Ks, float *Vs, const T *kp, const T *vp, int L, int dh, int dhp,
                                               int64_t krs, int64_t vrs, int lane) {
  const int cpr = dh / EPV;
  load_kv_batches<T, EPV, 4>(Ks, Vs, kp, vp, L * cpr, cpr, dhp, krs, vrs, lane);
}

template <typename T>
__device__ __forceinline__ void load_kv(float *Ks, float *Vs, const T *kp, const T *vp, const TokArgs &a, int lane) {
  const int L = a.L, dh = a.dh, dhp = a.dhp;
  const int64_t krs = a.K.row_stride, vrs = a.V.row_stride;
  constexpr int kWide = 16 / (int)sizeof(T);
  if (a.vec == kWide)
    load_kv_pieces<T, kWide>(Ks, Vs, kp, vp, L, dh, dhp, krs, vrs, lane);
  else if (a.vec == kWide / 2)
    load_kv_pieces<T, kWide / 2>(Ks, Vs, kp, vp, L, dh, dhp, krs, vrs, lane);
  else if (kWide / 4 > 1 && a.vec == kWide / 4)
    load_kv_pieces<T, (kWide / 4 > 1 ? kWide / 4 : 1)>(Ks, Vs, kp, vp, L, dh, dhp, krs, vrs, lane);
  else
    load_kv_pieces<T, 1>(Ks, Vs, kp, vp, L, dh, dhp, krs, vrs, lane);
}

// p_j = softmax_j(q . K[j]) of the tile in LDS, lane j (0 for lanes >= L); qs carries 1 / sqrt(dh).  WITH_DP: also
// dp_j = g . V[j] and ds_j = p_j (dp_j - sum p dp), returned in ds.
template <bool WITH_DP>
__device__ __forceinline__ float softmax_lane(const float *qs, const float *gs, const float *Ks, const float *Vs, int L,
                                              int dh, int dhp, int lane, float &ds) {
  float s = -3.0e38f, dp = 0.f;
  if (lane < L) {
    s = 0.f;
    const float *kr = Ks + lane * dhp, *vr = Vs + lane * dhp;
    for (int c = 0; c < dh; ++c) {
      s = fmaf(qs[c], kr[c], s);
      if (WITH_DP) dp = fmaf(gs[c], vr[c], dp);
    }
  }
  const float m = wave_max(s);
  const float e = lane < L ? expf(s - m) : 0.f;
  const float p = e / wave_sum(e);
  if (WITH_DP) ds = p * (dp - wave_sum(p * dp));
  return p;
}

struct Unit {
  int64_t row, out_node;
  int h, beg, end, deg;
};

__device__ __forceinline__ bool unit_of(const TokArgs &a, Unit &u) {
  const int64_t unit = blockIdx.x;
  if (unit >= a.n_units) return false;
  return map_unit(a.hub, a.ptr, unit, a.n_units, a.H, u.row, u.out_node, u.h, u.beg, u.end, u.deg);
}

// the groups' partial sums of one channel, added in a fixed tree; every lane ends with the total
__device__ __forceinline__ float group_sum(float x, int gw) {
  for (int o = gw; o < 64; o <<= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// BWD false: O[d, h] = (1 / deg) sum_edges sum_j p_j V[s, j, h].  BWD true: dQ[d, h] = sum_edges sum_j ds_j K[s, j, h] / sqrt(dh)
// with g = dObar[d, h] / deg.  The hub pass (mode 2) leaves the forward sum unnormalised: the combine applies the mean.
template <typename T, bool BWD>
__global__ __launch_bounds__(AMPCONV_WAVE) void token_row_kernel(TokArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  Unit u;
  if (!unit_of(a, u)) return;
  const int lane = threadIdx.x, L = a.L, dh = a.dh, dhp = a.dhp, tile = L * dhp;
  float *Ks = lds, *Vs = Ks + tile, *qs = Vs + tile, *gs = qs + dhp, *P = gs + dhp;
  const int g = lane >> a.gshift, c = lane & (a.gw - 1), G = 64 >> a.gshift;
  const float inv = u.deg > 0 ? 1.f / (float)u.deg : 0.f;
  if (lane < dh) {
    qs[lane] = a.scale * to_f(tile_ptr<const T>(a.Q, u.row, u.h)[lane]);
    if (BWD) gs[lane] = inv * to_f(tile_ptr<const T>(a.dO, u.row, u.h)[lane]);
  }
  float acc = 0.f;
  for (int p = u.beg; p < u.end; ++p) {
    const int64_t s = a.idx[p];
    __syncthreads();                      // the previous edge's readers are done with the tiles and P
    load_kv<T>(Ks, Vs, tile_ptr<const T>(a.K, s, u.h), tile_ptr<const T>(a.V, s, u.h), a, lane);
    __syncthreads();
    float ds = 0.f;
    const float pj = softmax_lane<BWD>(qs, gs, Ks, Vs, L, dh, dhp, lane, ds);
    P[lane] = BWD ? ds : pj;
    __syncthreads();
    const float *src = BWD ? Ks : Vs;
    if (c < dh)
      for (int j = g; j < L; j += G) acc = fmaf(P[j], src[j * dhp + c], acc);
  }
  acc = group_sum(acc, a.gw);
  const float mul = BWD ? a.scale : (a.hub.mode == 2 ? 1.f : inv);
  if (lane < dh)
    store_out<T>(a.O.ptr, u.out_node * a.O.node_stride + (int64_t)u.h * a.O.head_stride + lane, acc * mul, a.out_f32);
}

// dK[s, j, h] = sum_edges ds_j q_h / sqrt(dh), dV[s, j, h] = sum_edges p_j g over the out-edges of s in CSC order, the
// softmax and sum p.dp recomputed per edge from the destination's q and dObar rows.  NJ: rows per lane, at least
// ceil(L / G).
template <typename T, int NJ>
__global__ __launch_bounds__(AMPCONV_WAVE) void token_src_kernel(TokArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  Unit u;
  if (!unit_of(a, u)) return;
  const int lane = threadIdx.x, L = a.L, dh = a.dh, dhp = a.dhp, tile = L * dhp;
  float *Ks = lds, *Vs = Ks + tile, *qs = Vs + tile, *gs = qs + dhp, *P = gs + dhp, *dS = P + 64;
  const int g = lane >> a.gshift, c = lane & (a.gw - 1), G = 64 >> a.gshift;
  const int nj = (L + G - 1) / G;
  const bool on = c < dh;
  if (u.end > u.beg)                      // (a source without out-edges: zeros, its rows of K and V are not read)
    load_kv<T>(Ks, Vs, tile_ptr<const T>(a.K, u.row, u.h), tile_ptr<const T>(a.V, u.row, u.h), a, lane);
  float dk[NJ], dv[NJ];
#pragma unroll
  for (int k = 0; k < NJ; ++k) dk[k] = dv[k] = 0.f;
  // the rows of edge p + 1 and the indices of edge p + 2 are loaded while edge p is computed (lanes of padding channels
  // read channel 0: every lane loads a valid address)
  const int cl = on ? c : 0, last = u.end - 1;
  int64_t d1 = 0;
  float inv1 = 0.f;
  T qn = (T)0.f, gn = (T)0.f;
  if (u.beg < u.end) {
    const int64_t d0 = a.idx[u.beg];
    inv1 = a.cinv[u.beg];
    qn = tile_ptr<const T>(a.Q, d0, u.h)[cl];
    gn = tile_ptr<const T>(a.dO, d0, u.h)[cl];
    d1 = a.idx[u.beg < last ? u.beg + 1 : last];
  }
  for (int p = u.beg; p < u.end; ++p) {
    const float qc = on ? a.scale * to_f(qn) : 0.f, gc = on ? inv1 * to_f(gn) : 0.f;
    const int p1 = p < last ? p + 1 : last, p2 = p + 2 < u.end ? p + 2 : last;
    inv1 = a.cinv[p1];
    qn = tile_ptr<const T>(a.Q, d1, u.h)[cl];
    gn = tile_ptr<const T>(a.dO, d1, u.h)[cl];
    d1 = a.idx[p2];
    __syncthreads();                      // the previous edge's readers are done with qs, gs, P, dS (first edge: the tiles are in)
    if (lane < dh) {
      qs[lane] = qc;
      gs[lane] = gc;
    }
    __syncthreads();
    float ds = 0.f;
    const float pj = softmax_lane<true>(qs, gs, Ks, Vs, L, dh, dhp, lane, ds);
    P[lane] = pj;
    dS[lane] = ds;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NJ; ++k) {
      if (k < nj) {                       // (the same in every lane)
        const int j = g + G * k;
        const float w = j < L ? dS[j] : 0.f, pv = j < L ? P[j] : 0.f;
        dk[k] = fmaf(w, qc, dk[k]);
        dv[k] = fmaf(pv, gc, dv[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NJ; ++k) {
    const int j = g + G * k;
    if (on && k < nj && j < L) {
      const int64_t hc = (int64_t)u.h * a.O.head_stride + c, hc2 = (int64_t)u.h * a.O2.head_stride + c;
      store_out<T>(a.O.ptr, u.out_node * a.O.node_stride + (int64_t)j * a.O.row_stride + hc, dk[k], a.out_f32);
      store_out<T>(a.O2.ptr, u.out_node * a.O2.node_stride + (int64_t)j * a.O2.row_stride + hc2, dv[k], a.out_f32);
    }
  }
}

constexpr int kMaxL = 64, kMaxDh = 64;
constexpr size_t kLdsOptIn = 48 * 1024;

bool shape_ok(int L, int D, int H, int dtype) {
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return false;
  if (L <= 0 || D <= 0 || H <= 0 || D % H != 0) return false;
  const int dh = D / H;
  if (L > kMaxL || dh > kMaxDh) return false;
  return dtype == AMPCONV_F32 || dh % 2 == 0;       // bf16 rows move in pieces of at least two elements
}

size_t lds_bytes(int L, int dhp) { return ((size_t)2 * L * dhp + 2 * dhp + 2 * 64) * sizeof(float); }

// elements per K / V load piece: the widest of 16, 8, 4 (and, bf16, 2) bytes that divides a head's slice, both bases
// and every stride of K and V
int piece_elems(const ampconv_view_t &K, const ampconv_view_t &V, int dh, int esize) {
  for (int bytes = 16; bytes > esize; bytes /= 2) {
    bool ok = (int64_t)dh * esize % bytes == 0;
    for (const ampconv_view_t *v : {&K, &V})
      ok = ok && (uintptr_t)v->ptr % bytes == 0 && v->node_stride * esize % bytes == 0 &&
           v->row_stride * esize % bytes == 0 && v->head_stride * esize % bytes == 0;
    if (ok) return bytes / esize;
  }
  return 1;
}

void fill_common(TokArgs &a, int L, int D, int H, int dtype, HubArgs hub, int64_t n, bool bf) {
  a.hub = hub;
  a.n_units = n * H;
  a.L = L;
  a.dh = D / H;
  a.dhp = a.dh | 1;
  a.H = H;
  a.gw = 1;
  a.gshift = 0;
  while (a.gw < a.dh) a.gw <<= 1, ++a.gshift;
  a.vec = piece_elems(a.K, a.V, a.dh, bf ? 2 : 4);
  a.out_f32 = !bf || hub.mode == 2;
  a.scale = 1.f / sqrtf((float)a.dh);
  (void)dtype;
}

template <typename Kern>
int launch_token(Kern kernel, const TokArgs &a, hipStream_t stream) {
  if (a.n_units > INT32_MAX) return AMPCONV_E_BADARG;
  const size_t lds = lds_bytes(a.L, a.dhp);
  if (lds > kLdsOptIn) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  kernel<<<dim3((unsigned)a.n_units), dim3(AMPCONV_WAVE), lds, stream>>>(a);
  return ampconv_launch_status();
}

template <typename T>
int launch_src(const TokArgs &a, hipStream_t stream) {
  const int nj = (a.L + (64 >> a.gshift) - 1) / (64 >> a.gshift);
  if (nj <= 8) return launch_token(token_src_kernel<T, 8>, a, stream);
  if (nj <= 16) return launch_token(token_src_kernel<T, 16>, a, stream);
  if (nj <= 24) return launch_token(token_src_kernel<T, 24>, a, stream);
  if (nj <= 40) return launch_token(token_src_kernel<T, 40>, a, stream);
  return launch_token(token_src_kernel<T, 64>, a, stream);
}

// the checks the three entry points share; AMPCONV_OK: go on
int check_token(int L, int D, int H, int dtype, int64_t n, const void *ptr, const void *hub_plan, int64_t hub_chunks,
                const void *hub_ws, std::initializer_list<const ampconv_view_t *> views) {
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  if (L <= 0 || D <= 0 || H <= 0 || D % H != 0 || n < 0 || hub_chunks < 0) return AMPCONV_E_BADARG;
  if (!shape_ok(L, D, H, dtype)) return dtype == AMPCONV_BF16 && L <= kMaxL && D / H <= kMaxDh ? AMPCONV_E_DTYPE : AMPCONV_E_BADARG;
  if (hub_ws && !hub_plan) return AMPCONV_E_BADARG;
  if (hub_plan && hub_chunks > 0 && !hub_ws) return AMPCONV_E_BADARG;
  if (n == 0) return AMPCONV_OK;
  if (!ptr) return AMPCONV_E_BADARG;
  for (const ampconv_view_t *v : views)
    if (!view_ok(*v)) return AMPCONV_E_BADARG;
  return AMPCONV_OK;
}

}  // namespace

extern "C" int ampconv_token_supported(int L, int D, int H, int dtype) { return shape_ok(L, D, H, dtype) ? 1 : 0; }

extern "C" int ampconv_fwd_edge_token(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, const int32_t *rowptr,
                                      const int32_t *col, int64_t n_rows, int L, int D, int H, ampconv_view_t O,
                                      const void *hub_plan, int64_t hub_chunks, void *hub_ws, int dtype, void *stream) {
  if (int rc = check_token(L, D, H, dtype, n_rows, rowptr, hub_plan, hub_chunks, hub_ws, {&Q, &K, &V, &O})) return rc;
  if (n_rows == 0) return AMPCONV_OK;
  const bool bf = dtype == AMPCONV_BF16;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *) {
    TokArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.dO = Q; a.O = o[0]; a.O2 = o[0];
    a.ptr = rowptr; a.idx = col;
    fill_common(a, L, D, H, dtype, hub, n, bf);
    return bf ? launch_token(token_row_kernel<__bf16, false>, a, st) : launch_token(token_row_kernel<float, false>, a, st);
  };
  // (partial tiles and the combine see the output as ONE token of D channels)
  return run_edge_pass(run, n_rows, {O}, hub_plan, hub_chunks, hub_ws, 1, D, H, rowptr, {1.f}, bf, nullptr, st);
}

extern "C" int ampconv_bwd_edge_dst_token(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                                          const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D, int H,
                                          ampconv_view_t dQ, const void *hub_plan, int64_t hub_chunks, void *hub_ws,
                                          int dtype, void *stream) {
  if (int rc = check_token(L, D, H, dtype, n_rows, rowptr, hub_plan, hub_chunks, hub_ws, {&Q, &K, &V, &dObar, &dQ}))
    return rc;
  if (n_rows == 0) return AMPCONV_OK;
  const bool bf = dtype == AMPCONV_BF16;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *) {
    TokArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.dO = dObar; a.O = o[0]; a.O2 = o[0];
    a.ptr = rowptr; a.idx = col;
    fill_common(a, L, D, H, dtype, hub, n, bf);
    return bf ? launch_token(token_row_kernel<__bf16, true>, a, st) : launch_token(token_row_kernel<float, true>, a, st);
  };
  // (the partial tiles carry 1 / in-degree and 1 / sqrt(dh) already)
  return run_edge_pass(run, n_rows, {dQ}, hub_plan, hub_chunks, hub_ws, 1, D, H, nullptr, {1.f}, bf, nullptr, st);
}

extern "C" int ampconv_bwd_edge_src_token(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                                          const int32_t *cscptr, const int32_t *crow, const float *cinv, int64_t n_src,
                                          int L, int D, int H, ampconv_view_t dK, ampconv_view_t dV, const void *hub_plan,
                                          int64_t hub_chunks, void *hub_ws, int dtype, void *stream) {
  if (int rc = check_token(L, D, H, dtype, n_src, cscptr, hub_plan, hub_chunks, hub_ws, {&Q, &K, &V, &dObar, &dK, &dV}))
    return rc;
  if (n_src == 0) return AMPCONV_OK;
  if (!cinv) return AMPCONV_E_BADARG;
  const bool bf = dtype == AMPCONV_BF16;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *) {
    TokArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.dO = dObar; a.O = o[0]; a.O2 = o[1];
    a.ptr = cscptr; a.idx = crow; a.cinv = cinv;
    fill_common(a, L, D, H, dtype, hub, n, bf);
    return bf ? launch_src<__bf16>(a, st) : launch_src<float>(a, st);
  };
  return run_edge_pass(run, n_src, {dK, dV}, hub_plan, hub_chunks, hub_ws, L, D, H, nullptr, {1.f, 1.f}, bf, nullptr, st);
}
