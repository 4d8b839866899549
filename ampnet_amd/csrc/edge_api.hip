// C-ABI entry points of the edge phase: argument checks, the choice of a kernel family (edge_family) and one
// run_edge_pass (common.h) of that family.  AMPCONV_FORCE_GENERIC=1 in the environment pins the generic kernels for
// fp32 storage (used by the tests to cross-check the families).
#include <cstdlib>
#include "common.h"

namespace {
bool force_generic() { return env_switch("AMPCONV_FORCE_GENERIC", false); }      // re-read on every call: tests flip it
// short token sequences (L <= 4) have a family of their own (edge_small.hip); AMPCONV_SMALL=0 sends them to the tile
// kernels instead (the tests cross-check the two)
bool small_off() { return !env_switch("AMPCONV_SMALL", true); }      // re-read on every call, like AMPCONV_FORCE_GENERIC
int check_common(int L, int D, int H, int dtype) {
  if (dtype != AMPCONV_F32 && dtype != AMPCONV_BF16) return AMPCONV_E_DTYPE;
  if (L <= 0 || D <= 0 || H <= 0 || D % H != 0) return AMPCONV_E_BADARG;
  return AMPCONV_OK;
}

enum Pass { kFwd = AMPCONV_PASS_FWD, kDst = AMPCONV_PASS_DST, kSrc = AMPCONV_PASS_SRC };
enum Family {       // (the codes ampconv_edge_family reports)
  kBf16 = AMPCONV_FAMILY_BF16_MFMA,
  kSmall = AMPCONV_FAMILY_SMALL,
  kMfma = AMPCONV_FAMILY_MFMA,
  kBlock = AMPCONV_FAMILY_BLOCK,
  kGeneric = AMPCONV_FAMILY_GENERIC
};

// The kernel family of one edge pass, or a negative AMPCONV_E_* code.  `stats`: the softmax statistics hand-off is in
// use (written by the destination pass, read by the source pass) -- only the edge_mfma and workgroup-per-unit families
// keep statistics, each in its own layout, and a buffer sized for one must not reach the other.  views == nullptr,
// n = 0: the shape alone (ampconv_softmax_stats_bytes).
int edge_family(Pass pass, int dtype, int L, int D, int H, bool stats, const ampconv_view_t *views, int n) {
  const bool bf = dtype == AMPCONV_BF16, fp = !bf && !force_generic();
  if (stats && views) {
    // a buffer can only have been sized by ampconv_softmax_stats_bytes, i.e. for the family of the shape alone: where
    // that keeps none, `stats` must be NULL (a family that does keep them would write past whatever was passed)
    const int sized_for = edge_family(kDst, dtype, L, D, H, false, nullptr, 0);
    if (sized_for != kMfma && sized_for != kBlock) return sized_for < 0 ? sized_for : AMPCONV_E_BADARG;
  }
  if (bf && ampconv_bf16_supported(L, D, H, views, n)) return stats ? AMPCONV_E_BADARG : kBf16;
  // bf16 storage of the other shapes: the workgroup-per-unit kernels widen / round the rows themselves (their source
  // pass exists only with the statistics)
  const bool block = (bf || fp) && (stats || pass != kSrc) && ampconv_block_supported(L, D, H, views, n, bf);
  if (bf && !block) return AMPCONV_E_DTYPE;
  if (fp && !stats && !small_off() && ampconv_small_supported(L, D, H, views, n)) return kSmall;
  if (fp && ampconv_mfma_supported(L, D, H) && ampconv_mfma_views_ok(views, n)) return kMfma;
  // (fp32 statistics of the edge_mfma shapes are in edge_mfma's layout)
  if (block && (bf || !stats || !ampconv_mfma_supported(L, D, H))) return kBlock;
  if (bf) return AMPCONV_E_DTYPE;
  if (stats) return AMPCONV_E_BADARG;     // the generic kernels keep no statistics
  return kGeneric;
}

// out_absmax of the backward passes: edge_mfma's destination kernels record it as they write; for every other
// (family, pass) the entry point measures what was written (view_absmax)
bool records_absmax(int family, Pass pass) { return family == kMfma && pass == kDst; }

}  // namespace

extern "C" int ampconv_version(void) { return AMPCONV_VERSION; }

extern "C" const char *ampconv_error_string(int code) {
  switch (code) {
    case AMPCONV_OK: return "ok";
    case AMPCONV_E_BADARG: return "ampconv: bad argument";
    case AMPCONV_E_DTYPE: return "ampconv: dtype not supported";
    case AMPCONV_E_WORKSPACE: return "ampconv: workspace too small";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "ampconv: unknown error";
  }
}

extern "C" int ampconv_fwd_edge(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                const int32_t *rowptr, const int32_t *col, const int32_t *qidx,
                                int64_t n_rows, int L, int D, int H, ampconv_view_t O,
                                const void *hub_plan, int64_t hub_chunks, void *hub_ws, int dtype,
                                void *stream) {
  if (int rc = check_common(L, D, H, dtype)) return rc;
  if (n_rows < 0) return AMPCONV_E_BADARG;
  if (n_rows == 0) return AMPCONV_OK;
  if (!view_ok(Q) || !view_ok(K) || !view_ok(V) || !view_ok(O) || !rowptr) return AMPCONV_E_BADARG;
  const ampconv_view_t views[] = {Q, K, V, O};
  const int f = edge_family(kFwd, dtype, L, D, H, false, views, 4);
  if (f < 0) return f;
  const bool bf = dtype == AMPCONV_BF16;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *) {
    switch (f) {
      case kBf16: return ampconv_fwd_edge_bf16(Q, K, V, rowptr, col, qidx, n, L, D, H, o[0], hub, st);
      case kSmall: return ampconv_fwd_edge_small(Q, K, V, rowptr, col, qidx, n, L, D, H, o[0], hub, st);
      case kMfma: return ampconv_fwd_edge_mfma(Q, K, V, rowptr, col, qidx, n, L, D, H, o[0], hub, st);
      case kBlock: return ampconv_fwd_edge_block(Q, K, V, rowptr, col, qidx, n, L, D, H, o[0], hub, bf, st);
      default: return ampconv_fwd_edge_generic(Q, K, V, rowptr, col, qidx, n, L, D, H, o[0], st);
    }
  };
  // (no long-segment passes for a query subset or on the generic kernels)
  const void *plan = qidx || f == kGeneric ? nullptr : hub_plan;
  return run_edge_pass(run, n_rows, {O}, plan, hub_chunks, hub_ws, L, D, H, rowptr, {1.f}, bf, nullptr, st);
}

extern "C" size_t ampconv_softmax_stats_bytes(int64_t E, int L, int D, int H, int dtype) {
  // bf16 storage keeps none on the bf16 MFMA shapes: there the passes are HBM-bound and the extra 2 x 160 B per edge and
  // head cost the destination pass what they save the source pass (measured: +0.54 / -0.53 ms)
  if (E <= 0 || check_common(L, D, H, dtype) != AMPCONV_OK) return 0;
  switch (edge_family(kDst, dtype, L, D, H, false, nullptr, 0)) {      // (the same family with the buffer)
    case kMfma: return (size_t)E * H * kStatsPerUnit * sizeof(float);
    case kBlock: return (size_t)E * H * ampconv_block_stats_floats(L) * sizeof(float);
    default: return 0;
  }
}

// ampconv_absmax (proj_gemm.hip)
extern "C" int ampconv_absmax(const void *X, int64_t ld, int64_t M, int K, int dtype, float *out, int reset, void *stream);

namespace {
// out_absmax of the backward passes for the kernel families that do not record it themselves: one ampconv_absmax pass
// over what was just written, which must then be a row-major matrix that pass can walk in 16-byte pieces (token rows of
// D contiguous channels, nodes L rows apart, base, D and row stride whole pieces).  The entry points ask BEFORE they
// launch the pass: an error code means that nothing was written.
bool absmax_view_ok(const ampconv_view_t &v, int L, int D, int H) {
  return v.head_stride == D / H && v.node_stride == (int64_t)L * v.row_stride && v.row_stride >= D && D % 4 == 0 &&
         v.row_stride % 4 == 0 && (uintptr_t)v.ptr % 16 == 0;
}
int view_absmax(const ampconv_view_t &v, int64_t n, int L, int D, int H, float *out, void *stream) {
  if (!absmax_view_ok(v, L, D, H)) return AMPCONV_E_BADARG;
  return ampconv_absmax(v.ptr, v.row_stride, n * L, D, AMPCONV_F32, out, 0, stream);
}
}  // namespace

extern "C" int ampconv_edge_family(int pass, int dtype, int L, int D, int H, int stats, const ampconv_view_t *views,
                                   int n) {
  if (pass != AMPCONV_PASS_FWD && pass != AMPCONV_PASS_DST && pass != AMPCONV_PASS_SRC) return AMPCONV_E_BADARG;
  if (int rc = check_common(L, D, H, dtype)) return rc;
  if (n < 0 || (n > 0 && !views) || (stats && pass == AMPCONV_PASS_FWD)) return AMPCONV_E_BADARG;
  for (int i = 0; i < n; ++i)
    if (!view_ok(views[i])) return AMPCONV_E_BADARG;
  return edge_family((Pass)pass, dtype, L, D, H, stats != 0, views, n);
}

extern "C" int ampconv_bwd_edge_dst(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                    ampconv_view_t dObar, const int32_t *rowptr,
                                    const int32_t *col, int64_t n_rows, int L, int D, int H,
                                    ampconv_view_t dQ, const void *hub_plan, int64_t hub_chunks,
                                    void *hub_ws, const int32_t *spos, float *stats, float *out_absmax,
                                    int dtype, void *stream) {
  if (out_absmax && dtype != AMPCONV_F32) return AMPCONV_E_DTYPE;       // operand maxima: fp32 storage (scaled projections)
  if (int rc = check_common(L, D, H, dtype)) return rc;
  if (stats && (!spos || (uintptr_t)stats % 16 != 0)) return AMPCONV_E_BADARG;
  if (n_rows < 0) return AMPCONV_E_BADARG;
  if (n_rows == 0) return AMPCONV_OK;
  if (!view_ok(Q) || !view_ok(K) || !view_ok(V) || !view_ok(dObar) || !view_ok(dQ) || !rowptr)
    return AMPCONV_E_BADARG;
  const ampconv_view_t views[] = {Q, K, V, dObar, dQ};
  const int f = edge_family(kDst, dtype, L, D, H, stats, views, 5);
  if (f < 0) return f;
  const bool bf = dtype == AMPCONV_BF16, recorded = records_absmax(f, kDst);
  if (out_absmax && !recorded && !absmax_view_ok(dQ, L, D, H)) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *absmax) {
    const StatsArgs sa{spos, stats, absmax};
    switch (f) {
      case kBf16: return ampconv_bwd_edge_dst_bf16(Q, K, V, dObar, rowptr, col, n, L, D, H, o[0], hub, st);
      case kSmall: return ampconv_bwd_edge_dst_small(Q, K, V, dObar, rowptr, col, n, L, D, H, o[0], hub, st);
      case kMfma: return ampconv_bwd_edge_dst_mfma(Q, K, V, dObar, rowptr, col, n, L, D, H, o[0], hub, sa, st);
      case kBlock: return ampconv_bwd_edge_dst_block(Q, K, V, dObar, rowptr, col, n, L, D, H, o[0], hub, sa, bf, st);
      default: return ampconv_bwd_edge_dst_generic(Q, K, V, dObar, rowptr, col, n, L, D, H, o[0], st);
    }
  };
  if (int rc = run_edge_pass(run, n_rows, {dQ}, f == kGeneric ? nullptr : hub_plan, hub_chunks, hub_ws, L, D, H,
                             nullptr, {1.f / sqrtf((float)(D / H))}, bf, recorded ? out_absmax : nullptr, st))
    return rc;
  return out_absmax && !recorded ? view_absmax(dQ, n_rows, L, D, H, out_absmax, stream) : AMPCONV_OK;
}

extern "C" int ampconv_bwd_edge_src(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                    ampconv_view_t dObar, const int32_t *cscptr,
                                    const int32_t *crow, const float *cinv, int64_t n_src,
                                    int L, int D, int H, ampconv_view_t dK, ampconv_view_t dV,
                                    const void *hub_plan, int64_t hub_chunks, void *hub_ws,
                                    const float *stats, float *out_absmax, int dtype, void *stream) {
  if (out_absmax && dtype != AMPCONV_F32) return AMPCONV_E_DTYPE;
  if (int rc = check_common(L, D, H, dtype)) return rc;
  if (stats && (uintptr_t)stats % 16 != 0) return AMPCONV_E_BADARG;
  if (n_src < 0) return AMPCONV_E_BADARG;
  if (n_src == 0) return AMPCONV_OK;
  if (!view_ok(Q) || !view_ok(K) || !view_ok(V) || !view_ok(dObar) || !view_ok(dK) ||
      !view_ok(dV) || !cscptr || !cinv)
    return AMPCONV_E_BADARG;
  const ampconv_view_t views[] = {Q, K, V, dObar, dK, dV};
  const int f = edge_family(kSrc, dtype, L, D, H, stats, views, 6);
  if (f < 0) return f;
  const bool bf = dtype == AMPCONV_BF16, recorded = records_absmax(f, kSrc);
  if (out_absmax && !recorded && !(absmax_view_ok(dK, L, D, H) && absmax_view_ok(dV, L, D, H))) return AMPCONV_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](int64_t n, HubArgs hub, const ampconv_view_t *o, float *absmax) {
    const StatsArgs sa{nullptr, const_cast<float *>(stats), absmax};
    switch (f) {
      case kBf16:
        return ampconv_bwd_edge_src_bf16(Q, K, V, dObar, cscptr, crow, cinv, n, L, D, H, o[0], o[1], hub, st);
      case kSmall:
        return ampconv_bwd_edge_src_small(Q, K, V, dObar, cscptr, crow, cinv, n, L, D, H, o[0], o[1], hub, st);
      case kMfma:
        return ampconv_bwd_edge_src_mfma(Q, K, V, dObar, cscptr, crow, cinv, n, L, D, H, o[0], o[1], hub, sa, st);
      case kBlock:
        return ampconv_bwd_edge_src_block(Q, K, V, dObar, cscptr, crow, cinv, n, L, D, H, o[0], o[1], hub, stats, bf,
                                          st);
      default: return ampconv_bwd_edge_src_generic(Q, K, V, dObar, cscptr, crow, cinv, n, L, D, H, o[0], o[1], st);
    }
  };
  // partial dK tiles: the bf16 MFMA kernels leave 1 / sqrt(dh) to the combine; the others carry log2e / sqrt(dh) in Q
  // and leave ln 2 (bf16 workgroup-per-unit tiles included: store_xb compensates, edge_block_x3.hip)
  const float dk_scale = f == kBf16 ? 1.f / sqrtf((float)(D / H)) : 0.6931471805599453f;
  if (int rc = run_edge_pass(run, n_src, {dK, dV}, f == kGeneric ? nullptr : hub_plan, hub_chunks, hub_ws, L, D, H,
                             nullptr, {dk_scale, 1.f}, bf, recorded ? out_absmax : nullptr, st))
    return rc;
  if (!out_absmax || recorded) return AMPCONV_OK;
  if (int rc = view_absmax(dK, n_src, L, D, H, out_absmax, stream)) return rc;
  return view_absmax(dV, n_src, L, D, H, out_absmax, stream);
}
