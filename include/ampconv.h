/*
 * ampconv.h -- C ABI of libampconv.so: the MI355X (gfx950) implementation of the
 * AMPConv hot path of HarryL-Git/ampnet.
 *
 * The reference has no FFI layer of its own: its boundary for this path is the
 * Python class `AMPConv` (reference src/ampnet/conv/amp_conv.py:9-51) on top of
 * torch.nn.MultiheadAttention and torch_geometric.nn.MessagePassing.  Each entry
 * point below names the reference lines whose arithmetic it replaces.  The host
 * side that binds these with ctypes is ampnet_amd/conv/amp_conv.py; the stub a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; the library
 *     allocates nothing and keeps no state between calls (re-entrant);
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     no call synchronises the device;
 *   - every function returns 0 on success, a negative AMPCONV_E_* code for
 *     argument errors detected on the host, or a positive hipError_t;
 *     nothing throws or aborts;
 *   - N = nodes, E = edges, L = tokens per node, D = embed_dim, H = heads,
 *     dh = D / H.  Messages flow src = edge_index[0] -> dst = edge_index[1]
 *     (amp_conv.py:40-41).
 */
#ifndef AMPCONV_H_
#define AMPCONV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMPCONV_VERSION 111

enum {
  AMPCONV_OK = 0,
  AMPCONV_E_BADARG = -1,   /* null pointer, negative size, D % H != 0, ... */
  AMPCONV_E_DTYPE = -2,    /* dtype not supported by this build */
  AMPCONV_E_WORKSPACE = -3 /* workspace too small */
};

/* dtype codes.
 * AMPCONV_F32:  every view is fp32 in HBM; the per-edge products of the one-wave-per-unit shapes (L <= 20, dh = 32 or 16)
 *               run on v_mfma_f32_16x16x4_f32 (exact fp32, fmaf-chain numerics), those of the workgroup-per-unit shapes
 *               (other even dh <= 64, L <= 64) on the 16-bit matrix cores with every fp32 tile split exactly into three
 *               bf16 planes on its way into LDS (fp32-grade error; csrc/edge_block_x3.hip), the per-node projections
 *               (ampconv_proj_*) the same way.
 * AMPCONV_BF16: every view is bf16 in HBM (Q/K/V/O and gradients), fp32 softmax and accumulation.
 *               L <= 20 with dh = 32 (BASELINE config 5) or dh = 16 (half-filled tiles): products on the bf16 MFMA,
 *               no softmax statistics.  Other even dh <= 64 with L <= 64 (e.g. the reference's class default L = 40,
 *               dh = 50): the workgroup-per-unit kernels on the bf16 rows as they lie (one bf16 MFMA per product,
 *               softmax weights and dS rounded to bf16 for their second product); their source pass needs the
 *               statistics buffer of ampconv_softmax_stats_bytes like the fp32 call.  Anything else: AMPCONV_E_DTYPE.
 * (Versions <= 102 had three more codes for split-operand edge kernels; they were slower than the native fp32 MFMA
 * kernels on MI355X and were removed in 103.) */
enum { AMPCONV_F32 = 0, AMPCONV_BF16 = 1 };

/*
 * Strided view of a per-node token matrix: element (node n, token l, head h,
 * channel c) lives at  ptr + n*node_stride + l*row_stride + h*head_stride + c
 * (strides in ELEMENTS).  A row-major [N, L, D] tensor is
 * {ptr, L*D, D, dh}; the K third of a packed [N*L, 3D] projection is
 * {ptr + D, L*3*D, 3*D, dh}.
 */
typedef struct {
  void *ptr;
  int64_t node_stride;
  int64_t row_stride;
  int64_t head_stride;
} ampconv_view_t;

int ampconv_version(void);
const char *ampconv_error_string(int code);

/* ---- graph preparation ------------------------------------------------------
 * Replaces what PyG's propagate() does implicitly with index_select/scatter on
 * the unsorted edge list (amp_conv.py:25).  Builds, with stable sorts so that
 * every later floating-point sum has a fixed order:
 *   dst-sorted CSR: rowptr[N+1], col[E] (source of each sorted edge),
 *                   eperm[E] (original edge id at each sorted position)
 *   src-sorted CSC: cscptr[N+1], crow[E] (destination), cperm[E],
 *                   cinv[E] = 1 / in-degree(crow[p]) (the weight of edge p in its
 *                   destination's mean, read sequentially by the source pass)
 * `oob` (device int32) is set non-zero if any index is outside [0, N); such
 * indices are clamped on their int64 value -- v < 0 -> 0, v >= N -> N - 1 -- and every
 * array then describes the CLAMPED graph: col and crow lie in [0, N), eperm and cperm are
 * permutations of the edge ids, both pointers end at E, so that no kernel that walks them
 * faults.  E = 0 writes the flag (0) and both pointer arrays (all zero) and nothing else.
 * A refused call (AMPCONV_E_BADARG, AMPCONV_E_WORKSPACE) has launched and written nothing.  */
size_t ampconv_csr_workspace_bytes(int64_t N, int64_t E);
int ampconv_csr_build(const int64_t *edge_index, int64_t E, int64_t N,
                      int32_t *rowptr, int32_t *col, int32_t *eperm,
                      int32_t *cscptr, int32_t *crow, int32_t *cperm, float *cinv,
                      int32_t *oob, void *workspace, size_t workspace_bytes,
                      void *stream);

/* csr_build and both long-segment plans (below; chunk <= 0 or a NULL plan: none) in one call.  Graphs of at most
 * 12 288 edges and 16 384 nodes -- GraphSAINT batches, Cora: the reference's own regime -- are prepared by ONE launch
 * (two workgroups, the stable sorts in LDS); larger ones by the calls above.  Same outputs either way.
 * `status` (device int32[4]) = {bounds flag as `oob` above, chunks of plan_dst, chunks of plan_src, 0}: everything the
 * host needs back, in one 16-byte read.  `by_edge` (E int32, may be NULL): CSC position of every ORIGINAL edge id,
 * from which ampconv_csc_positions_from derives `spos` (below) in one launch.  `cinv` may be NULL too.  E = 0 writes
 * the four status words (0) and both pointer arrays (all zero) and nothing else; a refused call has written nothing,
 * the status words included.  */
int ampconv_graph_build(const int64_t *edge_index, int64_t E, int64_t N,
                        int32_t *rowptr, int32_t *col, int32_t *eperm,
                        int32_t *cscptr, int32_t *crow, int32_t *cperm, float *cinv,
                        int32_t *status, int chunk, void *plan_dst, void *plan_src,
                        int32_t *by_edge, void *workspace, size_t workspace_bytes, void *stream);
int ampconv_csc_positions_from(const int32_t *eperm, const int32_t *by_edge, int64_t E,
                               int32_t *spos, void *stream);

/* spos[p] = position in the src-sorted CSC of the edge at position p of the dst-sorted CSR
 * (eperm, cperm of ampconv_csr_build; `scratch` = E int32).  Needed only to hand softmax
 * statistics from the destination pass to the source pass (below).  */
int ampconv_csc_positions(const int32_t *eperm, const int32_t *cperm, int64_t E,
                          int32_t *scratch, int32_t *spos, void *stream);

/* Node lists for the projections' `nodes` argument (below): the ascending ids of the nodes with at least one in-edge
 * (which = 1), one out-edge (2) or either (3).  list: N + 8 int32 (the entries behind the count are padding the
 * projection kernels may read); ptr: N + 1 int32, ptr[n + 1] - ptr[n] = 1 iff node n is listed, ptr[N] = the count
 * -- a CSR-shaped array, so ampconv_mask_rows(Y, ptr, ...) zeroes exactly the rows of the nodes NOT listed;
 * count: one device int32.  */
size_t ampconv_active_nodes_workspace_bytes(int64_t N);
int ampconv_active_nodes(const int32_t *rowptr, const int32_t *cscptr, int64_t N, int which,
                         int32_t *list, int32_t *ptr, int32_t *count, void *workspace,
                         size_t workspace_bytes, void *stream);

/* ---- long segments ("hubs": power-law graphs, BASELINE config 5) ---------------------------
 * One wavefront per (row, head) runs as long as its longest segment.  A plan cuts every CSR
 * (or CSC) segment longer than `chunk` edges into chunks; the edge kernels then reduce each
 * chunk in its own wavefront into a partial tile in `hub_ws` and an ordered pass adds a row's
 * partial tiles (fixed order: bitwise reproducible).  plan = int32 header {n_chunks, chunk,
 * n_long = long rows, offset of the row list in int32 units}, then max_chunks = 2 * (E / chunk) + 2 slots of
 * 16-byte descriptors {row, begin, end, nfirst} (the first n_chunks in use; nfirst = the row's
 * chunk count in its first chunk, 0 in the others), then, at the offset 4 + 4 * max_chunks, the
 * list of the slots of the long rows' first chunks (max_chunks / 2 + 2 entries, the first n_long
 * in use), which the ordered pass launches over.  A row's chunks occupy CONSECUTIVE slots from
 * its first, in order k = 0, 1, ...: the partial tile of chunk k of the row whose first slot is c
 * is tile c + k of hub_ws.  Which row takes which slots, and the order of the list, are
 * arbitrary; no result depends on them.  ampconv_hub_plan_bytes covers all of it (header,
 * max_chunks slots, list; 0 for chunk <= 0), and nothing behind the slots and list entries in use
 * is written.  The caller reads header[0] back once (n_chunks), sizes
 * hub_ws with ampconv_hub_workspace_bytes and passes both to the edge calls (plan = NULL or
 * n_chunks = 0: no splitting).  n_tiles = 1 (forward, dst pass) or 2 (src pass: dK and dV).
 * A plan passed to an edge call must have been built over EXACTLY the rows the call covers --
 * ampconv_hub_plan(ptr, n_rows, ...) for a call with that n_rows (n_src), over the same ptr: the passes write the output
 * row of every long row the plan names, whatever their own row count is, so a plan over more rows overwrites rows behind
 * n_rows, and one over fewer leaves long rows unwritten.  (The row count of a plan lives in device memory only; the
 * entry points cannot check it without a read-back and do not.)  */
size_t ampconv_hub_plan_bytes(int64_t E, int chunk);
int ampconv_hub_plan(const int32_t *ptr, int64_t N, int64_t E, int chunk, void *plan, void *stream);
size_t ampconv_hub_workspace_bytes(int64_t n_chunks, int L, int D, int n_tiles);

/* ---- edge phase, forward ----------------------------------------------------
 * For every row r < n_rows (destination d = qidx ? qidx[r] : r) and head h:
 *   O[r,:,h] = (1/deg_r) * sum_{p in [rowptr[r], rowptr[r+1])}
 *                 softmax_rows(Q[d,:,h] K[col[p],:,h]^T / sqrt(dh)) V[col[p],:,h]
 * and O[r] = 0 when deg_r = 0.  Replaces, per edge: torch functional.py:6578
 * (scale), :6589 (QK^T), :6590 (softmax), :6594 (PV), and PyG's mean
 * aggregation (amp_conv.py:11).  Q/K/V are the per-NODE projections.  */
int ampconv_fwd_edge(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                     const int32_t *rowptr, const int32_t *col,
                     const int32_t *qidx, int64_t n_rows, int L, int D, int H,
                     ampconv_view_t O, const void *hub_plan, int64_t hub_chunks,
                     void *hub_ws, int dtype, void *stream);

/* ---- edge phase, backward (autograd of the above; amp_conv.py has no custom
 * backward, cora_benchmark_graphsaint.py:110 calls loss.backward()) ------------
 * dObar is the gradient w.r.t. the MEAN (the kernels apply 1/deg).
 * _dst: one pass over the dst-sorted CSR, writes dQ[r] for every row.
 * _src: one pass over the src-sorted CSC, writes dK[s], dV[s] for every source;
 *       `cinv[p]` = 1/in-degree of the destination of CSC edge p (ampconv_csr_build).
 * No atomics: every output row is owned by one wavefront.
 * Softmax statistics (optional): both passes need, per edge, head and destination token i, the
 * softmax normaliser and delta_i = sum_j P_ij dP_ij.  The destination pass has them as a by-product
 * (its softmax runs inside a lane); the source pass otherwise re-reduces them across lanes.  With
 * `stats` (ampconv_softmax_stats_bytes(E, ...) bytes, 16-byte aligned; 0 = this dtype/shape keeps
 * none and `stats` must be NULL) the destination pass stores them at the edge's CSC position
 * (`spos`, ampconv_csc_positions) as 20 log2-sum-exp + 20 delta floats per (edge, head), and the
 * source pass -- which must then run AFTER the destination pass -- reads them back sequentially.
 * `out_absmax` (may be NULL; AMPCONV_F32 only): a device float that receives, by atomic max, the largest finite
 * magnitude of what the pass writes to dQ (dK and dV) -- the scale source of the projections that consume the
 * gradient (SCALED MODE below); the caller zeroes it, both passes may share one.  The destination pass's tile kernels
 * record it as they store (one compare per wave); the source pass and the other kernel families get it from one
 * ampconv_absmax pass over the output, run by the entry point -- the output must then be a plain row-major matrix (rows
 * of D channels, a node's L rows consecutive: head_stride = dh, node_stride = L * row_stride >= L * D) that pass can walk
 * in 16-byte pieces (base 16-byte aligned, D and row_stride multiples of 4).  Any other output view with out_absmax:
 * AMPCONV_E_BADARG, checked BEFORE anything is launched -- nothing has been written.  */
size_t ampconv_softmax_stats_bytes(int64_t E, int L, int D, int H, int dtype);
int ampconv_bwd_edge_dst(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                         ampconv_view_t dObar, const int32_t *rowptr,
                         const int32_t *col, int64_t n_rows, int L, int D, int H,
                         ampconv_view_t dQ, const void *hub_plan, int64_t hub_chunks,
                         void *hub_ws, const int32_t *spos, float *stats, float *out_absmax,
                         int dtype, void *stream);
int ampconv_bwd_edge_src(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                         ampconv_view_t dObar, const int32_t *cscptr,
                         const int32_t *crow, const float *cinv,
                         int64_t n_src, int L, int D, int H, ampconv_view_t dK,
                         ampconv_view_t dV, const void *hub_plan, int64_t hub_chunks,
                         void *hub_ws, const float *stats, float *out_absmax, int dtype,
                         void *stream);

/* ---- which kernels serve a call (a query: launches nothing, reads no device memory; a pure addition, the ABI number stays 111)
 * The fp32 / bf16 entry points above choose a kernel family from dtype, shape, the statistics hand-off and the ALIGNMENT
 * of every view of the call (base address and all three strides), in this order -- the first that applies:
 *   AMPCONV_FAMILY_BF16_MFMA  bf16 storage, L <= 20, dh = 32 or 16, every view 16-byte aligned (base; strides multiples
 *                             of 8).  Keeps no statistics: with `stats` AMPCONV_E_BADARG.
 *   AMPCONV_FAMILY_SMALL      fp32, L <= 4, no statistics, a token row on at most 64 lanes of v = 1, 2 or 4 channels (the
 *                             smallest v with D / v <= 64 and a head of dh / v = 4, 8, 16 or 32 lanes), every view
 *                             aligned to v floats (base 4 v bytes; strides multiples of v).
 *   AMPCONV_FAMILY_MFMA       fp32, L <= 20, dh = 32 or 16, every view 16-byte aligned (base; strides multiples of 4).
 *   AMPCONV_FAMILY_BLOCK      fp32 or bf16, L <= 64, even dh <= 64, every view aligned to two elements (base 8 / 4 bytes;
 *                             even strides); vectors of 4 elements where dh % 4 == 0 and every view allows it.  Its
 *                             source pass exists only WITH the statistics; with statistics the fp32 shapes of
 *                             AMPCONV_FAMILY_MFMA are not served (their buffer has that family's layout).
 *   AMPCONV_FAMILY_GENERIC    fp32, any shape and any 4-byte aligned view; no statistics (AMPCONV_E_BADARG), no
 *                             long-segment plan (it is ignored).
 * bf16 storage that neither bf16 family serves: AMPCONV_E_DTYPE (so: no source pass at the bf16 MFMA shapes on views that
 * are not 16-byte aligned).  A statistics buffer is taken only where ampconv_softmax_stats_bytes is non-zero for the
 * shape, and only by the family that function sized it for: any other call with `stats` returns AMPCONV_E_BADARG (fp32,
 * L <= 20, dh = 32 or 16 on 8-byte aligned views; every short-sequence shape) -- pass NULL there.  AMPCONV_FORCE_GENERIC=1 / AMPCONV_SMALL=0 in the
 * environment act here as in the passes.  pass: AMPCONV_PASS_*; stats != 0: the call passes a statistics buffer
 * (backward passes only); views: the n views of the call in argument order (Q, K, V[, dObar], outputs), n = 0: the shape
 * alone.  Returns the family, or the negative AMPCONV_E_* the pass would return for these arguments.  */
enum { AMPCONV_PASS_FWD = 0, AMPCONV_PASS_DST = 1, AMPCONV_PASS_SRC = 2 };
enum {
  AMPCONV_FAMILY_BF16_MFMA = 0,
  AMPCONV_FAMILY_SMALL = 1,
  AMPCONV_FAMILY_MFMA = 2,
  AMPCONV_FAMILY_BLOCK = 3,
  AMPCONV_FAMILY_GENERIC = 4
};
int ampconv_edge_family(int pass, int dtype, int L, int D, int H, int stats, const ampconv_view_t *views, int n);

/* ---- edge phase on fp16 PLANES: fp32-grade results off the FP32 pipe (csrc/edge_mfma_f16x2.hip, ABI 106) --------
 * The same three passes (same reference arithmetic: torch functional.py:6578-6594 per edge, amp_conv.py:11, SURVEY.md
 * A.2) for L <= 20, dh = 32 or 16, with Q, K, V and dObar in the PLANE FORMAT: the 4 dh-byte slot of the dh fp32 channels
 * of one (token row, head) holds dh fp16 `hi` then dh fp16 `lo` with hi + lo = x * 2^e (to 2^-22 |x|, absolute 2^-25 in
 * scaled units below that), ONE exponent per tensor: e = 14 - floor(log2 bound) for a device-side upper bound of the
 * tensor's magnitudes -- bounds[0] for Q | K | V (written by ONE ampconv_proj_rows_planes call), bounds[1] for dObar.
 * `bounds` (device, 4 floats) also carries what the backward passes scale dS = P (dP - delta) by before they split it:
 * bounds[2] = the largest |V| and bounds[3] = the largest |dObar| (true fp32 magnitudes, as recorded by the out_absmax
 * of the two ampconv_proj_rows_planes calls; any upper bound serves).  The forward pass reads bounds[0] only.
 * Views keep the strides, in 4-byte elements, of the fp32 tensor the planes replace; head_stride must be dh.  Every
 * product is the fp32 sum of three v_mfma_f32_16x16x32_f16 partial products (dropped: lo x lo <= 2^-22 of the product),
 * softmax and all sums are fp32, the outputs (Obar, dQ, dK, dV) plain fp32 views.
 * dObar must arrive DIVIDED by the in-degree of its node (ampconv_proj_rows_planes, row_scale = 1): the passes carry no
 * per-edge weight.  Softmax statistics as above (`stats`: E * H * 40 floats, 16-byte aligned, or NULL; `spos` with
 * them; delta is handed over in the units of the scaled dObar V^T product, which both passes share).  out_absmax as
 * above (both backward passes record it themselves).
 * planes_supported: 1 if (L, D, H) is served.  Same accuracy class as the fp32 kernels on tensors whose rows lie
 * within ~2^12 of the tensor's maximum (ampconv_absmax_stats measures exactly that; callers fall back to the fp32
 * entry points otherwise).  */
int ampconv_planes_supported(int L, int D, int H);
int ampconv_fwd_edge_planes(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                            const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D,
                            int H, ampconv_view_t O, const void *hub_plan, int64_t hub_chunks,
                            void *hub_ws, const float *bounds, void *stream);
int ampconv_bwd_edge_dst_planes(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                ampconv_view_t dObar, const int32_t *rowptr, const int32_t *col,
                                int64_t n_rows, int L, int D, int H, ampconv_view_t dQ,
                                const void *hub_plan, int64_t hub_chunks, void *hub_ws,
                                const float *bounds, const int32_t *spos, float *stats,
                                float *out_absmax, void *stream);
int ampconv_bwd_edge_src_planes(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                ampconv_view_t dObar, const int32_t *cscptr, const int32_t *crow,
                                int64_t n_src, int L, int D, int H, ampconv_view_t dK,
                                ampconv_view_t dV, const void *hub_plan, int64_t hub_chunks,
                                void *hub_ws, const float *bounds, const float *stats,
                                float *out_absmax, void *stream);

/* ---- edge phase on fp32 VIEWS with operand bounds: the workgroup-per-unit shapes off the FP32 pipe (csrc/edge_block_x3.hip,
 * ABI 107) ----------------------------------------------------------------------------------------------------------
 * The same three passes for L <= 64 and even dh <= 64 outside the one-wave-per-unit kernels' shapes (L <= 20 with dh = 32 or
 * 16) -- the reference's AMPGCN class defaults L = 40, D = 100, H = 2 (src/ampnet/module/amp_gcn.py:21-35), or 40 tokens at
 * its 128 / 4 -- on plain fp32 views -- what ampconv_fwd_edge / _bwd_edge_dst / _bwd_edge_src take --
 * plus the `bounds` of the plane-format entry points above: bounds[0] >= max |Q|K|V|, bounds[1] >= max |dObar|,
 * bounds[2] >= max |V|, bounds[3] >= max |dObar| (device, 4 floats; the forward pass reads bounds[0] only).  With them
 * the kernels split every fp32 tile, on its way into LDS, into TWO fp16 planes of x * 2^(14 - floor(log2 bound)) and
 * run each product as three v_mfma_f32_16x16x32_f16 partial products (half the matrix-pipe cycles and two thirds of
 * the vector instructions of the bound-free kernels behind the fp32 entry points, which split into three bf16 planes).
 * dObar is the gradient of the mean as in the fp32 entry points (the passes apply 1 / in-degree; `cinv` as in
 * ampconv_bwd_edge_src).  Softmax statistics: ampconv_softmax_stats_bytes(E, L, D, H, AMPCONV_F32) bytes, REQUIRED by
 * the source pass, delta in the units of the scaled dObar V^T product -- E * H * 32 * ceil(L / 16) floats, which is also
 * what these entry points need at the few shapes they serve where that function answers 0 because the fp32 entry points
 * keep no statistics there (the short-sequence shapes, e.g. L <= 4 at D = 64, H = 1).  out_absmax as above.  Same accuracy class as the
 * fp32 kernels on tensors whose rows lie within ~2^12 of the tensor's maximum (see ampconv_planes_supported).  */
int ampconv_scaled_supported(int L, int D, int H);
int ampconv_fwd_edge_scaled(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                            const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D,
                            int H, ampconv_view_t O, const void *hub_plan, int64_t hub_chunks,
                            void *hub_ws, const float *bounds, void *stream);
int ampconv_bwd_edge_dst_scaled(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                ampconv_view_t dObar, const int32_t *rowptr, const int32_t *col,
                                int64_t n_rows, int L, int D, int H, ampconv_view_t dQ,
                                const void *hub_plan, int64_t hub_chunks, void *hub_ws,
                                const float *bounds, const int32_t *spos, float *stats,
                                float *out_absmax, void *stream);
int ampconv_bwd_edge_src_scaled(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V,
                                ampconv_view_t dObar, const int32_t *cscptr, const int32_t *crow,
                                const float *cinv, int64_t n_src, int L, int D, int H,
                                ampconv_view_t dK, ampconv_view_t dV, const void *hub_plan,
                                int64_t hub_chunks, void *hub_ws, const float *bounds,
                                const float *stats, float *out_absmax, void *stream);

/* ---- edge phase, ONE query token per node (csrc/edge_token.hip) ------------------------------------------------------
 * The three passes for a layer whose output is read at a single token per node (AMPGCN(average_pooling_flag=False)
 * reads token 0 of conv2, src/ampnet/module/amp_gcn.py:266-271).  The arithmetic is that of "edge phase, forward /
 * backward" above with ONE query row per (node, head):
 *   Q, dObar, O, dQ   views whose element (n, h, c) is at ptr + n*node_stride + h*head_stride + c; row_stride is
 *                     ignored.  Token t of an [N, L, D] tensor is selected by offsetting ptr by t*row_stride elements.
 *   K, V, dK, dV      L tokens per node, as in every other family.
 * Per destination row d, head h and in-edge s -> d, deg = in-degree of d:
 *   p = softmax_j(q_h . K[s,j,h] / sqrt(dh))   (length L)
 *   O[d,h] = (1/deg) sum_edges sum_j p_j V[s,j,h]                     (exactly 0 when deg = 0)
 * backward, g = dObar[d,h] / deg (dObar is the gradient of the MEAN; `cinv` as in ampconv_bwd_edge_src):
 *   dp_j = g . V[s,j,h];  ds = p (dp - sum p dp)
 *   dQ[d,h] = sum_edges sum_j ds_j K[s,j,h] / sqrt(dh)               (exactly 0 when deg = 0)
 *   dK[s,j,h] = sum_out-edges ds_j q_h / sqrt(dh);  dV[s,j,h] = sum_out-edges p_j g    (exactly 0 without out-edges)
 * No atomics: every output row has one owner, sums run in CSR / CSC order, results are bitwise reproducible.  No
 * softmax statistics: the source pass keeps K[s], V[s] of its own node on chip and recomputes the softmax and
 * sum p dp per out-edge from the destination's q and dObar rows.  Long segments: the plans of ampconv_hub_plan; the
 * workspace holds [1, D] partial tiles for the forward and destination pass (ampconv_hub_workspace_bytes(n, 1, D, 1))
 * and [L, D] x 2 for the source pass (ampconv_hub_workspace_bytes(n, L, D, 2)), combined in the fixed order of every
 * other family.  Rows from n_rows / n_src on are not touched.  dtype: AMPCONV_F32 or AMPCONV_BF16 (bf16 in HBM, fp32
 * softmax and accumulation, one rounding on the way out).  K / V rows are read in 16-byte pieces where bases, strides
 * and dh allow, else in 8-, 4- (or, bf16, 2-) byte pieces: no view is refused for its alignment.
 * ampconv_token_supported: 1 for L <= 64, dh <= 64 (bf16: even dh).  Null pointers, D % H != 0, an unsupported shape or
 * dtype, or a hub workspace without a plan return AMPCONV_E_BADARG / AMPCONV_E_DTYPE before anything is launched.
 * These entry points were added without a change of AMPCONV_VERSION (no existing argument list changed).  */
int ampconv_token_supported(int L, int D, int H, int dtype);
int ampconv_fwd_edge_token(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, const int32_t *rowptr,
                           const int32_t *col, int64_t n_rows, int L, int D, int H, ampconv_view_t O,
                           const void *hub_plan, int64_t hub_chunks, void *hub_ws, int dtype, void *stream);
int ampconv_bwd_edge_dst_token(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                               const int32_t *rowptr, const int32_t *col, int64_t n_rows, int L, int D, int H,
                               ampconv_view_t dQ, const void *hub_plan, int64_t hub_chunks, void *hub_ws, int dtype,
                               void *stream);
int ampconv_bwd_edge_src_token(ampconv_view_t Q, ampconv_view_t K, ampconv_view_t V, ampconv_view_t dObar,
                               const int32_t *cscptr, const int32_t *crow, const float *cinv, int64_t n_src, int L,
                               int D, int H, ampconv_view_t dK, ampconv_view_t dV, const void *hub_plan,
                               int64_t hub_chunks, void *hub_ws, int dtype, void *stream);

/* ---- per-edge side outputs, ORIGINAL edge order ------------------------------
 * attn_weights: W[e] = mean_h softmax_rows(Q[dst e,:,h] K[src e,:,h]^T/sqrt(dh)),
 * [E, L, L] fp32 -- `self.attn_output_weights` (amp_conv.py:39,43-47; torch
 * functional.py:6604-6606).  */
int ampconv_attn_weights(ampconv_view_t Q, ampconv_view_t K,
                         const int64_t *edge_index, int64_t E, int L, int D,
                         int H, float *W, int dtype, void *stream);

/* attn_scores: the same without the softmax, W[e] = mean_h Q K^T / sqrt(dh) -- the per-edge weights of
 * the reference's softmax-free attention (custom_multihead_attn_forward.py:4173-4184, :4441-4442).  */
int ampconv_attn_scores(ampconv_view_t Q, ampconv_view_t K,
                        const int64_t *edge_index, int64_t E, int L, int D,
                        int H, float *W, int dtype, void *stream);

/* attn_heatmap: the feature-to-feature attention table of the reference's experiments/visualize_cora_attn_coeffs.py
 * (calculate_attn_heatmap, :212-216), accumulated without ever forming attn_weights' [E, L, L].  For every selected
 * edge e = (s -> d), destination token i and source token j with r = rowpos[s, j] >= 0 and c = colpos[d, i] >= 0:
 *     sum[r, c] += rint(W[e, i, j] * 2^AMPCONV_HEATMAP_SHIFT);   cnt[r, c] += 1
 * with W the head-mean softmax weight of ampconv_attn_weights.  INDEX CONVENTION, as in the reference: ROW = feature
 * of the SOURCE token, COLUMN = feature of the DESTINATION token; heat = sum / 2^SHIFT / cnt (0 where cnt == 0).
 * rowpos / colpos [N, L] int32: position of each token's feature among the selected source / destination features,
 * -1 (or anything outside [0, rows) / [0, cols)) = not selected.  A feature id that a node holds twice counts once per
 * token.  edge_mask [E] bytes or NULL (all edges); edges with a node id outside [0, N) are ignored.  sum / cnt
 * [rows, cols] int64, 8-byte aligned, ACCUMULATED INTO: the caller zeroes them.  Integer adds (vector atomics): the
 * tables are bitwise independent of launch order and of how the edges are split over calls.  Per-term error
 * <= 2^-(SHIFT+1).  prior_triples: the (edge, i, j) triples the tables may already hold; a call that could take a cell
 * past INT64_MAX (prior_triples + E L^2 > AMPCONV_HEATMAP_MAX_TRIPLES) returns AMPCONV_E_BADARG.  E == 0 is OK.
 * dtype: AMPCONV_F32 views only (else AMPCONV_E_DTYPE).  Tables of at most 4096 cells are accumulated per workgroup in
 * LDS and flushed once; AMPCONV_HEATMAP_GLOBAL=1 in the environment pins the direct global accumulation.  */
#define AMPCONV_HEATMAP_SHIFT 28
#define AMPCONV_HEATMAP_MAX_TRIPLES ((((int64_t)1) << (63 - AMPCONV_HEATMAP_SHIFT)) - 1)
int ampconv_attn_heatmap(ampconv_view_t Q, ampconv_view_t K, const int64_t *edge_index, int64_t E,
                         int64_t N, const uint8_t *edge_mask, const int32_t *rowpos,
                         const int32_t *colpos, int L, int D, int H, int rows, int cols, int64_t *sum,
                         int64_t *cnt, int64_t prior_triples, int dtype, void *stream);
int ampconv_attn_heatmap_shift(void);   /* AMPCONV_HEATMAP_SHIFT of the loaded build */

/* ---- node-side helpers --------------------------------------------------------
 * segment_mean: PyG aggr='mean' on an [E, F] message matrix (amp_conv.py:11,
 * testing_message_passing_pyg.py:37-40): out[n] = mean of msg[eperm[p]] over the
 * CSR segment of n, 0 for empty segments.
 * mask_rows: zero, in place, the rows of Y[N, F] whose CSR segment is empty
 * (out-projection bias must not leak into nodes nobody sends to).
 * masked_colsum: out[f] = sum over rows with a non-empty segment of dY[n, f],
 * folded over the L tokens: out has D fp32 entries (out_proj.bias gradient).
 * `dtype` of Y / dY: AMPCONV_F32 or AMPCONV_BF16.
 * mask_rows stores +0 over the rows it zeroes, whatever they held (NaN and infinity included), and reads and writes
 * no other row.  It has two paths with the same result: 16-byte stores where Y is 16-byte aligned AND a row is a
 * multiple of 16 bytes (F * sizeof % 16 == 0), element stores for any other base address or row length -- no alignment
 * is asked of the caller.  `rowptr` may be the `ptr` array of ampconv_active_nodes: the rows of the nodes a list
 * leaves out are zeroed.
 * masked_colsum does not read the rows it leaves out (they may hold NaN); N == 0 gives D zeros; the result is bitwise
 * reproducible.  `out` needs room for D results followed by a scratch area of 1024 * D floats.
 * segment_mean: a message row no edge names is not read; E == 0 (every segment empty) gives zeros, msg may be NULL.  */
int ampconv_segment_mean(const float *msg, const int32_t *rowptr,
                         const int32_t *eperm, int64_t N, int64_t F, float *out,
                         void *stream);
int ampconv_mask_rows(void *Y, const int32_t *rowptr, int64_t N, int64_t F,
                      int dtype, void *stream);
/* gather_segment_sum: out[r, :] = scale_r * sum_{p in [ptr[r], ptr[r+1])} (w ? w[p] : 1) * rows[idx[p], :]
 * with F (a multiple of 4) fp32 per row, scale_r = 1/segment length if `mean` else 1, 0 for empty
 * segments.  The whole edge phase of the softmax-free variant ("next" row 3 of SURVEY.md 8f): without
 * softmax, sum_e Q_d K_s^T V_s = Q_d sum_e (K_s^T V_s), so the per-edge work collapses to this
 * segment reduction of the per-source dh x dh matrices K_s^T V_s (forward: CSR, mean; backward:
 * CSC, weights cinv).  */
int ampconv_gather_segment_sum(const float *rows, const int32_t *ptr, const int32_t *idx,
                               const float *w, int mean, int64_t N, int64_t F, float *out,
                               void *stream);
/* The per-node products around it (custom_multihead_attn_forward.py:4173-4184 re-associated), one
 * [L, dh] tile per (node, head) on either side, M = [N, H, dh, dh] fp32 row-major:
 *   linear_outer: M[n,h] = scale * A[n,:,h]^T B[n,:,h]      (K^T V; Q^T dObar for the backward)
 *   linear_apply: Out[n,:,h] = scale * A[n,:,h] M[n,h]      (transpose != 0: ... M[n,h]^T)
 *                 (Q Mbar; dObar Mbar^T, V dM^T, K dM for the backward)
 * Any dh, odd ones included (only the Python layer asks for an even head width); fp32 only.  One wavefront per
 * (node, head) holds both operands of a unit in LDS, rows padded to dh | 1 floats, and a call that would need more than
 * 64 KiB of it is refused: AMPCONV_E_BADARG, nothing launched or written, where
 *   linear_outer: 2 L (dh | 1) * 4 > 65536   (dh = 64: L <= 126 is served, 127 is not)
 *   linear_apply: (L + dh) (dh | 1) * 4 > 65536   (dh = 64: L <= 188; dh = 128 at no L).
 * Also refused with AMPCONV_E_BADARG: a NULL M or view pointer, D % H != 0, and a view with a zero node, row or head
 * stride (it would fold units onto each other).  N == 0 returns AMPCONV_OK and touches nothing.  */
int ampconv_linear_outer(ampconv_view_t A, ampconv_view_t B, int64_t N, int L, int D, int H,
                         float scale, float *M, void *stream);
int ampconv_linear_apply(ampconv_view_t A, const float *M, int transpose, int64_t N, int L,
                         int D, int H, float scale, ampconv_view_t Out, void *stream);
int ampconv_masked_colsum(const void *dY, const int32_t *rowptr, int64_t N,
                          int L, int D, float *out, int dtype, void *stream);

/* ---- node phase: the per-node projections ---------------------------------------------------
 * Replaces the packed in-projection (torch functional.py:5785-5862 `_in_projection_packed`; the
 * reference's copy src/ampnet/conv/custom_multihead_attn_forward.py:4070-4077) and the
 * out-projection (torch functional.py:6600), once per NODE instead of once per edge, and their
 * autograd backward (dObar = dY Wo, dX = dQKV Win, dW = dOut^T In, db = colsum).
 * `dtype` names the storage of EVERY tensor of a call (rows, weights, bias, outputs, gradients):
 *   AMPCONV_F32   fp32 in, fp32 out, fp32 accumulate; every operand element is split EXACTLY into three bf16 terms
 *                 and a product is the sum of the six partial products of order >= 2^-16 on
 *                 v_mfma_f32_32x32x16_bf16 (error of the dropped terms <= 3 * 2^-26 per product: fp32 grade).
 *                 Non-finite inputs: NaN propagates; +-Inf (and |x| above the largest bf16, 3.39e38) comes out as
 *                 NaN where an fp32 GEMM would return +-Inf (the residual planes are inf - inf).
 *   AMPCONV_BF16  bf16 in HBM (BASELINE config 5), ONE product per fragment pair on the same instruction, fp32
 *                 accumulate, results rounded to bf16 once (weight / bias gradients: after the ordered fp32 sum over
 *                 the row slices).  The weight-gradient PRODUCT is not masked in this mode (the in-degree mask acts
 *                 on the column sums only): the rows of nodes without in-edges contribute nothing because the other
 *                 operand (the forward pass's Obar) is exactly 0 there -- as in a plain dY^T Obar.
 *   proj_supported     : 1 if (N, K) is served, else 0 -- the caller then uses a library GEMM.  fp32: both multiples
 *                        of 4, bf16: of 8 (rows are read and written in 16-byte pieces); tiles are padded
 *                        internally, so the reference's default embed_dim = 100 is served in fp32
 *   proj_weight_image  : B[n][k] = W[n * stride_n + k * stride_k] (N x K) -> `image`
 *                        (proj_weight_image_bytes(N, K, dtype) bytes, 16-byte aligned): the weight as ready MFMA
 *                        fragments (fp32: its three bf16 planes), zero-padded.  (stride_n, stride_k) = (K, 1) uses a
 *                        row-major [N, K] weight as it stands (forward), (1, N) its transpose (backward).
 *   proj_weight_images : up to 8 of them in ONE launch (forward and transposed images of both weights of a layer)
 *   proj_rows          : out[m, :N] = (A[m, :K] B^T + bias) * (rowptr ? [node m / L has an in-edge] : 1)
 *                        A row-major with leading dimension lda (elements), out with ldc
 *   proj_wgrad         : dW[Na, Nb] = sum_m (mask_m A[m, :Na])^T B[m, :Nb] and colsum[Na] = sum_m mask_m A[m, :Na]
 *                        (mask as above, rowptr may be NULL; bf16: see above); deterministic: fixed row slices,
 *                        ordered sum.  `workspace`: proj_wgrad_workspace_bytes(M, Na, Nb, dtype) bytes.
 *   NODE LISTS (`nodes` != NULL, AMPCONV_BF16 only, 16 <= L <= 128; NULL: every row): only the L rows of each of the
 *   n_nodes listed nodes (ascending node ids < M / L; the array must be readable for 8 entries past n_nodes:
 *   ampconv_active_nodes makes such lists) are read, multiplied and -- proj_rows -- written; all other rows of
 *   `out` are left untouched.  proj_wgrad's workspace is then sized for the listed rows:
 *   proj_wgrad_workspace_bytes(n_nodes * L, ...).  The per-node formulation computes a projection for EVERY node, the reference one per EDGE:
 *   a node without in-edges needs no Q row and no output row (it is 0), one without out-edges no K / V rows -- on the
 *   R-MAT graph of BASELINE config 5 that is 48 % of the nodes on either side.  proj_rows with a list takes no mask
 *   (rowptr must be NULL: list the nodes that pass it); proj_wgrad sums over the listed rows only.
 *   SCALED MODE (AMPCONV_F32 only; `a_absmax` (+ `b_absmax` for proj_wgrad) != NULL: device floats holding the largest
 *   finite magnitude of the operand, or any upper bound of it within a few binades): the operands are scaled by a power
 *   of two into fp16's range and split into TWO fp16 planes, a product is three fp16 matrix products instead of six bf16
 *   ones -- as close to the fp64 result as the six-product form on operands whose elements lie within 2^17 of the
 *   maximum, absolute error <= 2^-39 of the maximum per element below that (csrc/proj_gemm.hip); the
 *   weight's scale is part of its image.  NULL: the six-product form, exact split at any range.  ampconv_absmax
 *   computes such a maximum (one pass over X[M, K], row stride ld; merged into *out by atomic max, `reset` zeroes it
 *   first; NaN and infinities are skipped); proj_rows in this mode records the maximum of what it WRITES into `out_absmax` (may be
 *   NULL; atomic max, the caller zeroes it) -- the next product's operand then needs no pass of its own.
 * Developer switches read from the environment at the first call (A/B measurements; the defaults are the
 * shipped configuration, nothing else keeps state; the projections have none: their tile shapes follow from the
 * problem shape alone), for the edge phase AMPCONV_FORCE_GENERIC=1,
 * AMPCONV_SMALL=0 (L <= 4 on the tile kernels instead of the short-sequence family), AMPCONV_{FWD,DST,SRC}_T4=0,
 * AMPCONV_{FWD,DST,SRC}_NT4=0 (older tilings of the same kernels, kept as cross-checks for the tests),
 * AMPCONV_CSR_SMALL=0 (graph preparation by the multi-launch path).  */
int ampconv_proj_supported(int N, int K, int dtype);
size_t ampconv_proj_weight_image_bytes(int N, int K, int dtype);
int ampconv_proj_weight_image(const void *W, int64_t stride_n, int64_t stride_k, int N, int K,
                              void *image, int dtype, void *stream);
typedef struct {
  const void *W;
  int64_t stride_n, stride_k;
  int N, K;
  void *image;
} ampconv_weight_image_t;
int ampconv_proj_weight_images(int count, const ampconv_weight_image_t *jobs, int dtype, void *stream);
int ampconv_proj_rows(const void *A, int64_t lda, int64_t M, int K, const void *wimage, int N,
                      const void *bias, const int32_t *rowptr, int L, void *out, int64_t ldc,
                      const int32_t *nodes, int64_t n_nodes, const float *a_absmax,
                      float *out_absmax, int dtype, void *stream);
size_t ampconv_proj_wgrad_workspace_bytes(int64_t M, int Na, int Nb, int dtype);
int ampconv_proj_wgrad(const void *A, int64_t lda, const void *B, int64_t ldb, int64_t M, int Na,
                       int Nb, const int32_t *rowptr, int L, void *dW, void *colsum,
                       void *workspace, size_t workspace_bytes, const int32_t *nodes, int64_t n_nodes,
                       const float *a_absmax, const float *b_absmax, int dtype, void *stream);
int ampconv_absmax(const void *X, int64_t ld, int64_t M, int K, int dtype, float *out, int reset,
                   void *stream);
/* PLANE OUTPUT (fp32 storage, scaled mode; N % 128 == 0, K % 32 == 0, ldc % 32 == 0): proj_rows whose result leaves in
 * the plane format of the edge kernels above instead of fp32 -- same bytes, same layout of 128-byte slots.
 *   proj_out_bound  : out[0] = *a_absmax * max_n sum_k |B[n][k]| + max_n |bias[n]| (B as in proj_weight_image): an upper
 *                     bound of |A B^T + bias| that is known BEFORE the product runs; the scale of its planes
 *   proj_rows_planes: as proj_rows; `out_bound` = that device float; plane_dh = 32 or 16: the slot width (head dimension); row_scale = 1 (with rowptr): rows are also DIVIDED
 *                     by their node's segment length (dObar / in-degree); out_absmax (may be NULL) records the largest
 *                     finite magnitude of the fp32 values behind the planes over the columns >= absmax_col0 only (the V
 *                     third of a packed in-projection bounds Obar, a mean of convex combinations of V rows)
 *   planes_to_f32   : the reverse: out[m, k] = (hi + lo) * 2^-e of X[M, K] in plane format (side outputs, fall-backs)
 *   absmax_stats    : out[0] = largest finite magnitude of X[M, K] (fp32), out[1] = the smallest NON-ZERO maximum of any
 *                     group of 8 consecutive 16-byte pieces (32 channels: a head slot); out[1] * 2^12 < out[0] says that
 *                     whole rows / heads lie far below the tensor's maximum: one scale per tensor then costs them their
 *                     low plane and the caller should use the exact kernels (six-product projections, fp32 edge passes)  */
int ampconv_proj_out_bound(const void *W, int64_t stride_n, int64_t stride_k, int N, int K,
                           const void *bias, const float *a_absmax, float *out, void *stream);
int ampconv_proj_rows_planes(const void *A, int64_t lda, int64_t M, int K, const void *wimage, int N,
                             const void *bias, const int32_t *rowptr, int L, int row_scale, void *out,
                             int64_t ldc, const float *a_absmax, const float *out_bound,
                             float *out_absmax, int absmax_col0, int plane_dh, void *stream);
int ampconv_planes_to_f32(const void *X, int64_t ld, int64_t M, int K, int plane_dh, const float *bound,
                          void *out, int64_t ldo, void *stream);
int ampconv_absmax_stats(const void *X, int64_t ld, int64_t M, int K, float *out, void *stream);

/* ---- GraphSAINT random-walk sampler ("next" row: the step before the hot path) -------------
 * In-tree spec: the reference's vendored PyG sampler, visualization/visualize_graphsaint_subgraphs.py
 * :195-199 (walks), :107-110 (unique nodes + induced sub-graph), :137-173 (norms).  The graph is
 * given as the src-sorted CSC of ampconv_csr_build (cscptr, crow = destinations, cperm = original
 * edge ids).  The caller reads n_sub / e_sub (device int32) back to size the next outputs.
 *   random_walk : walks[b, 0] = start[b]; each step moves to a uniform random out-neighbour
 *                 (stays if none); counter-based generator keyed by (seed, walk, step)
 *   nodes       : walked nodes (with repeats) -> mark[N], relabel[N], node_idx (sorted unique)
 *   count/fill  : induced sub-graph, edges grouped by source in CSC order: relabelled
 *                 edge_index [2, e_sub] and the original edge ids (count_edges_bounded: the same before
 *                 the host knows n_sub -- an upper bound sizes cnt / off, n_sub is read on the device --
 *                 so that n_sub and e_sub come back in ONE read)
 *   add_counts  : count[idx[i]] += 1 (occurrence statistics of nodes / edges)
 *   norms       : edge_norm = clamp(node_count[src] / edge_count, 0, 1e4) (NaN -> 0.1),
 *                 node_norm = num_samples / max(node_count, 0.1 if 0) / N
 *
 * THE WALK STREAM (a contract, like THE MASK below: tests rebuild it on the host, tests/pipeline_reference.py).  With
 *   draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b))      (uint64, wrapping; all 64 bits of seed)
 * step t = 0, 1, ... of walk b leaves the current node u, of out-degree deg = cscptr[u + 1] - cscptr[u], for
 *   crow[cscptr[u] + draw(seed, b, t) % deg]
 * -- the (draw % deg)-th out-edge of u in CSC order, a duplicate edge counting once per copy -- and stays at u if
 * deg == 0.  walk_length == 0 writes the starts alone.  A (seed, graph, starts) triple therefore always gives the same
 * walks, on any device and in any launch shape.
 * THE ORDER OF A SUB-GRAPH is part of the contract too: node_idx ascends; the edges of fill_edges stand at exact
 * positions, grouped by source in ascending relabelled source k, within a source in CSC order (= ascending original
 * edge id, the CSC being a stable sort), edge o of source k at off[k] + o.  Batches are reproducible element for
 * element, not only as sets.  */
int ampconv_saint_random_walk(const int32_t *cscptr, const int32_t *crow, const int64_t *start,
                              int64_t B, int walk_length, uint64_t seed, int64_t *walks, void *stream);
size_t ampconv_saint_workspace_bytes(int64_t N);
int ampconv_saint_nodes(const int64_t *nodes, int64_t n, int64_t N, int32_t *mark, int32_t *relabel,
                        int64_t *node_idx, int32_t *n_sub, void *workspace, size_t workspace_bytes,
                        void *stream);
int ampconv_saint_count_edges(const int64_t *node_idx, int64_t n_sub, const int32_t *cscptr,
                              const int32_t *crow, const int32_t *mark, int32_t *cnt, int32_t *off,
                              int32_t *e_sub, void *workspace, size_t workspace_bytes, void *stream);
int ampconv_saint_count_edges_bounded(const int64_t *node_idx, int64_t n_bound, const int32_t *n_sub_dev,
                                      const int32_t *cscptr, const int32_t *crow, const int32_t *mark,
                                      int32_t *cnt, int32_t *off, int32_t *e_sub, void *workspace,
                                      size_t workspace_bytes, void *stream);
int ampconv_saint_fill_edges(const int64_t *node_idx, int64_t n_sub, const int32_t *cscptr,
                             const int32_t *crow, const int32_t *cperm, const int32_t *mark,
                             const int32_t *relabel, const int32_t *off, int64_t E_sub,
                             int64_t *edge_index, int64_t *edge_id, void *stream);
int ampconv_saint_add_counts(const int64_t *idx, int64_t n, float *count, void *stream);
int ampconv_saint_norms(const float *node_count, const float *edge_count, const int64_t *edge_src,
                        int64_t N, int64_t E, float num_samples, float *node_norm, float *edge_norm,
                        void *stream);
/* gather_rows: the batch's rows of a resident per-node tensor, dst[i, :] = src[idx[i], :] (the collate step of the
 * vendored sampler, visualize_graphsaint_subgraphs.py:112-135: `item[node_idx]`).  Rows of row_bytes bytes (a multiple of
 * 16, both tensors 16-byte aligned, src rows src_stride_bytes apart), idx in [0, n_src).  */
int ampconv_saint_gather_rows(const void *src, int64_t src_stride_bytes, int64_t row_bytes, const int64_t *idx,
                              int64_t n, void *dst, void *stream);

/* ---- AMPGCN featuriser ("next" row: the step right before the first AMPConv layer) ----------
 * Reference src/ampnet/module/amp_gcn.py:120-183: z-score of the node features (:122-125), L present
 * (non-zero) features sampled per node with replacement (:132-135), token = concat(embedding row,
 * z-scored value) (:146-147).  x is [N, F] fp32, idx [N, L] int32 (-1 = node without any present
 * feature; `empty_flag` is raised), table [F, De], out [N, L, De + 1].  table_grad zeroes dtable and
 * accumulates the token gradients with float atomics: rows no token names come back as exact zeros whatever dtable
 * held; a token with idx -1 gives a zero row in feat_build and adds nothing in table_grad.
 *
 * THE SAMPLING STREAM (a contract, like THE MASK below: tests rebuild it on the host, tests/pipeline_reference.py).
 * With draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b)) (uint64, wrapping; all 64 bits of seed)
 * and count = the number of present columns of row n:
 *   idx[n, l] = the (draw(seed, n, l) % count)-th present column of row n, counted from 0 in ascending column order.
 * PRESENT means x[n, f] != 0 for a finite value: -0.0 is absent, denormals and negative values are present (the kernels
 * run with fp32 denormals on).  The library is built with -fno-honor-nans, so a NaN feature has NO defined presence
 * (today's build treats it as absent; numpy's `!=` would call it present): keep NaN out of x.
 * ACCURACY OF THE STATISTICS: zscore_stats accumulates in double (population variance; sklearn's constant-feature rule
 * var <= N eps var + (N mean eps)^2 gives scale 1) and returns mean and inv_std rounded to fp32, each within 1 ulp.  z is
 * then assembled in fp32 as (x - mean) * inv_std, so the rounding of `mean` alone moves z by up to
 * |mean| inv_std 2^-24: |z - z_fp64| <= 2^-24 (2 |mean| inv_std + 4 |z|).  For a column whose mean is large against its
 * spread (1000 +- 0.01: |mean| inv_std = 1e5) that is 1e-2, not the 1e-7 of a centred column.  */
int ampconv_feat_zscore_stats(const float *x, int64_t N, int64_t F, float *mean, float *inv_std,
                              void *stream);
int ampconv_feat_sample_present(const float *x, int64_t N, int F, int L, uint64_t seed, int32_t *idx,
                                int32_t *empty_flag, void *stream);
int ampconv_feat_build(const float *x, const float *mean, const float *inv_std, const int32_t *idx,
                       const float *table, int64_t N, int F, int L, int De, float *out, void *stream);
int ampconv_feat_table_grad(const float *dout, const int32_t *idx, int64_t N, int L, int De, int F,
                            float *dtable, void *stream);
/* The same two with the token storage given (`dtype`: AMPCONV_F32 or AMPCONV_BF16, else AMPCONV_E_DTYPE; pure additions,
 * the ABI number stays 111).  feat_build_as: every element of `out` is the round-to-nearest-even `dtype` value of what
 * ampconv_feat_build writes, for any De >= 0.  feat_table_grad_from: `dout` [N, L, De + 1] is read in `dtype`, widened and
 * accumulated in fp32 into the fp32 dtable, with the same float atomics.  */
int ampconv_feat_build_as(const float *x, const float *mean, const float *inv_std, const int32_t *idx,
                          const float *table, int64_t N, int F, int L, int De, void *out, int dtype, void *stream);
int ampconv_feat_table_grad_from(const void *dout, const int32_t *idx, int64_t N, int L, int De, int F, float *dtable,
                                 int dtype, void *stream);

/* ---- glue around the layers: activation, dropout, token pooling (csrc/glue.hip, ABI 109) ------------------------
 * Reference src/ampnet/module/amp_gcn.py:239-276: drop1 -> conv1 -> ReLU -> drop2 -> conv2 -> ReLU -> drop3 -> token
 * pooling (:268-271: mean over the L tokens, or token 0); amp_net_classifier_Rahul.py:45-57: the same with ELU.  Each
 * site is ONE pass over the [N, L*D] tensor, and no dropout mask is ever stored: both passes regenerate it.
 *
 * THE MASK (a contract: tests rebuild it on the host, tests/glue_reference.py).  Let i be the flat row-major index of
 * an element of the logical [N, L*D] tensor and
 *     splitmix64(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
 *                     x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)        (64-bit, wrapping)
 *     g = i >> 2;   h = splitmix64(seed ^ splitmix64(g));   f = (h >> (16 * (i & 3))) & 0xFFFF
 * The element is KEPT iff f >= threshold.  The caller passes threshold = round(p * 65536) <= 65535 (else
 * AMPCONV_E_BADARG) and scale = 65536 / (65536 - threshold) as a float: the inverse of the EFFECTIVE keep probability,
 * so E[keep * scale] = 1 exactly.  One hash serves four elements on purpose (a 64-bit hash per element would cost more
 * vector instructions than the chip has per byte streamed from HBM).  The mask depends on (seed, i) only: it is the
 * same for every dtype, vector width and launch shape.  threshold = 0 keeps everything; with scale = 1 the result is
 * then bit-identical to the activation alone.
 *
 * act: AMPCONV_ACT_IDENTITY, _RELU, _ELU (alpha = 1).  dtype: AMPCONV_F32 or AMPCONV_BF16 = the storage of every tensor
 * of the call; arithmetic is fp32.  Tensors are contiguous.  16-byte aligned bases with n (act_dropout) or D (pool) a
 * multiple of 16 bytes are streamed in 16-byte pieces; anything else (the XOR toy's L = 2, D = 3) runs element-wise.
 *   act_dropout_fwd: y[i] = keep(i) ? act(x[i]) * scale : 0                                     n elements
 *   act_dropout_bwd: dx[i] = keep(i) ? dy[i] * scale * act'(x[i]) : 0, act' taken from the saved OUTPUT y (ReLU: y > 0;
 *                    ELU: a = y / scale, a > 0 ? 1 : a + 1; identity: 1 and y may be NULL) -- y is what the next layer
 *                    saves as its input anyway, so the site adds no saved tensor
 *   pool_fwd:        pooled[n, c] = (1 / L) sum_l keep * act(x[n, l, c]) * scale (AMPCONV_POOL_MEAN), or the l = 0 term
 *                    alone (AMPCONV_POOL_TOKEN0); x [N, L, D], pooled [N, D]; one fp32 chain per output in ascending l,
 *                    no atomics: bitwise reproducible
 *   pool_bwd:        dx[n, l, c] = act'(x[n, l, c]) * keep * scale * dpooled[n, c] / L; token 0: without the 1 / L and
 *                    rows l > 0 are written as exact zeros.  x is the input of pool_fwd (identity: may be NULL).  */
enum { AMPCONV_ACT_IDENTITY = 0, AMPCONV_ACT_RELU = 1, AMPCONV_ACT_ELU = 2 };
enum { AMPCONV_POOL_MEAN = 0, AMPCONV_POOL_TOKEN0 = 1 };
int ampconv_act_dropout_fwd(const void *x, int64_t n, int act, uint64_t seed, uint32_t threshold,
                            float scale, void *y, int dtype, void *stream);
int ampconv_act_dropout_bwd(const void *dy, const void *y, int64_t n, int act, uint64_t seed,
                            uint32_t threshold, float scale, void *dx, int dtype, void *stream);
int ampconv_pool_fwd(const void *x, int64_t N, int L, int D, int act, int pooling, uint64_t seed,
                     uint32_t threshold, float scale, void *pooled, int dtype, void *stream);
int ampconv_pool_bwd(const void *x, const void *dpooled, int64_t N, int L, int D, int act, int pooling,
                     uint64_t seed, uint32_t threshold, float scale, void *dx, int dtype, void *stream);

/* ---- classifier head and GraphSAINT-weighted NLL loss (csrc/head.hip, ABI 110) --------------------------------------
 * Reference src/ampnet/module/amp_gcn.py:272-276 (final_linear_out, then log_softmax or, with softmax_out=False, the
 * sigmoid) and experiments/cora_benchmark_graphsaint.py:105-128:
 *     loss = (F.nll_loss(out, y, reduction='none') * node_norm)[mask].sum();  acc = (out.argmax(1) == y)[mask].mean()
 * pooled [N, D]: row n starts `stride` elements (>= D) behind row n - 1; dtype AMPCONV_F32 or AMPCONV_BF16 is ITS storage
 * (and dpooled's, which is contiguous [N, D]).  W [C, D] and b [C] are contiguous fp32, 1 <= C <= AMPCONV_HEAD_MAX_CLASSES,
 * D >= 1; all arithmetic is fp32.  Rows are read in 16-byte pieces where pooled, W and dpooled are 16-byte aligned and
 * D and stride are whole pieces, element by element otherwise.  No [N, C] tensor is written except the `out` / `logp`
 * the caller passes.  C outside 1..64, negative sizes, stride < D, an unknown kind, M outside 1..4 or grad_mask outside
 * [0, M): AMPCONV_E_BADARG; another dtype: AMPCONV_E_DTYPE; a short workspace: AMPCONV_E_WORKSPACE -- nothing is launched.
 * N == 0 succeeds: dW and db are written as zeros, the loss as 0, nothing is accumulated.
 *   head_fwd:  out[n, :] = log_softmax(pooled[n] W^T + b) (kind AMPCONV_HEAD_LOG_SOFTMAX; the row maximum is subtracted
 *              before exp) or sigmoid(...) (AMPCONV_HEAD_SIGMOID); out [N, C] fp32 contiguous.
 *   head_bwd:  dz = dout - exp(out) * rowsum(dout) (log_softmax) or dout * out * (1 - out) (sigmoid) from the saved out;
 *              dpooled = dz W (may be NULL: not wanted), dW = dz^T pooled, db = colsum(dz).
 *   head_nll_fwd: with logp = log_softmax(pooled W^T + b), labels y [N] int64, weights w [N] fp32 (NULL: 1), masks [M, N]
 *              bytes (NULL: M == 1, one all-true mask).  Node n is SELECTED by mask m when masks[m, n] != 0 and
 *              y[n] != AMPCONV_HEAD_IGNORE_INDEX (torch's ignore_index).  A selected node whose label is outside [0, C)
 *              is never used as an index: it is skipped by every mask and counted once in the bad-labels slot.  Per mask m,
 *              ADDED to metrics (int64 [AMPCONV_HEAD_METRICS_SLOTS], the caller zeroes it; NULL: not wanted):
 *                  metrics[3 m]     += sum_n rint(w[n] * -logp[n, y[n]] * 2^AMPCONV_HEAD_LOSS_SHIFT)
 *                  metrics[3 m + 1] += selected nodes;   metrics[3 m + 2] += those with argmax_c logp[n, c] == y[n]
 *                  metrics[12]      += bad labels                  (argmax ties: the lowest class, as torch.argmax)
 *              *loss (fp32, device) = this call's loss sum of mask grad_mask / 2^SHIFT.  logp [N, C] is written if not
 *              NULL.  scratch: AMPCONV_HEAD_METRICS_SLOTS int64 of the caller's, overwritten (the call's own sums).
 *   head_nll_bwd: dz[n] = *g * w[n] * [n selected by grad_mask, label in range] * (softmax[n] - onehot(y[n])) with the
 *              upstream gradient *g read ON THE DEVICE, then dpooled, dW, db as head_bwd.  Rows without a gradient get
 *              exact zeros written.
 * DETERMINISM.  Every output has the same bits on every launch.  dW and db: a fixed-order two-stage reduction --
 * workgroup partials [workgroups, C, D + 1] in `workspace` (ampconv_head_workspace_bytes(N, D, C); need not be zeroed),
 * added in workgroup order by a second kernel; no floating-point atomics anywhere.  The metric sums: 64-bit integer
 * atomics, the loss terms in fixed point with AMPCONV_HEAD_LOSS_SHIFT = 32 fraction bits: per-term error <= 2^-33, and a
 * running |sum| below 2^31 (e.g. 10^6 nodes of weighted loss 2000 each) is exact integer arithmetic.  */
enum { AMPCONV_HEAD_LOG_SOFTMAX = 0, AMPCONV_HEAD_SIGMOID = 1 };
#define AMPCONV_HEAD_MAX_CLASSES 64
#define AMPCONV_HEAD_MAX_MASKS 4
#define AMPCONV_HEAD_METRICS_SLOTS 13
#define AMPCONV_HEAD_LOSS_SHIFT 32
#define AMPCONV_HEAD_IGNORE_INDEX (-100)
size_t ampconv_head_workspace_bytes(int64_t N, int D, int C);
int ampconv_head_fwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, const float *b, int C,
                     int kind, float *out, int dtype, void *stream);
int ampconv_head_bwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, int C, int kind,
                     const float *dout, const float *out, void *dpooled, float *dW, float *db, void *workspace,
                     size_t workspace_bytes, int dtype, void *stream);
int ampconv_head_nll_fwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, const float *b, int C,
                         const int64_t *y, const float *w, const uint8_t *masks, int M, int grad_mask, float *logp,
                         int64_t *metrics, int64_t *scratch, float *loss, int dtype, void *stream);
int ampconv_head_nll_bwd(const void *pooled, int64_t N, int D, int64_t stride, const float *W, const float *b, int C,
                         const int64_t *y, const float *w, const uint8_t *masks, int M, int grad_mask, const float *g,
                         void *dpooled, float *dW, float *db, void *workspace, size_t workspace_bytes, int dtype,
                         void *stream);

/* ---- per-token LayerNorm sites (csrc/norm.hip, ABI 111) --------------------------------------------------------------
 * Reference experiments/cora_overfit_one_subgraph.py:46-107: behind each AMPConv layer
 *     reshape [N, L, D] -> nn.LayerNorm(D) -> ReLU -> reshape back,      the last one followed by the token pooling
 * (amp_net_classifier_Rahul.py:17 defines the same LayerNorm).  Each site is ONE pass over the [N, L*D] tensor per
 * direction: the normalisation, the activation, the dropout of THE MASK above and, for the pooled calls, the token
 * pooling of ampconv_pool_fwd / _bwd.  With T = N L tokens of D channels, x contiguous [T, D]:
 *     mu_t = mean_c x[t, c];   var_t = mean_c (x[t, c] - mu_t)^2   (biased; from the centred values, not E[x^2] - mu^2)
 *     rstd_t = 1 / sqrt(var_t + eps);   xhat = (x - mu) rstd;   z = xhat gamma[c] + beta[c]
 * keep(i) and scale are those of THE MASK with i = t D + c, the flat index in the logical [N, L*D] tensor: a norm site
 * with seed s drops the elements an act_dropout site with seed s drops.  act: AMPCONV_ACT_*.
 *   norm_fwd:      y[t, c] = keep ? act(z) scale : 0;   stats[t] = (mu_t, rstd_t), fp32 [T, 2]
 *   norm_bwd:      from x, dy, stats, gamma, beta (z is recomputed; act' from z: ReLU z > 0, ELU z > 0 ? 1 : exp(z)):
 *                  dz = keep scale act'(z) dy;   dxhat = dz gamma;
 *                  dx = rstd (dxhat - mean_c dxhat - xhat mean_c(dxhat xhat));
 *                  dgamma[c] = sum_t dz xhat;   dbeta[c] = sum_t dz
 *   norm_pool_fwd: x [N, L, D] -> pooled [N, D] = (1 / L) sum_l y[n, l, :] (AMPCONV_POOL_MEAN: one fp32 chain per output
 *                  in ascending l), stats [N L, 2]; or y[n, 0, :] (AMPCONV_POOL_TOKEN0): only token 0 of a node is read
 *                  and normalised, stats [N, 2]
 *   norm_pool_bwd: norm_bwd with dy[n, l, :] = dpooled[n, :] / L (mean) or dpooled[n, :] for l = 0 (token 0: rows l > 0
 *                  of dx are written as exact zeros and only token 0 contributes to dgamma, dbeta)
 * SAVED for backward: x (the layer output, which the model keeps anyway) and stats, 8 bytes per token; nothing else of
 * size [N, L*D].
 * dtype: AMPCONV_F32 or AMPCONV_BF16 = the storage of x, y, dy, dx, pooled, dpooled; gamma, beta, stats, dgamma, dbeta
 * and all arithmetic are fp32.  gamma and beta are both given or both NULL (= 1 and 0); dgamma and dbeta are both given
 * or both NULL (not wanted: nothing is reduced, no workspace is needed) and must be NULL without gamma.  A token is
 * owned by 4..64 lanes of one wave (the smallest power of two that covers the row's 16-byte pieces, at most 4 pieces per
 * lane), read once, reduced by xor butterflies; bases that are not 16-byte aligned or a D that is no whole number of
 * pieces (the XOR toy's D = 3) run element-wise.
 * ERRORS: D outside 1..AMPCONV_NORM_MAX_D, L < 1, negative sizes, eps <= 0, an unknown act or pooling, threshold > 65535,
 * a missing pointer: AMPCONV_E_BADARG; another dtype: AMPCONV_E_DTYPE; workspace_bytes below
 * ampconv_norm_workspace_bytes(T, D) (T = N L for the pooled call) where dgamma is wanted: AMPCONV_E_WORKSPACE --
 * nothing is launched.  T == 0 succeeds and writes dgamma = dbeta = 0.
 * DETERMINISM.  Every output has the same bits on every launch.  dgamma, dbeta: no floating-point atomics -- each
 * workgroup sums its tokens in a fixed order into its own [2, D] slot of `workspace` (need not be zeroed), a second
 * kernel adds the slots in ascending order (16 consecutive runs of slots, then the 16 run sums); the grid depends on
 * (T, D, dtype) only.  */
#define AMPCONV_NORM_MAX_D 1024
size_t ampconv_norm_workspace_bytes(int64_t T, int D);
int ampconv_norm_fwd(const void *x, int64_t T, int D, const float *gamma, const float *beta, float eps, int act,
                     uint64_t seed, uint32_t threshold, float scale, void *y, float *stats, int dtype, void *stream);
int ampconv_norm_bwd(const void *x, const void *dy, const float *stats, int64_t T, int D, const float *gamma,
                     const float *beta, int act, uint64_t seed, uint32_t threshold, float scale, void *dx,
                     float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes, int dtype, void *stream);
int ampconv_norm_pool_fwd(const void *x, int64_t N, int L, int D, const float *gamma, const float *beta, float eps,
                          int act, int pooling, uint64_t seed, uint32_t threshold, float scale, void *pooled,
                          float *stats, int dtype, void *stream);
int ampconv_norm_pool_bwd(const void *x, const void *dpooled, const float *stats, int64_t N, int L, int D,
                          const float *gamma, const float *beta, int act, int pooling, uint64_t seed,
                          uint32_t threshold, float scale, void *dx, float *dgamma, float *dbeta, void *workspace,
                          size_t workspace_bytes, int dtype, void *stream);

/* ---- optimizer step (csrc/optim.hip; pure additions, the ABI number stays 111) ----------------------------------------
 * Reference: every training script runs torch.optim.Adam with L2 weight decay (experiments/cora_benchmark_graphsaint.py:
 * 84-85: lr=0.1, weight_decay=1e-4), most under CosineAnnealingWarmRestarts.  One launch updates a whole parameter group:
 * `t` is a HOST array of n descriptors, one per tensor; all tensors are contiguous fp32 on the device.  At most
 * AMPCONV_ADAM_MAX_TENSORS descriptors travel with one launch, BY VALUE as kernel arguments -- no device table, no
 * host-to-device copy, no synchronisation --; n may be larger: a call issues ceil(n / AMPCONV_ADAM_MAX_TENSORS) launches.
 *   adam_step: per element, all in fp32, with the tensor's step count t (bias corrections computed on the host in double):
 *       c  = norm ? min(1, max_grad_norm / (*norm + 1e-6)) : 1        (torch.nn.utils.clip_grad_norm_; *norm is read ON
 *                                                                       THE DEVICE)
 *       g' = g * grad_scale * c
 *       decoupled == 0:  g' += weight_decay * p                        (torch.optim.Adam)
 *       decoupled == 1:  p  *= 1 - lr * weight_decay                   (torch.optim.AdamW)
 *       m  = m + (1 - beta1) * (g' - m)
 *       v  = beta2 * v + (1 - beta2) * g' * g'
 *       p  = p - step_size * m / (sqrt(v) * inv_bc2_sqrt + eps)
 *     p, m, v are updated in place; g is only read.  The betas are doubles: 1 - beta is formed in double and then
 *     rounded to fp32 (in fp32, 1 - 0.999 is 1.3e-5 off 0.001, which would scale every g' * g').
 *   adam_grad_norm: *norm = sqrt(sum over all n tensors of (g * grad_scale)^2), one fp32 value on the device.
 * MAPPING.  Every tensor is cut into chunks of AMPCONV_ADAM_CHUNK elements, a workgroup per chunk (a chunk never
 * straddles tensors); a tensor whose p, g, m and v are all 16-byte aligned is walked in 16-byte pieces with an
 * element-wise tail, any other tensor element by element.  The grid depends on the numels only.
 * DETERMINISM.  Every output has the same bits on every launch.  The norm: no floating-point atomics -- a lane's squares
 * in ascending order, xor butterflies within a wave, the waves of a workgroup in wave order into the chunk's slot of
 * `workspace` (ampconv_adam_workspace_bytes(t, n); need not be zeroed), and a second kernel adds the slots in ascending
 * order (256 consecutive runs of slots, then the 256 run sums).  Alignment does not change the bits of the norm.
 * ERRORS: n < 0, a NULL t with n > 0, a NULL p, g, m or v with numel > 0, a negative numel, more than 2^31 - 1 chunks,
 * lr < 0, eps <= 0, a beta outside [0, 1), weight_decay < 0, max_grad_norm <= 0 with norm given, or a NULL norm in
 * adam_grad_norm: AMPCONV_E_BADARG; workspace_bytes below ampconv_adam_workspace_bytes(t, n): AMPCONV_E_WORKSPACE --
 * nothing is launched.  n == 0 and tensors with numel == 0 succeed; the norm of nothing is written as 0.  */
#define AMPCONV_ADAM_MAX_TENSORS 24 /* descriptors per launch */
#define AMPCONV_ADAM_CHUNK 1024     /* elements per workgroup */
typedef struct {
  float *p;           /* parameter */
  const float *g;     /* gradient */
  float *m;           /* exp_avg */
  float *v;           /* exp_avg_sq */
  int64_t numel;
  float step_size;    /* lr / (1 - beta1^t) */
  float inv_bc2_sqrt; /* 1 / sqrt(1 - beta2^t) */
} ampconv_adam_tensor_t;
size_t ampconv_adam_workspace_bytes(const ampconv_adam_tensor_t *t, int n);
int ampconv_adam_grad_norm(const ampconv_adam_tensor_t *t, int n, float grad_scale, float *norm, void *workspace,
                           size_t workspace_bytes, void *stream);
int ampconv_adam_step(const ampconv_adam_tensor_t *t, int n, float lr, double beta1, double beta2, float eps,
                      float weight_decay, int decoupled, float grad_scale, const float *norm, float max_grad_norm,
                      void *stream);

/* ---- mixed-precision optimizer step (csrc/optim.hip; pure additions, the ABI number stays 111) -----------------------
 * The step above for parameters stored in bf16 and for gradients of either dtype; descriptors of both dtypes mix freely in
 * one call.  The formulas of "optimizer step" are evaluated in fp32 on the fp32 VALUE of the parameter: `master` for a
 * bf16 p, p itself for an fp32 p.  The gradient is widened to fp32 first (exact); weight decay, decoupled or L2, acts on
 * the fp32 value.  m, v and master are updated in place; a bf16 p is then written as the round-to-nearest-even bf16 of the
 * new master (torch's .to(torch.bfloat16)).  A bf16 update of lr = 1e-3 on a parameter near 1 is below half a bf16 ulp and
 * would be lost every step; the master keeps it.
 * MAPPING.  The chunks, the grid and a lane's elements 4 j .. 4 j + 3 are those of the fp32 step whatever the dtypes; a
 * piece is four elements of its own stream (16 bytes fp32, 8 bytes bf16).  A tensor whose pointers are ALL aligned to
 * their own piece is walked in pieces with an element-wise tail, any other tensor element by element.
 * DETERMINISM.  Every rounding of the step is pinned in the source (csrc/optim.hip, "ROUNDING"): a bf16 gradient gives the
 * norm and the outputs of the same call on its widened fp32 copy; alignment changes no bit; all-fp32 descriptors give the
 * bits of ampconv_adam_grad_norm always and the bits of ampconv_adam_step on every tensor whose p, g, m and v are 16-byte
 * aligned.  (ampconv_adam_step forms the denominator with one rounding in its 16-byte pieces and with two in its
 * element-wise path; the mixed step takes the former for every whole group of four elements and the latter for the up to
 * three elements behind the last one, by position, so it cannot follow ampconv_adam_step on a tensor that is not 16-byte
 * aligned without letting alignment change bits.)
 * ERRORS: everything the fp32 entry points refuse, a dtype code other than AMPCONV_F32 / AMPCONV_BF16, a NULL master with
 * a bf16 p (numel > 0), a non-NULL master with an fp32 p: AMPCONV_E_BADARG -- nothing is launched.  */
typedef struct {
  void *p;            /* parameter, storage p_dtype */
  const void *g;      /* gradient, storage g_dtype (independent of p_dtype) */
  float *m;           /* exp_avg: always fp32 */
  float *v;           /* exp_avg_sq: always fp32 */
  float *master;      /* fp32 copy of p: required when p_dtype == AMPCONV_BF16, NULL when AMPCONV_F32 */
  int64_t numel;
  float step_size;    /* lr / (1 - beta1^t) */
  float inv_bc2_sqrt; /* 1 / sqrt(1 - beta2^t) */
  int32_t p_dtype, g_dtype;
} ampconv_adam_mixed_tensor_t; /* 64 bytes */
size_t ampconv_adam_mixed_workspace_bytes(const ampconv_adam_mixed_tensor_t *t, int n);
int ampconv_adam_mixed_grad_norm(const ampconv_adam_mixed_tensor_t *t, int n, float grad_scale, float *norm,
                                 void *workspace, size_t workspace_bytes, void *stream);
int ampconv_adam_mixed_step(const ampconv_adam_mixed_tensor_t *t, int n, float lr, double beta1, double beta2, float eps,
                            float weight_decay, int decoupled, float grad_scale, const float *norm, float max_grad_norm,
                            void *stream);

/* ---- tensor statistics (csrc/stats.hip; pure additions, the ABI number stays 111) ----------------------------------------
 * Reference: src/ampnet/module/amp_gcn.py:278-405 copies every weight gradient and five [N, L*D] activation tensors to the
 * host and runs seaborn / numpy on them: 30- and 50-bin histograms, mean, median, std, abs().mean(), abs().max().  Here the
 * same numbers come from a few streaming passes over the tensors where they lie; what a caller reads back is a record of
 * 88 bytes, the bin counts and up to four order statistics per tensor.
 * `t` is a HOST array of n descriptors, one per tensor: contiguous fp32 or bf16 (`dtype`: AMPCONV_F32 / AMPCONV_BF16) on the
 * device.  At most AMPCONV_STATS_MAX_TENSORS descriptors travel with one launch, BY VALUE as kernel arguments; n may be
 * larger: a call then repeats its launches per batch of descriptors.  Within a batch the number of launches does not depend
 * on the number of tensors.  Every array argument below (records, range, counts, out) has one row per tensor, row i for
 * t[i].  No call synchronises or copies to the host; `workspace` (ampconv_stats_workspace_bytes(t, n), the same buffer may
 * serve the three calls one after the other on one stream) need not be zeroed.
 * MAPPING.  A tensor is cut into chunks of AMPCONV_STATS_CHUNK elements; it gets min(chunks, 1024) workgroups of 256 lanes,
 * workgroup w walks chunks w, w + workgroups, ...  A lane reads 16-byte pieces where the tensor's base is 16-byte aligned
 * and the piece lies inside it, element by element otherwise -- the element-to-lane assignment is the same either way, so
 * alignment changes no result bit.
 * BITS, NOT COMPARISONS.  The library is compiled with -fno-honor-nans: `x != x`, isnan, fmin and fmax mean nothing on a
 * NaN.  Every element is classified from its bit pattern (bf16 widened to fp32 by a shift) before any floating-point
 * instruction sees it: exponent all ones and mantissa non-zero is a NaN, mantissa zero an infinity.  Only finite elements
 * enter min / max / the sums / the histogram / the selection; min, max and the selection compare the order-preserving
 * unsigned key of the bits (sign bit set: ~bits, else bits | 0x80000000; -0 is first rewritten to +0), absmax compares
 * bits & 0x7fffffff.
 *
 *   stats_moments: one pass, records[i] = ampconv_stats_record_t of tensor i.  zero counts +0 and -0, negative counts
 *     the finite x < 0 (not -0).  min, max, absmax are exact (a bf16 value widened to fp32); with finite == 0 they are NaN.
 *     sum, sum_abs, sum_sq are over the finite elements, in fp64: a lane adds its elements in ascending order, the lanes of
 *     a wave combine in an xor butterfly, the waves in wave order into the workgroup's slot of `workspace`, and a second
 *     launch adds the slots of a tensor in ascending order (256 consecutive runs, then the run sums).  No floating-point
 *     atomics: the same bits on every call.  mean = sum / finite, unbiased variance = (sum_sq - sum * sum / finite) /
 *     (finite - 1) are left to the caller.
 *   stats_histogram: ADDS to counts[i * (bins + 2) + b] (unsigned 64-bit; zero them for a fresh histogram) the number of
 *     finite elements of tensor i in bin b of `bins` (1 .. AMPCONV_STATS_MAX_BINS) equal bins over [lo, hi]; index `bins`
 *     counts the finite x < lo, index bins + 1 the finite x > hi.  (lo, hi) = range[2 i], range[2 i + 1] (device fp32) if
 *     `range` is given, else records[i].min / .max READ ON THE DEVICE -- the pass may follow stats_moments on the stream
 *     with no host round trip.  THE BIN RULE, in fp32 with these roundings and no others (a numpy model reproduces it):
 *         scale = __fdiv_rn((float)bins, __fsub_rn(hi, lo));          hi == lo: every in-range element goes to bin 0
 *         b     = min((int)floorf(__fmul_rn(__fsub_rn(x, lo), scale)), bins - 1)
 *     A range with a NaN, an infinity, hi < lo, or so narrow that bins / (hi - lo) overflows is the caller's error: the
 *     counts are then unspecified (never out of bounds).  Workgroups count in LDS (32-bit) and flush into the 64-bit global
 *     counts with integer atomics, at the latest every 2^31 elements: integer addition commutes, the result does not
 *     depend on the order of arrival.
 *   stats_select: out[i * nq + j] (fp32) = the element of rank floor(q[j] * (finite - 1)) (in fp64, computed ON THE DEVICE
 *     from records[i].finite) among the finite elements of tensor i in ascending order: numpy's quantile method 'lower';
 *     q = 0.5 is rank (finite - 1) / 2, torch.median's lower median.  q: a HOST array of nq (1 .. AMPCONV_STATS_MAX_RANKS)
 *     values in [0, 1].  Radix select on the key above: fp32 in three digit passes (11, 11, 10 bits), bf16 on the 16-bit
 *     key in two (11, 5); a digit pass is the histogram kernel with another binning policy (bin = digit, for the elements
 *     under the prefix chosen so far).  The result is an element of the tensor, bit for bit (-0 reads as +0); nothing is
 *     interpolated.  finite == 0: NaN.
 * These four entry points were added without a change of AMPCONV_VERSION (no existing argument list changed): a binding
 * that declares them fails against an older 111 library at symbol lookup, not at the version check.
 * NO MODE.  amp_gcn.py:297 also shows torch.mode: on continuous data every value is unique and it returns the minimum, on
 * ReLU output it returns 0.  `zero` says the same thing honestly; there is no mode here.
 * ERRORS: n < 0, a NULL t with n > 0, a NULL x with numel > 0, a negative numel, a NULL records / counts / out, bins or nq
 * out of range, a q outside [0, 1]: AMPCONV_E_BADARG; a dtype other than the two: AMPCONV_E_DTYPE; workspace_bytes below the
 * query: AMPCONV_E_WORKSPACE -- nothing is launched.  A failed launch or a failed memset of stats_select's tables comes
 * back as the runtime's own POSITIVE hipError_t, as from every call of this header (conventions at the top; the Python
 * binding's check() raises on any non-zero code).  n == 0 and tensors with numel == 0 succeed (all counts 0).  */
#define AMPCONV_STATS_MAX_TENSORS 24 /* descriptors per launch */
#define AMPCONV_STATS_CHUNK 4096     /* elements one workgroup handles per iteration */
#define AMPCONV_STATS_MAX_BINS 2048
#define AMPCONV_STATS_MAX_RANKS 4
typedef struct {
  const void *x;
  int64_t numel;
  int dtype; /* AMPCONV_F32 or AMPCONV_BF16 */
} ampconv_stats_tensor_t;
typedef struct {
  int64_t numel, finite, nan, inf, zero, negative;
  double sum, sum_abs, sum_sq; /* over the finite elements */
  float min, max, absmax;      /* over the finite elements; NaN if there is none */
  float reserved;
} ampconv_stats_record_t; /* 88 bytes */
size_t ampconv_stats_workspace_bytes(const ampconv_stats_tensor_t *t, int n);
int ampconv_stats_moments(const ampconv_stats_tensor_t *t, int n, ampconv_stats_record_t *records, void *workspace,
                          size_t workspace_bytes, void *stream);
int ampconv_stats_histogram(const ampconv_stats_tensor_t *t, int n, int bins, const float *range,
                            const ampconv_stats_record_t *records, uint64_t *counts, void *stream);
int ampconv_stats_select(const ampconv_stats_tensor_t *t, int n, const double *q, int nq,
                         const ampconv_stats_record_t *records, float *out, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---- GCN baseline (csrc/gcn.hip; pure additions, the ABI number stays 111) -------------------------------------------
 * Reference: the other side of every training script's TRAIN_AMPCONV switch, src/ampnet/module/gcn_classifier.py:17-109:
 * two PyG GCNConv layers behind cat(feature_embedding_table.weight, zscore(x)[n]) per node.  PyG is not a dependency:
 * the semantics below restate PyG 2.0-2.1's gcn_norm / GCNConv and ARE the specification (GCN baseline).
 * fp32 throughout, no floating-point atomics, every sum in a fixed order: every output has the same bits on every launch.
 * (ptr, idx) is a sorted adjacency: segment n = idx[ptr[n] .. ptr[n + 1]) -- the destination-sorted CSR (rowptr, col) for
 * the forward operator, the source-sorted CSC (cscptr, crow) for the transposed one.  fill = 2 (improved) or 1.
 *   gcn_norm:  deg[n] = (entries of segment n with idx != n) + fill   with add_self_loops (every loop in the input is
 *              dropped, one loop of weight fill is added per node), else the segment length;
 *              dinv[n] = deg[n]^-1/2, 0 where deg[n] == 0.  Computed on the CSR; the same dinv serves both directions.
 *   gcn_aggregate:  keep(p) = !add_self_loops || idx[p] != n
 *              out[n, c] = dinv[n] (sum_{p in segment n, keep(p)} dinv[idx[p]] h[idx[p], c]
 *                                   + (add_self_loops ? fill dinv[n] h[n, c] : 0)) + (bias ? bias[c] : 0)
 *              The edge weight dinv[src] w dinv[dst] is symmetric in its two factors, so the transposed operator (the
 *              gradient to h) is the same call on the CSC with bias = NULL; no E-sized weight array exists.
 *              h [N, C] with row stride ld_h >= C, out likewise with ld_out; any C >= 1; columns >= C of a wider buffer
 *              are neither read nor written.  16-byte loads and stores where ld_h and ld_out are multiples of 4 and both
 *              bases are 16-byte aligned, 4-byte ones otherwise (same bits either way).
 *              MAPPING.  A row is owned by 4 edge slots x Q column quads of a wave (Q = the power of two that covers
 *              ceil(C / 4), at most 16: wider rows loop over column chunks), so 64 / (4 Q) rows are in flight per wave
 *              instruction.  A slot adds its entries in ascending order, the slots combine in a fixed xor order.  A segment
 *              of AMPCONV_GCN_LONG_SEGMENT entries or more is not walked by its lanes when `workspace` is given: it is cut
 *              into parts of AMPCONV_GCN_PART entries, a workgroup sums one part (256 / Q slots, ordered LDS combine) into
 *              a partial row, and a last kernel adds a row's partial rows in part order.  workspace NULL (what a caller may
 *              pass when it knows that no segment is long; required size 0 when E < AMPCONV_GCN_LONG_SEGMENT): every
 *              segment is walked by its lane group -- correct for any length, slow for long ones.
 *   gcn_colsum:  out[c] = sum_n g[n, c] (row stride ld): at most 1024 chunks of consecutive rows, each in ascending
 *              order, then the chunks in ascending order (the bias gradient).
 *   gcn_input_fwd / _bwd: the first layer's linear map over the embedded input WITHOUT forming it.  Token f of node n is
 *              cat(table[f, :De], z[n, f]), z = (x - mean) inv_std (the expression of ampconv_feat_build; mean, inv_std of
 *              ampconv_feat_zscore_stats); with W [C, F (De + 1)] viewed as [C, F, De + 1]:
 *                  h[n, j] = sum_f z[n, f] W[j, f, De] + c[j],     c[j] = sum_f sum_k table[f, k] W[j, f, k]
 *              De == 0 with table == NULL is the plain z-scored input (c = 0); mean == inv_std == NULL (De == 0 only)
 *              the raw one, z = x.  mean inv_std is never folded into the weights.  x [N, F] contiguous, h [N, C] with row
 *              stride ld_h.  Backward, from g = dL/dh [N, C] (row stride ld_g) and s[j] = sum_n g[n, j]:
 *                  dW[j, f, De] = sum_n z[n, f] g[n, j]   (at most 64 chunks of rows, ascending inside and across)
 *                  dW[j, f, k < De] = s[j] table[f, k];    dtable[f, k] = sum_j s[j] W[j, f, k]   (ascending j)
 *              dW [C, F (De + 1)] and dtable [F, De] (NULL with De == 0) are written whole.  No gradient to x.
 *              workspace: ampconv_gcn_input_workspace_bytes(N, F, C) bytes, 16-byte aligned, need not be zeroed.
 * ERRORS: a missing pointer, C < 1, a row stride below C, negative sizes, N or E above 2^31 - 1, a pointer that is not
 * 4-byte aligned, a table without De or De without a table or without mean: AMPCONV_E_BADARG; a short or misaligned
 * workspace: AMPCONV_E_WORKSPACE -- nothing is launched.  N == 0 succeeds.  */
#define AMPCONV_GCN_LONG_SEGMENT 256
#define AMPCONV_GCN_PART 2048
int ampconv_gcn_norm(const int32_t *ptr, const int32_t *idx, int64_t N, int add_self_loops, float fill, float *dinv,
                     void *stream);
size_t ampconv_gcn_aggregate_workspace_bytes(int64_t N, int64_t E, int C);
int ampconv_gcn_aggregate(const float *h, int64_t ld_h, int C, const int32_t *ptr, const int32_t *idx,
                          const float *dinv, int add_self_loops, float fill, const float *bias, float *out,
                          int64_t ld_out, int64_t N, int64_t E, void *workspace, size_t workspace_bytes, void *stream);
size_t ampconv_gcn_colsum_workspace_bytes(int64_t N, int C);
int ampconv_gcn_colsum(const float *g, int64_t ld, int64_t N, int C, float *out, void *workspace,
                       size_t workspace_bytes, void *stream);
size_t ampconv_gcn_input_workspace_bytes(int64_t N, int64_t F, int C);
int ampconv_gcn_input_fwd(const float *x, int64_t N, int64_t F, const float *mean, const float *inv_std, const float *W,
                          const float *table, int De, int C, float *h, int64_t ld_h, void *workspace,
                          size_t workspace_bytes, void *stream);
int ampconv_gcn_input_bwd(const float *x, int64_t N, int64_t F, const float *mean, const float *inv_std, const float *W,
                          const float *table, int De, int C, const float *g, int64_t ld_g, float *dW, float *dtable,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- pair loss ----------------------------------------------------------------
 * The unsupervised GraphSAGE loss the reference announces and leaves empty (synthetic_benchmark/contrastive_ssl_AMPNet.py
 * and predictive_ssl_AMPNet.py:79, `criterion = None  # Implement GraphSAGE unsupervised loss function`, with the
 * TensorFlow affinity / neg_cost / _skipgram_loss it means quoted at :14-49), over (anchor, positive, negatives) triples
 * of node embeddings.  Added without a version change, like the entry points of 111 before it: no existing argument list
 * changes.
 *   Z [N, D] fp32 or bf16 (`dtype`), row stride ldz >= D elements, 1 <= D <= AMPCONV_PAIR_MAX_D (odd D included);
 *   anchor[B], positive[B], negative[S] int64 node ids; weight[B] fp32 or NULL (1; no gradient flows to it);
 *   scale: a temperature's reciprocal; neg_weight: used by AMPCONV_PAIR_XENT only; exclude_anchor: 0 or 1.
 * With a_b = Z[anchor[b]], p_b = Z[positive[b]], n_s = Z[negative[s]]:
 *   aff_b = scale <a_b, p_b>,   g_bs = scale <a_b, n_s>;
 *   a pair (b, s) is KEPT unless exclude_anchor is set and negative[s] == anchor[b] (compared on the clamped ids);
 *   AMPCONV_PAIR_SKIPGRAM: l_b = log sum_{kept s} exp(g_bs) - aff_b.  This is the quoted _skipgram_loss NEGATED: as quoted,
 *       sum(aff - neg_cost) is a quantity to maximise; the library returns what an optimizer minimises.  A row with no
 *       kept negative has a negative term of 0.
 *   AMPCONV_PAIR_XENT:     l_b = softplus(-aff_b) + neg_weight sum_{kept s} softplus(g_bs)   (GraphSAGE's _xent_loss);
 *   loss = sum_b weight_b l_b.  B = 0: loss 0 and zero gradients.
 * Gradient for the upstream scalar g0 (read from the device, `gout`), with pi_bs = the softmax over the kept s
 * (skipgram) or neg_weight sigmoid(g_bs) (xent), c_b = -1 (skipgram) or -sigmoid(-aff_b) (xent):
 *   dZ[anchor[b]]   += g0 w_b scale (sum_s pi_bs n_s + c_b p_b)
 *   dZ[positive[b]] += g0 w_b scale c_b a_b
 *   dZ[negative[s]] += g0 scale sum_b w_b pi_bs a_b
 * A node may hold all three roles and repeat in each list; dZ sums every contribution.
 * FORWARD writes aff[B], neg_term[B] (the kept log-sum-exp, or the softplus sum), the scalar loss (a device float) and
 * `oob` (device int32): non-zero if any id lies outside [0, N).  Such ids are clamped on their int64 value before any
 * address is formed -- v < 0 -> 0, v >= N -> N - 1, as ampconv_csr_build does -- and the result is that of the clamped
 * ids.  The [B, S] logits are tiled on chip and never written; rows of Z are read through the index arrays (no gathered
 * copies); the log-sum-exp is online (running maximum and sum), so no exponential overflows at any logit.  Where B alone
 * does not fill the card the S range is split over workgroups and the partial (max, sum) pairs merge in split order.
 * BACKWARD recomputes the logits from Z, aff and neg_term in two atomic-free passes -- over anchor tiles (pi N; the
 * positive role falls out of it) and over negative tiles (pi^T A) -- into dense fp32 role gradients in the workspace
 * (rows padded to a multiple of 4 floats; the streamed side split as above, one partial per split), then folds them into
 * dZ [N, D] (row stride lddz, Z's dtype) per node, in the order of the caller's node-sorted slot list: slot b < B is
 * anchor b, B + b positive b, 2 B + s negative s; slot_idx[2 B + S] holds the slots sorted (stably) by clamped node id and
 * slot_ptr[N + 1] the segment of every node.  dZ is written in full, +0 for the nodes without a role.  Slots and segment
 * bounds are clamped, so a malformed list cannot fault.  Loss and dZ are bitwise reproducible: no floating-point atomics.
 * Products on v_mfma_f32_16x16x4_f32 (exact fp32; bf16 rows widened on load), K zero-padded.
 * workspace: ampconv_pair_loss_workspace_bytes(B, S, D) bytes (covers either direction), 256-byte aligned, not zeroed.
 * REFUSED with AMPCONV_E_BADARG, nothing launched or written: D outside [1, AMPCONV_PAIR_MAX_D], ldz < D (lddz < D),
 * S < 1 or N < 1 with B > 0, a NULL Z or index pointer with B > 0, a NULL output, an unknown kind or dtype, N above
 * 2^31 - 1, B or S above 2^29; AMPCONV_E_WORKSPACE: a short workspace.  */
#define AMPCONV_PAIR_MAX_D 256
enum { AMPCONV_PAIR_SKIPGRAM = 0, AMPCONV_PAIR_XENT = 1 };
size_t ampconv_pair_loss_workspace_bytes(int64_t B, int64_t S, int D);
int ampconv_pair_loss_fwd(const void *Z, int64_t N, int D, int64_t ldz, const int64_t *anchor, const int64_t *positive,
                          int64_t B, const int64_t *negative, int64_t S, const float *weight, int kind, float scale,
                          float neg_weight, int exclude_anchor, float *aff, float *neg_term, float *loss, int32_t *oob,
                          void *workspace, size_t workspace_bytes, int dtype, void *stream);
int ampconv_pair_loss_bwd(const void *Z, int64_t N, int D, int64_t ldz, const int64_t *anchor, const int64_t *positive,
                          int64_t B, const int64_t *negative, int64_t S, const float *weight, int kind, float scale,
                          float neg_weight, int exclude_anchor, const float *aff, const float *neg_term,
                          const float *gout, const int32_t *slot_ptr, const int32_t *slot_idx, void *dZ, int64_t lddz,
                          void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ---- nearest neighbours -------------------------------------------------------
 * The k best keys of every query among the rows of one node matrix: what a trained embedding is used for (nearest-
 * neighbour evaluation, ampnet_amd.knn_classify) and what the reference's synthetic benchmark builds its graphs with
 * (synthetic_benchmark/synthetic_xor.py:69-101, scikit-learn's NearestNeighbors, ampnet_amd.knn_graph).  Added without
 * a version change, like the pair loss: no existing argument list changes.
 *   X [N, D] fp32 or bf16 (`dtype`), row stride ldx >= D elements, 1 <= D <= AMPCONV_KNN_MAX_D (odd D included);
 *   query[Q], key[S] int64 node ids, or NULL: the list is every node in order (its count must then be N; a count of 0
 *   is taken with either); 1 <= k <= AMPCONV_KNN_MAX_K; N, Q, S <= 2^31 - 1; exclude_self: 0 or 1.
 * Ids outside [0, N) are clamped on their int64 value before any address is formed -- v < 0 -> 0, v >= N -> N - 1, as
 * ampconv_pair_loss_fwd and ampconv_csr_build do --, set *oob (device int32) non-zero, and the result is that of the
 * clamped ids; *oob is 0 otherwise.
 * GOODNESS g of the pair (q, s), with a = X[query[q]], b = X[key[s]], products and sums in fp32 (bf16 rows widened on
 * load), <a, b> on v_mfma_f32_16x16x4_f32 (exact fp32), K zero-padded:
 *   AMPCONV_KNN_DOT:    g = <a, b>;
 *   AMPCONV_KNN_COSINE: g = (<a, b> r_a) r_b,  r = 1 / max(sqrt(sum of squares), 1e-12)  (torch.nn.functional.normalize's
 *                       epsilon);
 *   AMPCONV_KNN_L2:     d2 = max(fma(-2, <a, b>, |a|^2 + |b|^2), 0),  g = -d2.  This is the EXPANSION, not a sum of squared
 *                       differences: its absolute error is of the order of 2^-24 (|a|^2 + |b|^2) however close the two
 *                       rows are.
 *   r and |x|^2 are one fp32 value per node, summed in one fixed order per row by a pre-pass into the workspace.
 * `score` holds g for DOT and COSINE, descending along a row, and d2 for L2, ascending.
 * SELECTION.  The pair (q, s) is a CANDIDATE unless exclude_self is set and the clamped key id equals the clamped query
 * id, or its g is NaN (for L2: the value before the max is NaN).  Candidates are totally ordered by (g descending,
 * s ascending); s is the POSITION in the key list, not the node id; -0 counts as +0; +-infinity are ordinary values.
 * Row q of the output is the first min(k, #candidates) of its candidates in that order: idx [Q, k] (row stride k) holds
 * their node ids (the clamped key[s], or s), score [Q, k] their scores.  The slots behind them hold idx = -1 and score =
 * -infinity (DOT, COSINE) or +infinity (L2).
 * The order is one unsigned compare of a 64-bit key: high word = the image of g's bits u (0x80000000 first replaced by 0)
 * under u -> ~u if the sign bit is set, else u | 0x80000000; low word = ~s.  Key 0 is no candidate (-infinity maps to
 * 0x007FFFFF).
 * DETERMINISM.  The order is strict and a pair's g does not depend on where the pair falls in a tile, so the result does
 * not depend on tile order, on how the key range is split over workgroups, on Q, or on the other queries of the call:
 * two calls give bitwise-equal idx and score, and row q of a call over a query subset equals bitwise that node's row of
 * the all-rows call.  No atomics.
 * The [Q, S] scores are tiled on chip and never written; the best k of a row are kept in LDS.  Where Q alone does not
 * fill the card the key range is split over workgroups, each split writes its k keys per row to the workspace and a
 * merge takes the best k of a row's partials.
 * workspace: ampconv_knn_workspace_bytes(Q, S, N, D, k) bytes (non-decreasing in every argument), 256-byte aligned, not
 * zeroed.
 * REFUSED with AMPCONV_E_BADARG, nothing launched or written: D outside [1, AMPCONV_KNN_MAX_D], k outside
 * [1, AMPCONV_KNN_MAX_K], ldx < D, a NULL X, idx, score or oob or N < 1 with Q > 0, a NULL id list whose count is
 * neither N nor 0, an unknown metric or dtype, a negative N, Q or S or one above 2^31 - 1; AMPCONV_E_WORKSPACE: a
 * NULL or short workspace.  Q == 0 succeeds and writes only *oob = 0 (if oob is given); S == 0 fills Q rows of empty
 * slots.  */
#define AMPCONV_KNN_MAX_D 256
#define AMPCONV_KNN_MAX_K 64
enum { AMPCONV_KNN_DOT = 0, AMPCONV_KNN_COSINE = 1, AMPCONV_KNN_L2 = 2 };
size_t ampconv_knn_workspace_bytes(int64_t Q, int64_t S, int64_t N, int D, int k);
int ampconv_knn(const void *X, int64_t N, int D, int64_t ldx,
                const int64_t *query, int64_t Q,      /* node ids, or NULL: Q == N, query q is node q */
                const int64_t *key, int64_t S,        /* node ids, or NULL: S == N, key s is node s   */
                int k, int metric, int exclude_self,
                int64_t *idx, float *score,           /* [Q, k] each, row stride k */
                int32_t *oob, void *workspace, size_t workspace_bytes, int dtype, void *stream);

/* ---- principal components -------------------------------------------------------
 * The kernels under ampnet_amd.pca (csrc/pca.hip): the reference's sklearn.decomposition.PCA -- the PCA featuriser
 * (src/ampnet/module/amp_gcn.py:185-237, fit_transform(x.T)), the explained-variance curve and the 2-D plot
 * (visualization/plot_PCA_2D_plot.py).  Added without a version change: no existing argument list changes.
 *
 * WHAT ampnet_amd.pca COMPUTES is sklearn's PCA(n_components=k, svd_solver='full') of the data X [M, P]:
 *   samples='rows':    X = x (embeddings [N, D]);   samples='columns': X = x^T, never formed (the reference's
 *   fit_transform(x.transpose()): the samples are the F feature columns).
 *   mean [P] = the per-column mean of X over the M samples; Xc = X - mean = U S Vt;
 *   components = Vt[:k], scores = U[:, :k] S[:k], singular_values = S[:k],
 *   explained_variance = S^2 / (M - 1), explained_variance_ratio = S^2 / (sum of all S^2), 0 where that sum is 0.
 *   Sign: every component is flipped so that its largest-magnitude entry is positive, the first such entry on a tie
 *   (scikit-learn >= 1.5, svd_flip(u_based_decision=False)); the scores flip with it.
 *   Domain: x [R, W] fp32 or bf16, W <= AMPCONV_PCA_MAX_W, row stride ldx >= W; 2 <= M; 1 <= k <= min(M, P,
 *   AMPCONV_PCA_MAX_K).
 *   Rank-deficient directions: where S_j <= S_1 max(M, P) 2^-23, a vector that has to be recovered by a division by
 *   S_j is written as zeros; S_j itself is reported, clamped at 0.
 * Whatever `samples` is, the W x W matrix is Sm = A^T A contracted over the stored rows of x:
 *   'rows':    A[n, w] = x[n, w] - mean[w] (a column shift); Sm is the scatter matrix, its eigenvectors are the
 *              components and the scores are a projection;
 *   'columns': A[n, f] = x[n, f] - mean[n] (a row shift); Sm is the Gram matrix of the samples, eigenvectors sqrt(lambda)
 *              are the scores and the components [k, N] a projection divided by S_j.
 * The eigen-decomposition of Sm (fp64, W x W) is the caller's.
 *
 * Common to the three calls: x [R, W] fp32 or bf16 (`dtype`, bf16 widened on load), 1 <= R <= 2^31 - 1,
 * 1 <= W <= AMPCONV_PCA_MAX_W, ldx >= W; anything else, a NULL x or output: AMPCONV_E_BADARG, nothing launched.  No
 * atomics: two calls give bitwise-equal results.
 *
 * ampconv_pca_shift: out[w] = the mean of column w over the R rows (axis 0, out [W]) or out[r] = the mean of row r
 * over the W columns (axis 1, out [R]): summed in fp64 in one fixed order, divided in fp64, written as fp32.  Axis 0
 * is a two-level reduction: chunks of rows (at most 512, from R alone) into fp64 partial sums in the workspace
 * (ampconv_pca_shift_workspace_bytes, 0 for axis 1), then the chunks in order.
 *
 * ampconv_pca_gram: Sm [W, W] fp64, row stride W, Sm[i][j] = sum over n of A[n, i] A[n, j] with
 *   A[n, w] = (fp32(x[n, w]) - row_shift[n]) - col_shift[w]  in fp32; a NULL shift is no subtraction, so with one
 *   shift given the element is rounded once.
 * Products are exact fp32 on v_mfma_f32_16x16x4_f32, summed in fp32 over a run of at most AMPCONV_PCA_RUN rows; the
 * runs are added in fp64.  The rows are split over workgroups -- ampconv_pca_gram_splits(R, W) splits, from the shape
 * alone, their fp64 partials in the workspace (at most 64 MiB from the second split on) -- and a second launch adds
 * the splits in order.  Only the tiles on and above the diagonal are computed; Sm[j][i] is written from Sm[i][j]: the
 * result is exactly symmetric.  |Sm - exact| <= (AMPCONV_PCA_RUN + 2) 2^-24 (|A|^T |A|) elementwise.
 * AMPCONV_E_WORKSPACE: a NULL workspace or one shorter than ampconv_pca_gram_workspace_bytes(R, W).
 *
 * ampconv_pca_project: out[r, j] = scale[j] * sum over w of A[r, w] V[w, j], j < k, with A as above; V [W, k] fp32,
 * row stride k; scale [k] or NULL (1 / S_j, or 0 for a rank-deficient direction); out fp32 [R, k], row stride
 * ldo >= k; 1 <= k <= AMPCONV_PCA_MAX_K.  The same MFMA, fp32 sums over all of W:
 * |out - exact| <= (W + 2) 2^-24 |scale| (|A| |V|).  */
#define AMPCONV_PCA_RUN 32
#define AMPCONV_PCA_MAX_W 2048
#define AMPCONV_PCA_MAX_K 128
size_t ampconv_pca_shift_workspace_bytes(int64_t R, int W, int axis);
int ampconv_pca_shift(const void *x, int64_t R, int W, int64_t ldx, int axis, float *out, void *workspace,
                      size_t workspace_bytes, int dtype, void *stream);
int ampconv_pca_gram_splits(int64_t R, int W);
size_t ampconv_pca_gram_workspace_bytes(int64_t R, int W);
int ampconv_pca_gram(const void *x, int64_t R, int W, int64_t ldx, const float *row_shift, const float *col_shift,
                     double *Sm, void *workspace, size_t workspace_bytes, int dtype, void *stream);
int ampconv_pca_project(const void *x, int64_t R, int W, int64_t ldx, const float *row_shift, const float *col_shift,
                        const float *V, int k, const float *scale, float *out, int64_t ldo, int dtype, void *stream);

/* ---- t-SNE ------------------------------------------------------------------------
 * The kernels under ampnet_amd.tsne (csrc/tsne.hip): the reference's visualization/plot_TSNE_2D_plot.py,
 * TSNE(n_components=2, perplexity=10, learning_rate=10).fit_transform(x.T).  Added without a version change: no
 * existing argument list changes.
 *
 * WHAT ampnet_amd.tsne COMPUTES is scikit-learn 1.7.2's TSNE(method='barnes_hut') with the repulsive term summed
 * exactly (what its own code computes at angle = 0), for TWO output dimensions only: one degree of freedom,
 * q_ij = 1 / (1 + |y_i - y_j|^2).
 *   neighbours: the k = min(M - 1, int(3 perplexity + 1)) nearest other samples by squared Euclidean distance;
 *   conditional affinities p_{j|i} over those k by the perplexity search below (_utils._binary_search_perplexity);
 *   P = (p + p^T) / max(sum, 2^-52) as a CSR, indices ascending within a row, a pair that is a neighbour both ways once
 *   with the summed value, a pair whose fp64 sum is exactly 0 not at all (_t_sne._joint_probabilities_nn, scipy's
 *   P + P.T); values float32, as _kl_divergence_bh reads them;
 *   gradient_i = 4 (sum_j P_ij q_ij (y_i - y_j)  -  sum_{j != i} q_ij^2 (y_i - y_j) / max(Z, 2^-52)),
 *   Z = sum_{i != j} q_ij (_kl_divergence_bh); error = sum_ij P_ij log(max(P_ij, FLT_MIN) / max(q_ij / Z, FLT_MIN));
 *   the update is _gradient_descent's: gains += 0.2 where update * gradient < 0, else gains *= 0.8, clipped below at
 *   min_gain = 0.01; gradient *= gains; update = momentum update - learning_rate gradient; y += update; 250 iterations
 *   at momentum 0.5 on early_exaggeration P, the rest at 0.8 on P with update and gains reset; error and gradient norm
 *   every 50 iterations and at the last, with scikit-learn's two stopping rules.
 * Where this differs from scikit-learn: j = i is excluded BY INDEX, so another point that coincides with y_i adds
 * q = 1 to Z and no force; scikit-learn's tree skips every point at distance 0.  Embeddings without coincident points
 * (any that has left the 1e-4-scaled start) see no difference.  The start is exact PCA, so nothing is random.
 *
 * ampconv_tsne_affinities: dist2 [N, K] fp32 (row stride ldd >= K), 1 <= K <= AMPCONV_TSNE_MAX_K; P [N, K] fp32 (row
 * stride K) and beta [N] fp64.  Per row, in fp64: beta = 1, the bounds infinite; at most 100 times
 *   p_j = exp(-dist2_j beta), s = sum p_j (s = 1e-8f if it is 0), p_j /= s, H = log(s) + beta sum dist2_j p_j;
 *   stop if |H - log(perplexity)| <= 1e-5f; H too large: lower bound = beta, beta doubles while the upper bound is
 *   infinite, else the midpoint; H too small: upper bound = beta, beta halves while the lower bound is infinite, else
 *   the midpoint.
 * P = fp32(p), except that a p that is positive in fp64 and rounds to 0 is written as the smallest fp32 denormal (bits
 * 0x00000001): whether a pair is an entry of the joint P is decided by p != 0 in fp64, as scipy's P + P.T decides it, and
 * the consumer reads that off the BITS of P.  beta = the value p was evaluated at.  Every one of the K columns takes part (scikit-learn's K < N
 * case).  1e-5f, 1e-8f and the perplexity are float32 values widened, as in scikit-learn.  One wave per row; the two
 * sums are butterflies over the lanes, so they differ from a sequential sum by fp64 rounding only.
 *
 * ampconv_tsne_repulsion: y [N, 2] fp32 dense, 8-byte aligned; neg_f [N, 2] fp32, neg_f[i] = sum_{j != i} q_ij^2 (y_i - y_j)
 * and *Z fp64 (device).  Pair arithmetic is fp32 (y_i - y_j, two FMAs for 1 + d^2, v_rcp_f32: 1 ulp).  For row i the
 * three sums run over the keys j in ascending order in fp32 for a run of AMPCONV_TSNE_RUN keys (runs start at
 * multiples of it), the runs of a chunk are added in order in fp64, the chunks in order in fp64, neg_f is rounded
 * once.  A chunk is AMPCONV_TSNE_CHUNK ceil(ceil(N / AMPCONV_TSNE_CHUNK) / 64) keys: a function of N alone, so is the
 * launch, and the entry point exposes no split.  Z: the rows' fp64 sums, 256 consecutive rows by a binary tree
 * (s[t] += s[t + o], o = 128 .. 1), those sums by lane t adding t, t + 256, ... and the same tree.  No atomics: two
 * calls give the same bits.  |neg_f - exact| <= (AMPCONV_TSNE_RUN + 16) 2^-24 sum_j |q_ij^2 (y_i - y_j)| per
 * coordinate and |Z_i - exact| <= (AMPCONV_TSNE_RUN + 8) 2^-24 Z_i per row.
 * Workspace: ampconv_tsne_repulsion_workspace_bytes(N), 8-byte aligned: the chunks' fp64 sums [chunk][3][N], i.e.
 * 24 bytes x chunks x N with chunks = ceil(N / chunk length) <= 64, plus 8 bytes per 256 rows.  It grows with N^2 up
 * to 262 144 points and linearly beyond: 55 MB at 96 000 points (24 chunks), 403 MB at 262 144 (64 chunks), 1.5 GB at
 * a million, 25.8 GB at AMPCONV_TSNE_MAX_N -- the limit of the index arithmetic, not a size the workspace makes cheap.
 *
 * ampconv_tsne_step: one iteration.  y_in, y_out (a different buffer: rows read their neighbours' y_in), update, gains,
 * neg_f [N, 2] fp32 dense and 8-byte aligned, update and gains updated in place; the CSR of P (indptr [N + 1], indices
 * [nnz] int64, val [nnz] fp32; a column outside [0, N) is clamped, positions outside [0, nnz] likewise); *Z fp64 as
 * ampconv_tsne_repulsion left it.  Per row i, with p = exaggeration val in fp32 and q as above:
 *   pos = sum over the row of (p q) (y_i - y_j): lane l of a wave adds the entries l, l + 64, ... in fp32, a butterfly
 *   adds the lanes; a row longer than AMPCONV_TSNE_PART entries is cut into parts of that length from its start, each
 *   summed this way, the parts added in order in fp64;
 *   grad = 4 fp32(pos - neg_f / max(Z, 2^-52)) (the difference in fp64), then the fp32 statements above.
 * error (NULL: not computed): error[0] = sum of p log(max(p, FLT_MIN) / max(fp32(q / Z), FLT_MIN)) (terms and row sums
 * in fp32 in the order of pos, rows in fp64), error[1] = sum over the elements of (gains grad)^2 (fp64); both over the
 * rows by lane t adding t, t + 256, ... and the tree above.
 * Workspace: ampconv_tsne_step_workspace_bytes(N, nnz), 8-byte aligned.
 * AMPCONV_E_BADARG (nothing launched): a NULL or misaligned pointer, y_in == y_out, N outside [1, AMPCONV_TSNE_MAX_N],
 * K outside its range, perplexity <= 0.  AMPCONV_E_WORKSPACE: a NULL or short workspace.  */
#define AMPCONV_TSNE_MAX_K 256
#define AMPCONV_TSNE_MAX_N (1 << 24)
#define AMPCONV_TSNE_RUN 256
#define AMPCONV_TSNE_TILE 1024
#define AMPCONV_TSNE_CHUNK 4096
#define AMPCONV_TSNE_PART 1024
int ampconv_tsne_affinities(const float *dist2, int64_t N, int K, int64_t ldd, float perplexity, float *P, double *beta,
                            void *stream);
size_t ampconv_tsne_repulsion_workspace_bytes(int64_t N);
int ampconv_tsne_repulsion(const float *y, int64_t N, float *neg_f, double *Z, void *workspace, size_t workspace_bytes,
                           void *stream);
size_t ampconv_tsne_step_workspace_bytes(int64_t N, int64_t nnz);
int ampconv_tsne_step(const float *y_in, float *y_out, float *update, float *gains, int64_t N, const int64_t *indptr,
                      const int64_t *indices, const float *val, int64_t nnz, const float *neg_f, const double *Z,
                      float exaggeration, float momentum, float learning_rate, float min_gain, double *error,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- UMAP -------------------------------------------------------------------------
 * The kernels under ampnet_amd.umap (csrc/umap.hip): the reference's visualization/UMAP_testing.ipynb,
 * umap.UMAP(n_neighbors=15, n_components=2, min_dist=0.1, metric='euclidean').fit_transform(x), and its UMAP featuriser
 * (src/ampnet/utils/preprocess.py: n_components=30 on x.T).  Added without a version change: no existing argument list
 * changes.
 *
 * WHAT ampnet_amd.umap COMPUTES.  This text and the fp64 model in tests/umap_reference.py ARE the specification: the
 * semantics are umap-learn 0.5's defaults (metric='euclidean', set_op_mix_ratio=1, local_connectivity=1, spread=1,
 * repulsion_strength gamma = 1, negative_sample_rate=5, initial_alpha=1), restated here because umap-learn is not a
 * dependency; PARITY WITH umap-learn's BITS IS UNPINNED, and two things differ on purpose: the epoch is synchronous
 * (below) and the start is PCA, not spectral.
 *   neighbours: k = n_neighbors columns per sample, column 0 the sample itself at distance 0, columns 1 .. k - 1 its
 *   k - 1 nearest other samples as Euclidean distances (float32 sqrt of the squared ones), nearest first;
 *   2 <= k <= min(M, AMPCONV_UMAP_MAX_K).
 *   calibration (smooth_knn_dist), per row in fp64: target = log2(k); rho = the smallest distance of the row that is
 *   > 0, or 0; lo = 0, hi = inf, mid = 1, at most 64 rounds of
 *     psum = sum_{j = 1 .. k-1} (d_j - rho > 0 ? exp(-(d_j - rho) / mid) : 1);  stop if |psum - target| < 1e-5;
 *     psum > target: hi = mid, mid = (lo + hi) / 2;  else lo = mid, mid = 2 mid while hi is infinite, else (lo + hi) / 2;
 *   sigma = mid, floored: rho > 0: sigma = max(sigma, 1e-3 x the mean of the row's k distances, column 0 included);
 *   rho = 0: sigma = max(sigma, 1e-3 x the mean of all M k distances).
 *   memberships (float32 [M, k]): 0 where the neighbour is the row itself; 1 where d - rho <= 0 or sigma = 0; else
 *   exp(-(d - rho) / sigma), evaluated in fp64 and rounded once.
 *   fuzzy union: the CSR of W = P + P^T - P o P^T for P[i, idx[i, j]] = membership[i, j]: indices ascend within a
 *   row, exact zeros are no entries, each value is (p + q) - p q in float32 from the two float32 memberships (a missing
 *   one is 0): the expression is symmetric in p and q, so W[i, j] and W[j, i] are THE SAME BITS.
 *   curve: (a, b) = the least-squares fit of 1 / (1 + a x^(2b)) to y(x) = 1 for x < min_dist, else
 *   exp(-(x - min_dist) / spread), on x = linspace(0, 3 spread, 300) (a ~ 1.5769, b ~ 0.8951 for the defaults).
 *   schedule: n_epochs defaults to 500 for M <= 10000, else 200; entries with w < max(w) / n_epochs are dropped (float32
 *   division); per remaining DIRECTED entry e (its position in the CSR) eps_e = max(w) / w_e (float32) and the state
 *   next_e = eps_e, nextneg_e = eps_e / 5 (float32), drawn_e = 0 (int32).
 *   epoch n (SYNCHRONOUS: reads Y_in, writes Y_out, alpha = 1 - n / n_epochs): entry e = (j -> k) FIRES if next_e <= n.
 *     attraction: d2 = |Y_j - Y_k|^2, c = d2 > 0 ? -2 a b d2^(b-1) / (a d2^b + 1) : 0, g = clip(c (Y_j - Y_k), +-4) per
 *     coordinate; row j receives 2 g alpha.  The factor 2 is umap-learn's move_other: the mirrored entry (k -> j) has
 *     the same weight bits, hence the same eps and firing history, and with the positions frozen for the epoch its
 *     update of its tail is exactly this g -- so every row gathers over its own CSR row, nothing is scattered and
 *     there are no atomics.  umap-learn's loop is sequential (or Hogwild) and in place; this one is not.
 *     then next_e += eps_e; epn = eps_e / 5; m = int((n - nextneg_e) / epn), clamped to [0, AMPCONV_UMAP_MAX_NEGATIVES]
 *     (float32 subtraction and IEEE division, truncated); for p < m: s = draw(seed, e, drawn_e + p) % M with
 *     draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b)) (uint64, wrapping: the library's stream),
 *     d2 = |Y_j - Y_s|^2, c = d2 > 0 ? 2 gamma b / ((0.001 + d2) (a d2^b + 1)) : 0, row j receives
 *     clip(c (Y_j - Y_s), +-4) alpha (nothing if c = 0); then drawn_e += m, nextneg_e += m epn (the product rounded to
 *     float32, then the sum).  Firing decisions, m and the drawn ids are integer-exact.
 *   start: PCA scores (there is NO spectral start) or a given [M, n_components] tensor, every column mapped to [0, 10]:
 *   10 (y - min) / (max - min), as umap-learn does before its optimiser.
 *
 * ampconv_umap_memberships: idx [M, k] int64 (row stride ldi >= k) and dist [M, k] fp32 (row stride ldd >= k), both
 * read in place; memb [M, k] fp32 (row stride k), sigma and rho [M] fp64.  One wave per row; psum and the row's sum
 * are butterflies over the lanes, the sum of all distances is the rows' sums added by lane t taking t, t + 256, ...
 * and a binary tree (s[t] += s[t + o], o = 128 .. 1): fixed orders, two calls give the same bits, and they differ from
 * sequential sums by fp64 rounding only.  Workspace: ampconv_umap_memberships_workspace_bytes(M), 8-byte aligned.
 *
 * ampconv_umap_epoch: one epoch, one launch sequence, nothing read back.  y_in, y_out [M, dim] fp32 dense and 8-byte
 * aligned, different buffers; 2 <= dim <= AMPCONV_UMAP_MAX_DIM (dim = 2 has its own instantiation with 8-byte loads);
 * the CSR (indptr [M + 1], indices [nnz] int64; a column outside [0, M) is clamped, positions outside [0, nnz] likewise)
 * with eps [nnz] fp32 and the state next, nextneg [nnz] fp32, drawn [nnz] int32 updated in place.  d2 by FMAs over the
 * coordinates in order, d2^b = exp2(b log2(d2)) in fp32, one division per coefficient (ampconv_umap_coefficients
 * evaluates exactly these two functions on an array of d2, for measuring their error).  The sum of a row: the row is
 * cut into groups of 64 entries from its start; lane l of a wave adds entry l's attraction, then its negatives in
 * order, in fp32 (FMAs with alpha); a butterfly adds the lanes; the groups are added in order in fp64 and
 * y_out = fp32(y_in + sum) with the addition in fp64.  A row longer than AMPCONV_UMAP_PART entries is cut into parts
 * of that length whose groups separate waves compute and store; the order of the additions is the same, so THE RESULT
 * DOES NOT DEPEND ON THE PART LENGTH -- ampconv_umap_epoch_split takes it as an argument (a multiple of 64 in
 * [64, 2^24]) for tests to show that.  Workspace: ampconv_umap_epoch_workspace_bytes(M, nnz, dim), 8-byte aligned:
 * (nnz / 64 + M + 1) dim floats; nothing of size M^2 exists.
 * AMPCONV_E_BADARG (nothing launched): a NULL or misaligned pointer, y_in == y_out, M outside [2, AMPCONV_UMAP_MAX_M]
 * (the epoch takes M = 1), k outside [2, min(M, AMPCONV_UMAP_MAX_K)], a stride below k, dim or part out of range,
 * epoch outside [0, 2^24].  AMPCONV_E_WORKSPACE: a NULL or short workspace.  */
#define AMPCONV_UMAP_MAX_K 256
#define AMPCONV_UMAP_MAX_M (1 << 24)
#define AMPCONV_UMAP_MAX_DIM 32
#define AMPCONV_UMAP_PART 1024
#define AMPCONV_UMAP_MAX_NEGATIVES 65536
size_t ampconv_umap_memberships_workspace_bytes(int64_t M);
int ampconv_umap_memberships(const int64_t *idx, int64_t ldi, const float *dist, int64_t ldd, int64_t M, int k, float *memb,
                             double *sigma, double *rho, void *workspace, size_t workspace_bytes, void *stream);
int ampconv_umap_coefficients(const float *d2, int64_t n, float a, float b, float gamma, float *attract, float *repel,
                              void *stream);
size_t ampconv_umap_epoch_workspace_bytes(int64_t M, int64_t nnz, int dim);
int ampconv_umap_epoch(const float *y_in, float *y_out, int64_t M, int dim, const int64_t *indptr, const int64_t *indices,
                       int64_t nnz, const float *eps, float *next, float *nextneg, int32_t *drawn, float a, float b,
                       float gamma, float alpha, int epoch, uint64_t seed, void *workspace, size_t workspace_bytes,
                       void *stream);
int ampconv_umap_epoch_split(const float *y_in, float *y_out, int64_t M, int dim, const int64_t *indptr,
                             const int64_t *indices, int64_t nnz, const float *eps, float *next, float *nextneg,
                             int32_t *drawn, float a, float b, float gamma, float alpha, int epoch, uint64_t seed, int part,
                             void *workspace, size_t workspace_bytes, void *stream);

/* ---- Spring layout ----------------------------------------------------------------
 * The kernels under ampnet_amd.spring (csrc/spring.hip): the reference's picture of a graph --
 * synthetic_benchmark/synthetic_xor.py (plot_graph: nx.spring_layout(G)) and
 * visualization/visualize_graphsaint_subgraphs.py (nx.draw(g), whose default layout is the same).  Added without a
 * version change: no existing argument list changes.
 *
 * WHAT ampnet_amd.spring_layout COMPUTES.  This text and the fp64 model in tests/spring_reference.py ARE the
 * specification: networkx 3.4.2's spring_layout (drawing/layout.py: _fruchterman_reingold,
 * _sparse_fruchterman_reingold, rescale_layout), restated here because networkx is not a dependency.  Parity with
 * networkx's VALUES is pinned by the fixtures under tests/golden/spring; parity with its bits is not.  With N nodes,
 * dim in {2, 3}, the adjacency A as a CSR with float32 weights and positions y [N, dim] float32:
 *   optimal distance: k = 1 / sqrt(N) unless given; with fixed nodes and no k, dom_size / sqrt(N), dom_size = the
 *   largest coordinate of the given positions, 1 if that is 0.
 *   temperature: t0 = 0.1 max(extent of column 0, extent of column 1) of the start -- the first two columns only, as
 *   networkx has it -- and dt = t0 / (iterations + 1), both fp64.
 *   iteration (SYNCHRONOUS: reads y_in, writes y_out):
 *     rep_i = sum_j (y_i - y_j) / max(|y_i - y_j|^2, 1e-4f) over ALL j: a coincident point and j = i contribute exactly
 *     0, so no index is excluded;
 *     att_i = sum over the entries e = (i -> j) of row i of w_e max(sqrt(|y_i - y_j|^2), 0.01f) (y_i - y_j);
 *     disp_i = k^2 rep_i - att_i / k (fp64); len_i = |disp_i|, replaced by 0.1 where it is < 0.01;
 *     delta_i = fp32(disp_i (t / len_i)), zero for fixed nodes; y_out = y_in + delta (fp32);
 *     then t -= dt, ran += 1, done = sqrt(sum delta^2) / N < threshold.
 *   start: a given tensor, or uniform [0, 1): y[i, c] = (draw(seed, i, c) >> 40) 2^-24 with the library's stream,
 *   draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b)) (uint64, wrapping); with fixed nodes and
 *   partial positions the others are rand dom_size + center, networkx's rule.
 *   finish (no fixed nodes, scale not None): subtract the fp64 column means, multiply by scale / max|y| (skipped if the
 *   maximum is 0), add center.
 *
 * DEVICE STATE.  ampconv_spring_state: {double t, double dt, int64 ran, int64 done}, 32 bytes on the device, 8-byte
 * aligned; the host reads nothing during the layout.  A step entered with done != 0 copies y_in to y_out and changes
 * nothing else (the repulsion, given the state, launches and returns at once), so a fixed sequence of `iterations`
 * steps reproduces networkx's `break`.
 *
 * ampconv_spring_start: y [N, dim] fp32 dense = the uniform start above.
 *
 * ampconv_spring_repulsion: y [N, dim] fp32 dense, 8-byte aligned; rep [N, dim] fp64.  Pair arithmetic is fp32:
 * y_i - y_j, |.|^2 by FMAs over the coordinates in order from 0, max with 1e-4f, one v_rcp_f32 (1 ulp), one FMA per
 * coordinate into the sum -- k^2 is applied by the step, after the sums.  For row i the sums run over the keys j in
 * ascending order in fp32 for a run of AMPCONV_SPRING_RUN keys (runs start at multiples of it), the runs of a chunk are
 * added in order in fp64, the chunks in order in fp64.  A chunk is AMPCONV_SPRING_CHUNK
 * ceil(ceil(N / AMPCONV_SPRING_CHUNK) / 64) keys: a function of N alone, so is the launch.  No atomics: two calls give
 * the same bits.  |rep - exact| <= (AMPCONV_SPRING_RUN + 16) 2^-24 sum_j |term_j| per coordinate.  state (NULL: always
 * computed): with state->done != 0 rep is left as it is.  Workspace: ampconv_spring_repulsion_workspace_bytes(N, dim),
 * 8-byte aligned: the chunks' fp64 sums [chunk][dim][N], at most 64 chunks (37 MB at 96 000 points, dim 2).
 *
 * ampconv_spring_step: one iteration from rep as ampconv_spring_repulsion left it.  y_in, y_out [N, dim] fp32 dense,
 * 8-byte aligned, different buffers; the CSR of A (indptr [N + 1], indices [nnz] int64; a column outside [0, N) is
 * clamped, positions outside [0, nnz] likewise); val [nnz] fp32, NULL: every weight is 1; fixed [N] bytes, nonzero: the
 * node does not move, NULL: none is fixed.  The attraction of a row: the row is cut into groups of 64 entries from its
 * start, lane l of a wave takes entry l of the group in fp32 (the pair arithmetic above, sqrt correctly rounded, the
 * weight times the clamped distance, one FMA per coordinate), a butterfly adds the lanes, the groups are added in order
 * in fp64.  A row longer than AMPCONV_SPRING_PART entries is cut into parts of that length whose groups separate waves
 * compute and store; the order of the additions is the same, so THE RESULT DOES NOT DEPEND ON THE PART LENGTH --
 * ampconv_spring_step_split takes it as an argument (a multiple of 64 in [64, 2^24]) for tests to show that.
 * |att - exact| <= 16 2^-24 sum_e |term_e| per coordinate.  The rows' sum delta^2 (fp64, of the float32 delta) is added
 * by lane t of one workgroup taking the rows t, t + 256, ... in order and a binary tree (s[t] += s[t + o],
 * o = 128 .. 1); that workgroup then moves the state.  Workspace: ampconv_spring_step_workspace_bytes(N, nnz, dim),
 * 8-byte aligned: (nnz / 64 + N + 1) dim floats and N doubles.
 * AMPCONV_E_BADARG (nothing launched): a NULL or misaligned pointer, y_in == y_out, N outside
 * [1, AMPCONV_SPRING_MAX_N], dim outside {2, 3}, nnz < 0, k not positive and finite, part out of range.
 * AMPCONV_E_WORKSPACE: a NULL or short workspace.  */
#define AMPCONV_SPRING_MAX_N (1 << 24)
#define AMPCONV_SPRING_RUN 256
#define AMPCONV_SPRING_TILE 1024
#define AMPCONV_SPRING_CHUNK 4096
#define AMPCONV_SPRING_PART 1024
typedef struct {
  double t, dt;
  int64_t ran, done;
} ampconv_spring_state;
int ampconv_spring_start(float *y, int64_t N, int dim, uint64_t seed, void *stream);
size_t ampconv_spring_repulsion_workspace_bytes(int64_t N, int dim);
int ampconv_spring_repulsion(const float *y, int64_t N, int dim, double *rep, const ampconv_spring_state *state,
                             void *workspace, size_t workspace_bytes, void *stream);
size_t ampconv_spring_step_workspace_bytes(int64_t N, int64_t nnz, int dim);
int ampconv_spring_step(const float *y_in, float *y_out, int64_t N, int dim, const int64_t *indptr, const int64_t *indices,
                        const float *val, int64_t nnz, const uint8_t *fixed, const double *rep, double k, double threshold,
                        ampconv_spring_state *state, void *workspace, size_t workspace_bytes, void *stream);
int ampconv_spring_step_split(const float *y_in, float *y_out, int64_t N, int dim, const int64_t *indptr,
                              const int64_t *indices, const float *val, int64_t nnz, const uint8_t *fixed, const double *rep,
                              double k, double threshold, ampconv_spring_state *state, int part, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---- stochastic block model graphs (csrc/sbm.hip; pure additions, the ABI number stays 111) -------------------------
 * Random graphs with class structure, drawn on the device: ampnet_amd.random_graphs (stochastic_block_model,
 * random_partition_graph, gnp_random_graph, xor_link_dataset -- the link data of the reference's
 * synthetic_benchmark/synthetic_xor.py:104-165 and the graph of synthetic_rpg.py:39-121).
 *
 * THE BLOCK MODEL (a contract, like THE WALK STREAM: tests rebuild it on the host, tests/sbm_reference.py).
 *   inputs: sizes[K], every entry >= 0, N = sum(sizes); start[0] = 0, start[b + 1] = start[b] + sizes[b]; block b is the
 *   contiguous node range [start[b], start[b + 1]), block(u) the block that holds node u.  P fp64 [K, K] row-major,
 *   every entry in [0, 1].  Flags `directed` and `selfloops`, a 64-bit seed.
 *   unit (u, b), u a node and b a block: its candidates C(u, b) are the nodes v of block b in ascending order, without
 *   v == u unless `selfloops`, and, if not `directed`, only those with v > u (v >= u with `selfloops`).  m = |C|,
 *   p = P[block(u)][b].  m == 0 or p <= 0: no edge.  p >= 1: every candidate.  Otherwise, with
 *     lq = log1p(-p)       taken on the HOST in fp64 (numpy.log1p) and handed to the calls as the [K, K] table `lq`, so
 *                          that a host model and the kernel share its bits,
 *     draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b))      (uint64, wrapping: the library's stream)
 *   start with j = -1 and for t = 0, 1, ...:
 *     r = draw(seed, u K + b, t);  U = ((r >> 11) + 1) 2^-53, in (0, 1];  q = log(U) / lq in fp64;
 *     if !(q < m - 1 - j): stop -- compared IN FP64, before any conversion to an integer (q reaches 1e300 for tiny p);
 *     j += 1 + (int64)floor(q);  emit the edge (u, C[j]).
 *   j grows by at least 1 per step and stays below m, so every chain ends.  The skips are geometric, hence memoryless:
 *   every candidate pair is an independent Bernoulli(p) trial -- the distribution of networkx's
 *   stochastic_block_model(sizes, p, directed=, selfloops=) and, up to the 2^-53 grid of U, of the reference's loops.
 *   output, directed: the edges ordered by u, then b, then j: row-major (row, col) ascending, the order of the
 *   reference's listing loops (synthetic_xor.py:158-162).  Undirected: that list of pairs u <= v, followed by the
 *   mirrors (v, u) of its pairs with v != u in the same order.  edge_index int64 [2, E], block int64 [N].
 *   limits: E <= 2^31 - 1, N <= 2^31 - 1, K <= AMPCONV_SBM_MAX_K.
 * The only floating-point operation the device adds to the host's share is log(U) (the division is IEEE): a host model
 * whose log is a few ulp from the device's gives the same graph unless some q lies that close to an integer.
 *
 * ampconv_sbm_count: count[u K + b] = the number of edges unit (u, b) emits (int64 [N K]); mcount (NULL: not wanted),
 * the same shape: that number without the unit's self loop (u, u) -- the number of MIRRORS the unit has in an undirected
 * graph.  Units with p >= 1 or p <= 0 are closed forms, the others walk their chain.
 * ampconv_sbm_fill: walks the same chains and writes edge i of unit (u, b) to row[off[u K + b] + i] = u,
 * col[...] = C[j]; off is the exclusive prefix sum of count (the caller's scan).  With moff (NULL: no mirrors) mirror i
 * of the unit -- its edges with v != u, in order -- goes to position mirror_base + moff[u K + b] + i as (v, u); moff is the
 * exclusive prefix sum of mcount (== off without self loops) and mirror_base the total of count.  E: the length of row
 * and of col; a position outside [0, E) -- offsets that are not those of the same arguments -- is not written.
 * Lane l of a wave takes node 64 w + l of ONE block b: the lanes share p (where they share block(u)) and nearly share
 * m, and a wave lasts as long as its longest chain.  No atomics, every position written by exactly one lane: two calls
 * give the same bits.  Nothing is allocated and nothing synchronised.
 * sizes: a HOST array [K] (like the descriptors of ampconv_adam_step: it travels as a kernel argument); P, lq, count,
 * mcount, off, moff, row, col: device pointers, 8-byte aligned.
 * AMPCONV_E_BADARG (nothing launched): a NULL or misaligned pointer (mcount, moff may be NULL), K outside
 * [1, AMPCONV_SBM_MAX_K], a negative size, N above 2^31 - 1, E or mirror_base negative.  N == 0 succeeds.  */
#define AMPCONV_SBM_MAX_K 256
int ampconv_sbm_count(const int64_t *sizes, int K, const double *P, const double *lq, int directed, int selfloops,
                      uint64_t seed, int64_t *count, int64_t *mcount, void *stream);
int ampconv_sbm_fill(const int64_t *sizes, int K, const double *P, const double *lq, int directed, int selfloops,
                     uint64_t seed, const int64_t *off, const int64_t *moff, int64_t mirror_base, int64_t *row, int64_t *col,
                     int64_t E, void *stream);

/* ---- MASKED FEATURE MODELLING (csrc/mfm.hip; pure additions, the ABI number stays 111) -------------------------------
 * The training signal of the reference's predictive_ssl_AMPNet.py, which stops at `criterion = None`: some tokens of the
 * featuriser are hidden behind a learned mask token (the masked-autoencoder `mask_token` of every reference model class,
 * gcn_one_layer.py:43-54; the replacement loop of gcn_classifier.py:138-151) and a linear decoder behind the last AMPConv
 * layer is asked for their z-scored values back: the mean squared residual over the masked tokens.  One pass per
 * direction that reads the masked rows only.  N nodes, L tokens per node, T = N L tokens, t = n L + l.
 *
 * THE TOKEN MASK (a contract, like THE SAMPLING STREAM: tests rebuild it on the host, tests/mfm_reference.py).  With the
 * library's stream draw(seed, a, b) = splitmix64(seed ^ splitmix64(a * 0x100000001B3 + b)) (uint64, wrapping):
 *   token (n, l) is MASKED iff idx[n, l] >= 0 and (uint32)(draw(seed, n, l) >> 48) < threshold.
 * The caller passes threshold = round(rate * 65536), 0 <= threshold <= 65536 (anything else: AMPCONV_E_BADARG); the
 * comparison is a 32-bit one, so 65536 masks every valid token and 0 none.  The mask depends on (seed, n, l) only: not on
 * the dtype, the row width or the launch shape.
 *
 * ampconv_mfm_build: ampconv_feat_build_as with the masking fused in.  x, mean, inv_std, idx, table, N, F, L, De, out,
 *   dtype as there (out [N, L, De + 1] in `dtype`), and: mask_token [De + 1] fp32; seed, threshold: THE TOKEN MASK;
 *   masked_in [N, L] bytes or NULL -- not NULL: that mask is REPLAYED (a token is masked iff masked_in[t] != 0 and
 *   idx[t] >= 0) and seed, threshold are not used (threshold is still checked).  Outputs besides `out`:
 *     masked [N, L] uint8: 1 for a masked token, else 0 -- the mask that was used;
 *     target [N, L] fp32: z = (x[n, idx] - mean[idx]) * inv_std[idx] of EVERY token, masked or not, the fp32 value that
 *                         feat_build puts into the value slot before any rounding to `dtype`; 0 where idx == -1.
 *   mode AMPCONV_MFM_TOKEN: a masked token is mask_token as a whole, out[t, c] = mask_token[c] for c in [0, De]
 *                           (gcn_classifier.py:151).
 *   mode AMPCONV_MFM_VALUE: a masked token keeps out[t, :De] = table[idx[t]] and gets out[t, De] = mask_token[De]: the
 *                           value is hidden, the identity of the feature is kept (with sampled tokens the only
 *                           well-posed task: which feature a hidden token stood for is otherwise unknown).
 *   Every element is the fp32 value rounded to nearest even to `dtype`.  An unmasked token, and a token with idx == -1
 *   (a zero row, never masked), has the bits ampconv_feat_build_as writes; with threshold == 0 the whole of `out` has.
 * ampconv_mfm_token_grad: dmask_token [De + 1] fp32 from dout [N, L, De + 1] (read in `dtype`, summed in fp32).  TOKEN:
 *   dmask_token[c] = sum of dout[t, c] over the masked tokens; VALUE: component De is that sum, the others exact zeros.
 *   Rows of unmasked tokens are not read.  The table gradient needs no call of its own: ampconv_feat_table_grad_from on
 *   idx with the masked entries set to -1 (TOKEN), on idx as it is (VALUE).
 * ampconv_mfm_loss_fwd: h [N, L, D] contiguous in `dtype`, masked [N, L] bytes, target [N, L] fp32, w [D] and b [1] fp32.
 *   For each MASKED token only (masked[t] != 0):  pred = b + sum_c w[c] h[t, c],  r = pred - target[t], fp32 arithmetic.
 *   Rows of unmasked tokens are NOT READ (they may hold NaN).  Outputs:
 *     resid [N, L] fp32: r for the masked tokens, exact 0 elsewhere;
 *     state int64 [2], overwritten: this call's own sums, state[0] = sum over the masked tokens of
 *           rint(r * r * 2^AMPCONV_MFM_LOSS_SHIFT), the product of the fp32 r taken in fp64 (exact), state[1] = their number;
 *     sums  int64 [2] or NULL (not wanted): state is ADDED to it -- the caller zeroes it (a running buffer over many calls);
 *     *loss fp32 on the device = state[0] / 2^SHIFT / max(state[1], 1): the mean squared residual, 0 without masked tokens.
 *   The sums are 64-bit integer atomics (the fixed point of AMPCONV_HEAD_LOSS_SHIFT): independent of the order, so
 *   bitwise reproducible; per-term error <= 2^-33; exact while the sum of squares stays below 2^31.  No host read-back.
 * ampconv_mfm_loss_bwd: h, masked, w as above, resid and state as loss_fwd left them, *g the upstream gradient of *loss,
 *   read ON THE DEVICE like the count state[1]:  c = 2 * *g / max(state[1], 1),
 *     dh[t, :] = c * resid[t] * w for the masked tokens, exact zeros for all others: the whole [N, L, D] is written, in
 *                `dtype` (rounded to nearest even); NULL: not wanted;
 *     dw[c] = sum_t c * resid[t] * h[t, c],  db[0] = sum_t c * resid[t]   over the masked tokens (rows of the others are
 *                not read), fp32.
 *   Without masked tokens dh, dw and db are exact zeros and nothing is NaN.
 * DETERMINISM.  Every output has the same bits on every launch.  dw, db and dmask_token: a fixed-order two-stage
 * reduction -- per workgroup the tokens in a fixed order, the workgroup's partial row in `workspace`
 * (ampconv_mfm_workspace_bytes(N, L, D), D = De + 1 for token_grad; need not be zeroed), the rows added in workgroup order
 * by a second kernel.  No floating-point atomics in any of these kernels.
 * ACCESS.  A token row sits in the registers of a group of 4..64 lanes.  h, dh and dout are read and written in 16-byte
 * pieces where they and w are 16-byte aligned and D is a whole number of pieces (bf16: 8-byte pieces where those hold
 * for 8 bytes and D % 4 == 0), element by element otherwise (the XOR toy's D = 3).  The build moves one element per lane
 * (a table row of De floats starts on no 16-byte boundary).
 * ERRORS, nothing launched: a negative size, L < 1, D < 1, F < 1, De < 0, N L D beyond int64, an unknown mode, a threshold
 * above 65536 or a missing pointer: AMPCONV_E_BADARG; a dtype other than AMPCONV_F32 / AMPCONV_BF16: AMPCONV_E_DTYPE; a
 * workspace shorter than ampconv_mfm_workspace_bytes: AMPCONV_E_WORKSPACE.  N == 0 succeeds (data pointers may be NULL):
 * the loss is 0, state zeros, dw, db and dmask_token zeros.  */
enum { AMPCONV_MFM_TOKEN = 0, AMPCONV_MFM_VALUE = 1 };
#define AMPCONV_MFM_LOSS_SHIFT 32
size_t ampconv_mfm_workspace_bytes(int64_t N, int L, int D);
int ampconv_mfm_build(const float *x, const float *mean, const float *inv_std, const int32_t *idx, const float *table,
                      int64_t N, int F, int L, int De, const float *mask_token, uint64_t seed, uint32_t threshold, int mode,
                      const uint8_t *masked_in, void *out, uint8_t *masked, float *target, int dtype, void *stream);
int ampconv_mfm_token_grad(const void *dout, const uint8_t *masked, int64_t N, int L, int De, int mode, float *dmask_token,
                           void *workspace, size_t workspace_bytes, int dtype, void *stream);
int ampconv_mfm_loss_fwd(const void *h, const uint8_t *masked, const float *target, const float *w, const float *b,
                         int64_t N, int L, int D, float *resid, int64_t *sums, int64_t *state, float *loss, int dtype,
                         void *stream);
int ampconv_mfm_loss_bwd(const void *h, const uint8_t *masked, const float *resid, const float *w, const int64_t *state,
                         const float *g, int64_t N, int L, int D, void *dh, float *dw, float *db, void *workspace,
                         size_t workspace_bytes, int dtype, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AMPCONV_H_ */
