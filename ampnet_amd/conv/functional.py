"""Fused AMPConv forward/backward on MI355X: projections as dense GEMMs on the
per-NODE rows, edge phase in hand-written HIP through the C ABI.

What it replaces in the reference (paths relative to /root/reference):
  src/ampnet/conv/amp_conv.py:24-26,28-51   propagate -> message -> mean
  torch functional.py:5785-5862             packed in-projection (per edge there, per node here)
  torch functional.py:6578-6601             scale, QK^T, softmax, PV, out-projection
Backward formulas: SURVEY.md A.2 (the reference relies on autograd).

Data layout in HBM (fp32):
  QKV   [N*L, 3D]   one packed projection; Q/K/V are column thirds (strided views)
  Obar  [N*L, D]    mean over in-edges of the per-edge attention output, pre out-proj
  dQKV  [N*L, 3D]   written by the two backward edge passes, consumed by one GEMM each
                    for dX and d(in_proj_weight)
"""
import contextlib
import ctypes
import dataclasses
import os
import threading

import torch

from .. import _lib
from ..graph import EdgeCSR, _stream


def _view(buf2d, col_off, L, dh):
    """ampconv_view_t over columns [col_off, col_off + D) of a contiguous [rows*L, W] buffer."""
    assert buf2d.is_contiguous() and buf2d.dtype in (torch.float32, torch.bfloat16)
    W = buf2d.size(1)
    return _lib.View(buf2d.data_ptr() + buf2d.element_size() * col_off, L * W, W, dh)


def _ptr(t):
    return t.data_ptr() if t is not None else None


GEMM_PRECISIONS = ('native', 'fp32', 'bf16x3')
# hand the softmax statistics of the destination pass to the source pass (AMPCONV_SOFTMAX_STATS=0:
# both passes reduce their own; used by the tests to cross-check the two ways)
SOFTMAX_STATS = os.environ.get('AMPCONV_SOFTMAX_STATS', '1') != '0'


_GEMM_SWITCH_LOCK = threading.RLock()


@contextlib.contextmanager
def gemm_precision(mode):
    """How the dense fp32 projections run.  'fp32': plain fp32 MFMA GEMMs (rocBLAS, ~135-150
    TFLOP/s on MI355X).  'bf16x3': hipBLASLt's fp32 GEMM that splits each operand into two bf16
    planes and sums three bf16 MFMA products in fp32 (what ROCm serves as "TF32" on gfx950, which
    has no xf32 matrix instruction): ~2x the rate, element error ~5e-6 of the largest output
    instead of ~6e-7 (tools/bench_gemm.py).  Inputs, outputs and accumulation stay fp32; the
    edge kernels are not affected.

    torch's switches (allow_tf32, preferred BLAS library, HIPBLASLT_ALLOW_TF32) are PROCESS-GLOBAL:
    they are set for the duration of the block and restored, under a lock so that two layers (the
    autograd thread runs backward) never interleave their set/restore.  fp32 GEMMs issued by OTHER
    threads while a 'bf16x3' block is open run in that mode too -- keep the default 'fp32' if that
    matters (tests/test_gpu_parity.py::test_gemm_precision_is_restored pins the restore)."""
    if mode not in GEMM_PRECISIONS:
        raise ValueError(f'gemm precision must be one of {GEMM_PRECISIONS}, got {mode!r}')
    if mode in ('fp32', 'native'):      # 'native': libampconv's own projection kernels (proj_* below); what they
        yield                           # do not serve (bf16 storage, D % 4 != 0) runs as plain library GEMMs
        return
    with _GEMM_SWITCH_LOCK:
        prev_env = os.environ.get('HIPBLASLT_ALLOW_TF32')
        prev_tf32 = torch.backends.cuda.matmul.allow_tf32
        prev_lib = torch.backends.cuda.preferred_blas_library()
        os.environ['HIPBLASLT_ALLOW_TF32'] = '1'
        torch.backends.cuda.matmul.allow_tf32 = True
        torch.backends.cuda.preferred_blas_library('hipblaslt')
        try:
            yield
        finally:
            torch.backends.cuda.preferred_blas_library(prev_lib)
            torch.backends.cuda.matmul.allow_tf32 = prev_tf32
            if prev_env is None:
                os.environ.pop('HIPBLASLT_ALLOW_TF32', None)
            else:
                os.environ['HIPBLASLT_ALLOW_TF32'] = prev_env


def _tn_matmul(a, b, chunks=128):
    """a^T @ b for tall operands a [M, p], b [M, q] (the weight-gradient GEMMs, reduction over
    the N*L node-token rows).  rocBLAS runs the single [p, M] x [M, q] product at 65-95 TFLOP/s
    at M = 2e7; splitting the reduction into `chunks` batched GEMMs + one sum runs at
    ~150 TFLOP/s (measured on MI355X, tools/bench_dw.py) and sums pairwise, i.e. more accurately."""
    M = a.size(0)
    if M < (1 << 18):
        return a.t().mm(b)
    per = M // chunks
    main = per * chunks
    out = torch.bmm(a[:main].view(chunks, per, -1).transpose(1, 2), b[:main].view(chunks, per, -1)).sum(0)
    if main < M:
        out += a[main:].t().mm(b[main:])
    return out


# ---- the per-node projections in libampconv.so.  fp32 storage (csrc/proj_gemm.hip): operands scaled by a power of two
# and split into two fp16 planes, three partial products on v_mfma_f32_32x32x16_f16 (large operands; PROJ_SCALED below), or
# split exactly into three bf16 terms, six partial products on v_mfma_f32_32x32x16_bf16; fp32 accumulate.  bf16 storage
# (csrc/proj_gemm_bf16.hip): one product, fp32 accumulate, one rounding on the way out
NODE_LISTS = os.environ.get('AMPCONV_NODE_LISTS', '1') != '0'      # developer switch (A/B measurements)
# fp32 storage: two scaled fp16 planes, three products (include/ampconv.h "SCALED MODE"); '0': three bf16 planes, six
PROJ_SCALED = os.environ.get('AMPCONV_PROJ_SCALED', '1') != '0'
# ... for operands of at least this many elements: the mode costs five more (tiny) launches per layer call -- two
# maxima in the forward pass, two in the backward, one for the weights -- which a Cora-sized step (0.6 ms) feels and a
# GraphSAINT batch (24 ms) does not
PROJ_SCALED_MIN_ELEMENTS = 1 << 24


# fp32 storage, scaled mode, L <= 20, head width 32 or 16, self-attention layers (xq is xkv): the edge passes run on the
# 16-bit matrix pipe -- the in-projection and dObar = dY Wo leave their kernels as two fp16 planes of the scaled value
# (csrc/edge_mfma_f16x2.hip, include/ampconv.h "edge phase on fp16 PLANES"); '0': the fp32-MFMA edge kernels
EDGE_PLANES = os.environ.get('AMPCONV_EDGE_PLANES', '1') != '0'
# ONE power-of-two scale per tensor serves rows within this many binades of the tensor's maximum at fp32 grade; operands
# that have a head slot further down (ampconv_absmax_stats) take the exact kernels instead: six-product projections,
# fp32 edge passes.  The price of knowing is one 8-byte read-back per operand (x: cached per tensor version; dY: per step)
RANGE_LOG2 = 12
_STATS_CACHE = {}         # id(tensor) -> (weakref, _version, stats tensor, narrow, (data_ptr, shape))


def operand_stats(t2, key=None):
    """(stats, narrow): stats = device tensor [largest finite magnitude, smallest non-zero head-slot maximum] of the
    2-D fp32 tensor t2 (one pass, ampconv_absmax_stats), narrow = the whole tensor lies within 2^RANGE_LOG2 of its
    maximum (host bool: ONE 8-byte read-back).  key: the tensor OBJECT the caller was handed (t2 may be a view of it);
    the result is remembered for as long as that object lives and its version counter stands still -- the features of
    a full-graph run are measured once, not once per step."""
    import weakref
    if key is not None:
        hit = _STATS_CACHE.get(id(key))
        if (hit is not None and hit[0]() is key and hit[1] == key._version and hit[4] == (key.data_ptr(), tuple(key.shape))
                and hit[2].device == t2.device):
            return hit[2], hit[3]
    lib = _lib.load()
    t2 = _aligned(t2)
    st = torch.empty(2, dtype=torch.float32, device=t2.device)
    _lib.check(lib.ampconv_absmax_stats(t2.data_ptr(), t2.stride(0), t2.size(0), t2.size(1), st.data_ptr(), _stream()),
               'ampconv_absmax_stats')
    amax, smin = st.tolist()
    narrow = not (smin * float(1 << RANGE_LOG2) < amax)          # (an all-zero tensor: inf < 0 is false -> narrow)
    if key is not None:
        if len(_STATS_CACHE) >= 16:
            for k in [k for k, v in _STATS_CACHE.items() if v[0]() is None] or list(_STATS_CACHE)[:8]:
                _STATS_CACHE.pop(k, None)
        _STATS_CACHE[id(key)] = (weakref.ref(key), key._version, st, narrow, (key.data_ptr(), tuple(key.shape)))
    return st, narrow


def planes_to_f32(buf2d, bound, dh=32):
    """fp32 copy of a projection buffer held in the plane format with slots of `dh` channels (side outputs, fall-backs)."""
    out = torch.empty_like(buf2d)
    _lib.check(_lib.load().ampconv_planes_to_f32(buf2d.data_ptr(), buf2d.stride(0), buf2d.size(0), buf2d.size(1), dh,
                                                 bound.data_ptr(), out.data_ptr(), out.stride(0), _stream()),
               'ampconv_planes_to_f32')
    return out


def proj_out_bound(W, transpose, bias, amax, out):
    """out[0] = amax * (largest absolute row sum of B) + max |bias|, B = W (transpose: W^T): the scale source of a
    plane-format projection output, on the device."""
    R, C = W.shape
    N, K = (C, R) if transpose else (R, C)
    sn, sk = (1, W.stride(0)) if transpose else (W.stride(0), 1)
    _lib.check(_lib.load().ampconv_proj_out_bound(W.data_ptr(), sn, sk, N, K, _ptr(bias), amax.data_ptr(), out.data_ptr(),
                                                  _stream()), 'ampconv_proj_out_bound')


def proj_rows_planes(a2, image, bound, bias=None, rowptr=None, L=0, row_scale=0, amax=None, out_amax=None, amax_col0=0,
                     dh=32):
    """proj_rows whose output leaves as two fp16 planes of value * 2^e(bound) in the 4 dh-byte head slots of the fp32 buffer
    (include/ampconv.h; dh = 32 or 16).  row_scale = 1 (with rowptr): rows are divided by their node's in-degree (0 for none)."""
    lib = _lib.load()
    img, N, K, wdt = image
    assert a2.dim() == 2 and a2.size(1) == K and a2.stride(1) == 1 and a2.dtype == wdt == torch.float32
    a2 = _aligned(a2)
    out = torch.empty(a2.size(0), N, dtype=wdt, device=a2.device)
    _lib.check(lib.ampconv_proj_rows_planes(a2.data_ptr(), a2.stride(0), a2.size(0), K, img.data_ptr(), N, _ptr(bias),
                                            _ptr(rowptr), L, row_scale, out.data_ptr(), out.stride(0), amax.data_ptr(),
                                            bound.data_ptr(), _ptr(out_amax), amax_col0, dh, _stream()),
               'ampconv_proj_rows_planes')
    return out


# Sequences of at most 4 tokens stay on the short-sequence kernels (csrc/edge_small.hip: one wave per ROW, no tile padding):
# the plane-format kernels pad every sequence to 20-token tiles (config 3's L = 4 sweep: 4.0 ms per step there, 14.2 here)
PLANES_MIN_L = 5


def absmax(t2, out=None, reset=False):
    """Largest finite magnitude of a 2-D tensor with contiguous rows, as a one-element device tensor (no host sync):
    the scale source of the fp32 projections' two-plane mode.  `out`: merge into an existing maximum (reset: zero it
    first)."""
    lib = _lib.load()
    t2 = _aligned(t2)
    if out is None:
        out, reset = torch.empty(1, dtype=torch.float32, device=t2.device), True
    _lib.check(lib.ampconv_absmax(t2.data_ptr(), t2.stride(0), t2.size(0), t2.size(1), _code(t2.dtype), out.data_ptr(),
                                  1 if reset else 0, _stream()), 'ampconv_absmax')
    return out


def _zero(scalar):
    """Zero a one-element fp32 device tensor on the current stream (the receiving end of proj_rows' out_amax)."""
    _lib.check(_lib.load().ampconv_absmax(None, 0, 0, 0, _lib.AMPCONV_F32, scalar.data_ptr(), 1, _stream()),
               'ampconv_absmax')


def _code(dtype):
    return _lib.AMPCONV_BF16 if dtype == torch.bfloat16 else _lib.AMPCONV_F32


def proj_native(gemm, dtype, D):
    """Does the 'native' mode serve this layer?  fp32 storage with embed_dim a multiple of 4, bf16 storage with a
    multiple of 8 (rows move in 16-byte pieces)."""
    return (gemm == 'native' and dtype in (torch.float32, torch.bfloat16)
            and bool(_lib.load().ampconv_proj_supported(D, D, _code(dtype))))


def _aligned(t):
    """Rows in 16-byte pieces: a view whose first element is not 16-byte aligned (a slice of a larger tensor) is copied."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


def proj_images(jobs):
    """MFMA-fragment images of weights, ALL in one launch: `jobs` = [(W, transpose), ...] (at most 8), W [R, C]
    with contiguous rows, all of one dtype; an image of W itself serves out = in @ W^T (the forward direction of
    nn.Linear), of W^T serves out = in @ W (its input gradient).  Returns [(image bytes, N, K, dtype), ...]."""
    lib = _lib.load()
    descs, outs, off = (_lib.WeightImage * len(jobs))(), [], 0
    dims = []
    wdt = jobs[0][0].dtype
    code = _code(wdt)
    for W, transpose in jobs:
        assert W.dim() == 2 and W.stride(1) == 1 and W.dtype == wdt
        R, C = W.shape
        N, K = (C, R) if transpose else (R, C)
        dims.append((N, K, lib.ampconv_proj_weight_image_bytes(N, K, code)))
    buf = torch.empty(sum(d[2] for d in dims), dtype=torch.uint8, device=jobs[0][0].device)
    for i, ((W, transpose), (N, K, nb)) in enumerate(zip(jobs, dims)):
        sn, sk = (1, W.stride(0)) if transpose else (W.stride(0), 1)
        img = buf[off:off + nb]
        descs[i] = _lib.WeightImage(W.data_ptr(), sn, sk, N, K, img.data_ptr())
        outs.append((img, N, K, wdt))
        off += nb
    _lib.check(lib.ampconv_proj_weight_images(len(jobs), ctypes.cast(descs, ctypes.c_void_p), code, _stream()),
               'ampconv_proj_weight_images')
    return outs


def proj_image(W, transpose=False):
    return proj_images([(W, transpose)])[0]


def proj_rows(a2, image, bias=None, rowptr=None, L=0, nodes=None, out=None, amax=None, out_amax=None):
    """out[M, N] = (a2[M, K] @ B^T + bias) * [node of the row has an in-edge]  (mask only with rowptr).
    nodes = (ids, count[, ptr]) (EdgeCSR.active_nodes): only the L rows of each listed node are computed and written
    (bf16; the other rows of `out` keep what they hold: uninitialised unless the caller passes `out`).
    amax (fp32 storage): one-element tensor, the operand's largest finite magnitude or a bound of it (absmax) -> the
    two-plane scaled kernels; out_amax: a zeroed one-element tensor that receives the output's."""
    lib = _lib.load()
    img, N, K, wdt = image
    assert a2.dim() == 2 and a2.size(1) == K and a2.stride(1) == 1 and a2.dtype == wdt
    assert bias is None or bias.dtype == wdt
    a2 = _aligned(a2)
    if out is None:
        out = torch.empty(a2.size(0), N, dtype=wdt, device=a2.device)
    assert out.shape == (a2.size(0), N) and out.stride(1) == 1 and out.dtype == wdt
    ids, cnt = (nodes[0].data_ptr(), nodes[1]) if nodes is not None else (None, 0)
    _lib.check(lib.ampconv_proj_rows(a2.data_ptr(), a2.stride(0), a2.size(0), K, img.data_ptr(), N, _ptr(bias),
                                     _ptr(rowptr), L, out.data_ptr(), out.stride(0), ids, cnt, _ptr(amax), _ptr(out_amax),
                                     _code(wdt), _stream()), 'ampconv_proj_rows')
    return out


def proj_wgrad(a2, b2, dw, colsum=None, rowptr=None, L=0, nodes=None, amax=None):
    """dw[Na, Nb] = (mask * a2)^T @ b2 and colsum[Na] = column sums of mask * a2, into caller-owned (views of)
    contiguous tensors of the inputs' dtype; reduction over the rows in fixed slices (bitwise reproducible).
    bf16: the mask acts on the column sums only (include/ampconv.h).  nodes: the sums run over the L rows of each
    listed node only (bf16).  amax = (a2's, b2's) largest finite magnitudes (fp32 storage: scaled two-plane kernels)."""
    lib = _lib.load()
    M, Na = a2.shape
    Nb = b2.size(1)
    assert b2.size(0) == M and dw.shape == (Na, Nb) and dw.is_contiguous() and a2.stride(1) == 1 and b2.stride(1) == 1
    assert a2.dtype == b2.dtype == dw.dtype and (colsum is None or colsum.dtype == a2.dtype)
    a2, b2 = _aligned(a2), _aligned(b2)
    code = _code(a2.dtype)
    ids, cnt = (nodes[0].data_ptr(), nodes[1]) if nodes is not None else (None, 0)
    nws = lib.ampconv_proj_wgrad_workspace_bytes(cnt * L if nodes is not None else M, Na, Nb, code)
    ws = torch.empty(max(nws, 16) // 4, dtype=torch.float32, device=a2.device)
    _lib.check(lib.ampconv_proj_wgrad(a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), M, Na, Nb,
                                      _ptr(rowptr), L, dw.data_ptr(), _ptr(colsum), ws.data_ptr(), nws, ids, cnt,
                                      _ptr(amax[0]) if amax else None, _ptr(amax[1]) if amax else None, code,
                                      _stream()), 'ampconv_proj_wgrad')


def _zero_unlisted(t2, nodes, n_nodes, L):
    """Zero the rows of the nodes a list leaves out (its CSR-shaped `ptr`: include/ampconv.h, ampconv_active_nodes)."""
    lib = _lib.load()
    assert t2.is_contiguous()
    io = _lib.AMPCONV_BF16 if t2.dtype == torch.bfloat16 else _lib.AMPCONV_F32
    _lib.check(lib.ampconv_mask_rows(t2.data_ptr(), nodes[2].data_ptr(), n_nodes, L * t2.size(1), io, _stream()),
               'ampconv_mask_rows')


def edge_forward(Q, K, V, csr, n_rows, L, D, H, out2d, qidx=None, dtype=_lib.AMPCONV_F32):
    """The plain forward edge pass (ampconv_fwd_edge): what edge_fwd runs for a 'plain' plan."""
    lib = _lib.load()
    plan, nch, ws = csr.hub_args('dst', L, D, 1) if qidx is None else (None, 0, None)
    rc = lib.ampconv_fwd_edge(Q, K, V, csr.rowptr.data_ptr(), csr.col.data_ptr(), _ptr(qidx),
                              n_rows, L, D, H, _view(out2d, 0, L, D // H), plan, nch, _ptr(ws),
                              dtype, _stream())
    _lib.check(rc, 'ampconv_fwd_edge')


@dataclasses.dataclass(frozen=True)
class LayerPlan:
    """Which kernels one AMPConvFunction call runs: chosen once by choose_plan, kept on ctx, and turned into the backward
    pass's plan by backward().
      native      the projections run on libampconv's own kernels (proj_* above); False: library GEMMs (`gemm`)
      scaled      fp32 projections in the scaled two-plane mode (their operand maxima: Scalars); False: exact
      edge        'planes': Q|K|V and dObar in the plane format, ampconv_*_edge_planes; 'views': fp32 views with bounds,
                  ampconv_*_edge_scaled; 'plain': ampconv_fwd_edge / _bwd_edge_dst / _bwd_edge_src at storage `dtype`
      lists       EdgeCSR.active_nodes() when the projections run over the listed nodes only (bf16), else None
      qkv_to_f32  (backward plans) the saved qkv is in the plane format but this pass reads fp32: planes_to_f32 first"""
    L: int
    D: int
    H: int
    shared: bool = True
    native: bool = False
    scaled: bool = False
    edge: str = 'plain'
    dtype: int = _lib.AMPCONV_F32
    gemm: str = 'fp32'
    lists: object = None
    qkv_to_f32: bool = False

    @property
    def dh(self):
        return self.D // self.H

    def backward(self, dy_narrow):
        """The backward pass's plan.  The scaled products serve dY only if it lies within 2^RANGE_LOG2 of its maximum too
        (dy_narrow, operand_stats); otherwise the whole pass takes the exact kernels: six-product projections and plain
        fp32 edge passes."""
        if not self.scaled or dy_narrow:
            return self
        return dataclasses.replace(self, scaled=False, edge='plain', qkv_to_f32=self.edge == 'planes')


def choose_plan(L, D, H, shared, dtype, gemm, numel, x_narrow, xkv_narrow, active_nodes, capturing,
                edge_dtype=_lib.AMPCONV_F32):
    """The LayerPlan of one call.  dtype: storage (torch); numel: elements of x (query side).  What depends on data comes
    in as callables, called only once the cheap conditions hold, x first: x_narrow / xkv_narrow -> operand_stats' verdict
    on x / xkv (xkv: unshared calls; one pass and one read-back unless cached, so never while a HIP graph is being
    recorded: `capturing`), active_nodes -> EdgeCSR.active_nodes(), or None when the call's rows are not the graph's
    nodes.  edge_dtype: storage code of the plain edge passes (bf16 storage: always AMPCONV_BF16)."""
    lib = _lib.load()
    bf16 = dtype == torch.bfloat16
    native = proj_native(gemm, dtype, D)
    # node lists: bf16 projections of a self-attention layer with 16 <= L <= 128 on a graph where a good share of the
    # nodes has no edge
    lists = None
    if NODE_LISTS and native and shared and bf16 and 16 <= L <= 128 and active_nodes is not None:
        lists = active_nodes()
    # the scaled mode serves operands that lie within 2^RANGE_LOG2 of their maximum; anything wider takes the exact
    # six-product kernels
    scaled = bool(native and PROJ_SCALED and dtype == torch.float32 and numel >= PROJ_SCALED_MIN_ELEMENTS
                  and not capturing() and x_narrow() and (shared or xkv_narrow()))
    edge = 'plain'
    if scaled and EDGE_PLANES and shared and L >= PLANES_MIN_L:
        if D % 128 == 0 and lib.ampconv_planes_supported(L, D, H):
            edge = 'planes'
        elif SOFTMAX_STATS and lib.ampconv_scaled_supported(L, D, H):   # (the workgroup-per-unit shapes, e.g. the
            edge = 'views'                                              # AMPGCN class defaults L = 40, D = 100, H = 2)
    return LayerPlan(L, D, H, shared, native, scaled, edge, _lib.AMPCONV_BF16 if bf16 else edge_dtype, gemm, lists)


@dataclasses.dataclass
class Scalars:
    """The device scalars of one layer call (one-element fp32 tensors; None where a field does not apply, i.e. all of
    them unless the plan is scaled): operand maxima of the scaled projections, and `bounds`, the float[4] that the plane
    and bound-carrying entry points read (include/ampconv.h), under the names below."""
    x: torch.Tensor = None          # max |x| (query side; self-attention: all of x), operand_stats
    xkv: torch.Tensor = None        # max |xkv| (unshared calls), operand_stats
    obar: torch.Tensor = None       # operand maximum of Obar, recorded by the in-projection (for_forward)
    bounds: torch.Tensor = None     # float[4] of the 'planes' and 'views' plans
    dy: torch.Tensor = None         # max |dY|, operand_stats
    dqkv: torch.Tensor = None       # max |dQ| (self-attention: of all of dQKV), recorded by the passes that write it
    dkv: torch.Tensor = None        # max |dK | dV| (unshared calls)

    qkv_bound = property(lambda s: s.bounds[0:1])       # >= max |Q|K|V|: the scale of the planes / views of QKV
    dobar_bound = property(lambda s: s.bounds[1:2])     # >= max |dObar|: the scale of dObar's planes / views
    v_max = property(lambda s: s.bounds[2:3])           # recorded max |V|
    dobar_max = property(lambda s: s.bounds[3:4])       # recorded max |dObar|

    @classmethod
    def for_forward(cls, plan, x, xkv):
        """Obar is a mean of convex combinations of V rows, so a maximum of |V| is its operand maximum, and the
        in-projection records it into `obar`, which is: 'planes': v_max (the V third only); 'views': qkv_bound
        (max |Q|K|V|, the scale of the whole tensor and the bound of |V|; the forward pass copies it to v_max, and the
        backward pass likewise copies dobar_bound, the recorded max |dObar|, to dobar_max); 'plain': a scalar of its
        own."""
        if not plan.scaled:
            return cls()
        s = cls(x=x, xkv=xkv)
        if plan.edge != 'plain':
            s.bounds = torch.zeros(4, dtype=torch.float32, device=x.device)
        s.obar = (s.v_max if plan.edge == 'planes' else s.qkv_bound if plan.edge == 'views'
                  else torch.zeros(1, dtype=torch.float32, device=x.device))
        return s

    def for_backward(self, dy):
        """The backward pass's holder: these scalars, max |dY| and a zeroed maximum of dQKV."""
        return dataclasses.replace(self, dy=dy, dqkv=torch.zeros(1, dtype=torch.float32, device=dy.device))


def _verdict(t2, key, maxima, name):
    """choose_plan's callable for one operand: operand_stats' narrow-range verdict, its maximum kept in maxima[name]."""
    def narrow():
        st, ok = operand_stats(t2, key=key)
        maxima[name] = st[0:1]
        return ok
    return narrow


def _qkv_views(q, kv, L, D, dh):
    """Views of the Q, K, V column thirds: all three in q (kv None: self-attention), or Q in q and K | V in kv."""
    src, off = (q, D) if kv is None else (kv, 0)
    return _view(q, 0, L, dh), _view(src, off, L, dh), _view(src, off + D, L, dh)


# ---- the three edge passes, each through the entry point of the plan's family (views: _view; sc: the call's Scalars)
def edge_fwd(plan, csr, Q, K, V, n_rows, obar, sc):
    if plan.edge == 'plain':
        return edge_forward(Q, K, V, csr, n_rows, plan.L, plan.D, plan.H, obar, dtype=plan.dtype)
    name = 'ampconv_fwd_edge_' + ('planes' if plan.edge == 'planes' else 'scaled')
    hub, nch, ws = csr.hub_args('dst', plan.L, plan.D, 1)
    _lib.check(getattr(_lib.load(), name)(Q, K, V, csr.rowptr.data_ptr(), csr.col.data_ptr(), n_rows, plan.L, plan.D,
                                          plan.H, _view(obar, 0, plan.L, plan.dh), hub, nch, _ptr(ws),
                                          sc.bounds.data_ptr(), _stream()), name)


def edge_bwd_dst(plan, csr, Q, K, V, dO, n_rows, dQ, sc):
    """dQ; returns the softmax statistics (normaliser, delta) per edge that this pass hands to the source pass, saving it
    its cross-lane reductions (include/ampconv.h), or None: that pass reduces its own.  Records max |dQ| into sc.dqkv."""
    lib = _lib.load()
    L, D, H = plan.L, plan.D, plan.H
    stats = spos = None
    nstat = lib.ampconv_softmax_stats_bytes(csr.num_edges, L, D, H, plan.dtype) if SOFTMAX_STATS else 0
    if nstat:
        stats = torch.empty(nstat // 4, dtype=torch.float32, device=csr.rowptr.device)
        spos = csr.csc_positions()
    hub, nch, ws = csr.hub_args('dst', L, D, 1)
    args = (Q, K, V, dO, csr.rowptr.data_ptr(), csr.col.data_ptr(), n_rows, L, D, H, dQ, hub, nch, _ptr(ws))
    if plan.edge == 'plain':
        name, args = 'ampconv_bwd_edge_dst', args + (_ptr(spos), _ptr(stats), _ptr(sc.dqkv), plan.dtype)
    else:
        name = 'ampconv_bwd_edge_dst_' + ('planes' if plan.edge == 'planes' else 'scaled')
        args += (sc.bounds.data_ptr(), _ptr(spos), _ptr(stats), sc.dqkv.data_ptr())
    _lib.check(getattr(lib, name)(*args, _stream()), name)
    return stats


def edge_bwd_src(plan, csr, Q, K, V, dO, n_src, dK, dV, stats, sc):
    """dK, dV from the destination pass's statistics (None: its own softmax).  The 'planes' and 'views' passes record
    max |dK | dV| into sc.dqkv as well; the plain fp32 kernels have no register to spare for it (csrc/edge_mfma.hip)."""
    lib = _lib.load()
    L, D, H = plan.L, plan.D, plan.H
    hub, nch, ws = csr.hub_args('src', L, D, 2)
    cinv = () if plan.edge == 'planes' else (csr.cinv.data_ptr(),)
    args = (Q, K, V, dO, csr.cscptr.data_ptr(), csr.crow.data_ptr()) + cinv + (n_src, L, D, H, dK, dV, hub, nch,
                                                                               _ptr(ws))
    if plan.edge == 'plain':
        name, args = 'ampconv_bwd_edge_src', args + (_ptr(stats), None, plan.dtype)
    else:
        name = 'ampconv_bwd_edge_src_' + ('planes' if plan.edge == 'planes' else 'scaled')
        args += (sc.bounds.data_ptr(), _ptr(stats), sc.dqkv.data_ptr())
    _lib.check(getattr(lib, name)(*args, _stream()), name)


class AMPConvFunction(torch.autograd.Function):
    """y = mask(deg>0) * (mean_in-edges(attention) Wo^T + bo), differentiable in
    xq, xkv and the four nn.MultiheadAttention parameters.

    `xq` supplies the query (destination) rows and `xkv` the key/value (source)
    rows; AMPConv.forward passes the same tensor for both, AMPConv.message passes
    the pre-gathered x_i / x_j with an identity graph."""

    @staticmethod
    def forward(ctx, xq, xkv, w_in, b_in, w_out, b_out, csr, num_heads, shared, dtype=_lib.AMPCONV_F32,
                gemm='fp32'):
        lib = _lib.load()
        D = w_out.size(0)
        H = int(num_heads)
        dh = D // H
        L = xq.size(1) // D
        if w_in.dtype != xq.dtype or w_out.dtype != xq.dtype:
            raise ValueError(f'inputs are {xq.dtype} but the parameters are {w_in.dtype}: storage is all float32 or all '
                             f'bfloat16 (layer.to(torch.bfloat16))')
        if xq.dtype == torch.bfloat16:                   # bf16 storage: one mode only
            if not ((dh in (16, 32) and L <= 20) or (dh % 2 == 0 and dh <= 64 and L <= 64)):
                raise ValueError(f'bf16 storage is implemented for head dimensions 32 and 16 with at most 20 tokens per '
                                 f'node (csrc/edge_mfma_bf16.hip; BASELINE configs 5 and 3) and for even head dimensions '
                                 f'up to 64 with at most 64 tokens (csrc/edge_block_x3.hip: the workgroup-per-unit kernels on bf16 rows); '
                                 f'got head dimension {dh}, {L} tokens: use float32 for this shape')
        Nq, Nk = xq.size(0), xkv.size(0)
        xq2 = xq.contiguous().view(Nq * L, D)
        with torch.cuda.device(xq.device), gemm_precision(gemm):
            xkv2 = xq2 if shared else xkv.contiguous().view(Nk * L, D)
            maxima = {}
            plan = choose_plan(L, D, H, shared, xq.dtype, gemm, xq2.numel(), _verdict(xq2, xq, maxima, 'x'),
                               _verdict(xkv2, xkv, maxima, 'xkv'), csr.active_nodes if Nq == csr.num_nodes else None,
                               torch.cuda.is_current_stream_capturing, dtype)
            imgs = None
            if plan.native:      # every weight image this call and its backward need, in one launch
                ws = [w_in, w_out] if shared else [w_in[:D], w_in[D:], w_out]
                imgs = proj_images([(w, False) for w in ws] + [(w, True) for w in ws])
            sc = Scalars.for_forward(plan, maxima.get('x'), maxima.get('xkv'))
            lists = plan.lists
            kv = None
            if plan.edge == 'planes':
                # Q | K | V leave the in-projection as two fp16 planes scaled by a bound known before the product runs
                # (max |x| times the largest absolute row sum of W, plus max |b|)
                proj_out_bound(w_in, False, b_in, sc.x, sc.qkv_bound)
                qkv = proj_rows_planes(xq2, imgs[0], sc.qkv_bound, b_in, amax=sc.x, out_amax=sc.obar, amax_col0=2 * D,
                                       dh=dh)
            elif shared:
                # (node lists: Q rows matter for nodes with in-edges, K / V rows for nodes with out-edges; the rows of
                # nodes with neither are never read by an edge pass and stay unwritten)
                qkv = (proj_rows(xq2, imgs[0], b_in, L=L, nodes=lists and lists['any'], amax=sc.x, out_amax=sc.obar)
                       if plan.native else torch.addmm(b_in, xq2, w_in.t()))              # [N*L, 3D]
            elif plan.native:
                qkv = proj_rows(xq2, imgs[0], b_in[:D], amax=sc.x)
                kv = proj_rows(xkv2, imgs[1], b_in[D:], amax=sc.xkv, out_amax=sc.obar)
            else:
                qkv = torch.addmm(b_in[:D], xq2, w_in[:D].t())         # [Nq*L, D]
                kv = torch.addmm(b_in[D:], xkv2, w_in[D:].t())         # [Nk*L, 2D]
            Qv, Kv, Vv = _qkv_views(qkv, kv, L, D, dh)
            obar = torch.empty(Nq * L, D, dtype=xq.dtype, device=xq.device)
            if plan.edge == 'views':
                sc.v_max.copy_(sc.qkv_bound)                 # (Scalars.for_forward)
            edge_fwd(plan, csr, Qv, Kv, Vv, Nq, obar, sc)
            if lists:       # the rows of the nodes with in-edges; the others are zeroed without being read
                y = proj_rows(obar, imgs[1], b_out, L=L, nodes=lists['in'])
                _zero_unlisted(y, lists['in'], Nq, L)
            elif plan.native:    # bias and the in-degree mask (rows nobody sends to stay exactly 0) in the epilogue
                y = proj_rows(obar, imgs[1 if shared else 2], b_out, csr.rowptr, L, amax=sc.obar)
            else:
                y = torch.addmm(b_out, obar, w_out.t())
                io = _lib.AMPCONV_BF16 if y.dtype == torch.bfloat16 else _lib.AMPCONV_F32
                rc = lib.ampconv_mask_rows(y.data_ptr(), csr.rowptr.data_ptr(), Nq, L * D, io, _stream())
                _lib.check(rc, 'ampconv_mask_rows')
        ctx.set_materialize_grads(False)     # no zero-filled [N*L, 3D] gradient for the qkv side output
        ctx.save_for_backward(xq2, xkv2, w_in, w_out, qkv, kv, obar)
        ctx.csr, ctx.dims, ctx.plan, ctx.scalars = csr, (Nq, Nk), plan, sc
        ctx.images_t = imgs[len(imgs) // 2:] if imgs else None     # the transposed images, for the input gradients
        ctx.mark_non_differentiable(qkv)
        if kv is not None:
            ctx.mark_non_differentiable(kv)
        if plan.edge == 'planes':           # plane format: the third output is what reads `qkv` back (planes_to_f32)
            ctx.mark_non_differentiable(sc.bounds)
            return y.view(Nq, L * D), qkv, sc.bounds
        return y.view(Nq, L * D), qkv, kv

    @staticmethod
    def backward(ctx, dy, _dqkv=None, _dkv=None):
        lib = _lib.load()
        if dy is None:
            return (None,) * 11
        xq2, xkv2, w_in, w_out, qkv, kv, obar = ctx.saved_tensors
        csr, (Nq, Nk), plan, sc = ctx.csr, ctx.dims, ctx.plan, ctx.scalars
        L, D, dh, shared = plan.L, plan.D, plan.dh, plan.shared
        dev = dy.device
        need_xq, need_xkv = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        with torch.cuda.device(dev), gemm_precision(plan.gemm):
            dy2 = dy.contiguous().view(Nq * L, D)
            if plan.scaled:     # (one pass + one read-back per step: gradients are new every step)
                st, narrow = operand_stats(dy2)
                plan = plan.backward(narrow)
                sc = sc.for_backward(st[0:1]) if plan.scaled else Scalars()
            if plan.qkv_to_f32:                 # the saved projections as fp32 for the exact edge passes
                qkv = planes_to_f32(qkv, ctx.scalars.qkv_bound, dh)
            # out-projection: rows with no in-edge contribute nothing (their obar is 0, and
            # the bias gradient masks them explicitly)
            if plan.native:
                dw_out = torch.empty_like(w_out)
                db_out = torch.empty(D, dtype=dy2.dtype, device=dev)
                if plan.lists:   # the listed nodes ARE the ones that pass the mask; dObar is read for destinations only
                    proj_wgrad(dy2, obar, dw_out, db_out, L=L, nodes=plan.lists['in'])
                    dobar = proj_rows(dy2, ctx.images_t[-1], L=L, nodes=plan.lists['in'])
                else:
                    proj_wgrad(dy2, obar, dw_out, db_out, csr.rowptr, L, amax=(sc.dy, sc.obar))
                    if plan.edge == 'planes':   # dObar / in-degree as two fp16 planes (the edge passes then carry no
                        proj_out_bound(w_out, True, None, sc.dy, sc.dobar_bound)        # per-edge weight)
                        sc.dobar_max.zero_()
                        dobar = proj_rows_planes(dy2, ctx.images_t[-1], sc.dobar_bound, rowptr=csr.rowptr, L=L,
                                                 row_scale=1, amax=sc.dy, out_amax=sc.dobar_max, dh=dh)
                    elif plan.edge == 'views':  # fp32 dObar, its maximum recorded by the product that writes it
                        sc.dobar_bound.zero_()
                        dobar = proj_rows(dy2, ctx.images_t[-1], amax=sc.dy, out_amax=sc.dobar_bound)
                        sc.dobar_max.copy_(sc.dobar_bound)       # (Scalars.for_forward)
                    else:
                        dobar = proj_rows(dy2, ctx.images_t[-1], amax=sc.dy)
            else:
                scratch = torch.empty((1 + _lib.COLSUM_BLOCKS) * D, dtype=torch.float32, device=dev)
                io = _lib.AMPCONV_BF16 if dy2.dtype == torch.bfloat16 else _lib.AMPCONV_F32
                rc = lib.ampconv_masked_colsum(dy2.data_ptr(), csr.rowptr.data_ptr(), Nq, L, D,
                                               scratch.data_ptr(), io, _stream())
                _lib.check(rc, 'ampconv_masked_colsum')
                db_out = scratch[:D].to(dy2.dtype)
                dw_out = _tn_matmul(dy2, obar)
                dobar = dy2.mm(w_out)                                      # [Nq*L, D]
            dOv = _view(dobar, 0, L, dh)
            dqkv = torch.empty(Nq * L, (3 if shared else 1) * D, dtype=dy2.dtype, device=dev)
            dkv = None if shared else torch.empty(Nk * L, 2 * D, dtype=dy2.dtype, device=dev)
            Qv, Kv, Vv = _qkv_views(qkv, kv, L, D, dh)
            dQv, dKv, dVv = _qkv_views(dqkv, dkv, L, D, dh)
            stats = edge_bwd_dst(plan, csr, Qv, Kv, Vv, dOv, Nq, dQv, sc)
            edge_bwd_src(plan, csr, Qv, Kv, Vv, dOv, Nk, dKv, dVv, stats, sc)
            if plan.scaled and plan.edge == 'plain':
                # (the operand maximum of the two products that consume dQKV: max |dQ| came from the destination pass,
                # dK | dV take one pass here; shared: one maximum, else dQ and dK | dV apart)
                if shared:
                    absmax(dqkv[:, D:], sc.dqkv)                # merged into the maximum of dQ
                else:
                    sc.dkv = absmax(dkv)
            # in_proj_bias gradient without a pass over all of dQKV: softmax rows sum to 1, so the
            # column sum of dV over every source token equals the column sum of dObar over the rows
            # that receive messages, and dObar = dY Wo is linear in dY, so that sum is (masked column sum of
            # dY) Wo = db_out Wo: a [D] x [D, D] product instead of a second 20 GB reduction pass.  The K bias
            # shifts every score of a row equally, i.e. has gradient exactly 0 (torch's autograd returns ~1e-9 noise)
            db_v = None
            if shared and dy2.dtype == torch.float32 and not plan.native:
                db_v = scratch[:D] @ w_out
            del dobar, stats
            if plan.native:
                # weight and bias gradients in one pass each (the column sums ride on the rows the product reads
                # anyway: all three thirds of in_proj_bias.grad are the true sums, as autograd's are)
                dw_in = torch.empty_like(w_in)
                db_in = torch.empty(3 * D, dtype=dy2.dtype, device=dev)
                if plan.lists:   # the dQKV rows of a node without any edge are zeros (both edge passes wrote them)
                    proj_wgrad(dqkv, xq2, dw_in, db_in, L=L, nodes=plan.lists['any'])
                    dxq = dxkv = None
                    if need_xq:
                        dxq2 = proj_rows(dqkv, ctx.images_t[0], L=L, nodes=plan.lists['any'])
                        _zero_unlisted(dxq2, plan.lists['any'], Nq, L)
                        dxq = dxq2.view(Nq, L * D)
                elif shared:
                    proj_wgrad(dqkv, xq2, dw_in, db_in, amax=(sc.dqkv, sc.x))
                    dxq = proj_rows(dqkv, ctx.images_t[0], amax=sc.dqkv).view(Nq, L * D) if need_xq else None
                    dxkv = None
                else:
                    proj_wgrad(dqkv, xq2, dw_in[:D], db_in[:D], amax=(sc.dqkv, sc.x))
                    proj_wgrad(dkv, xkv2, dw_in[D:], db_in[D:], amax=(sc.dkv, sc.xkv))
                    dxq = proj_rows(dqkv, ctx.images_t[0], amax=sc.dqkv).view(Nq, L * D) if need_xq else None
                    dxkv = proj_rows(dkv, ctx.images_t[1], amax=sc.dkv).view(Nk, L * D) if need_xkv else None
            elif shared:
                dw_in = _tn_matmul(dqkv, xq2)
                if db_v is not None:
                    db_in = torch.cat([dqkv[:, :D].sum(dim=0), torch.zeros_like(db_v), db_v])
                else:
                    db_in = dqkv.sum(dim=0)
                dxq = dqkv.mm(w_in).view(Nq, L * D) if need_xq else None
                dxkv = None
            else:
                dw_in = torch.cat([_tn_matmul(dqkv, xq2), _tn_matmul(dkv, xkv2)], dim=0)
                db_in = torch.cat([dqkv.sum(dim=0), dkv.sum(dim=0)])
                dxq = dqkv.mm(w_in[:D]).view(Nq, L * D) if need_xq else None
                dxkv = dkv.mm(w_in[D:]).view(Nk, L * D) if need_xkv else None
        return dxq, dxkv, dw_in, db_in, dw_out, db_out, None, None, None, None, None


def attention_weights(Qv, Kv, edge_index, L, D, H):
    """[E, L, L] head-averaged softmax weights in ORIGINAL edge order
    (amp_conv.py:39,43-47; torch functional.py:6604-6606)."""
    lib = _lib.load()
    E = edge_index.size(1)
    W = torch.empty(E, L, L, dtype=torch.float32, device=edge_index.device)
    with torch.cuda.device(edge_index.device):
        rc = lib.ampconv_attn_weights(Qv, Kv, edge_index.data_ptr(), E, L, D, H, W.data_ptr(),
                                      _lib.AMPCONV_F32, _stream())
    _lib.check(rc, 'ampconv_attn_weights')
    return W


class SegmentMeanFunction(torch.autograd.Function):
    """PyG aggr='mean' of an [E, F] message matrix over the dst-sorted CSR; differentiable in the
    messages (d msg[e] = d out[dst(e)] / in-degree(dst(e))), so the decomposed public path
    message() -> aggregate() trains like the fused propagate()."""

    @staticmethod
    def forward(ctx, msg, csr, index):
        lib = _lib.load()
        msg = msg.contiguous()
        N, F = csr.num_nodes, msg.size(1)
        out = torch.empty(N, F, dtype=torch.float32, device=msg.device)
        with torch.cuda.device(msg.device):
            rc = lib.ampconv_segment_mean(msg.data_ptr(), csr.rowptr.data_ptr(), csr.eperm.data_ptr(),
                                          N, F, out.data_ptr(), _stream())
        _lib.check(rc, 'ampconv_segment_mean')
        ctx.csr, ctx.index = csr, index
        return out

    @staticmethod
    def backward(ctx, dout):
        csr = ctx.csr
        deg = (csr.rowptr[1:] - csr.rowptr[:-1]).clamp(min=1).to(dout.dtype)
        return (dout / deg[:, None]).index_select(0, ctx.index), None, None


def segment_mean(msg, csr, index=None):
    """PyG aggr='mean' of an [E, F] message matrix over the dst-sorted CSR.  `index` (the int64
    destination of every message, original order) is needed only for the gradient."""
    if index is None:
        if msg.requires_grad and torch.is_grad_enabled():
            raise ValueError('segment_mean of messages that require grad needs `index`')
        index = torch.empty(0, dtype=torch.int64, device=msg.device)
    return SegmentMeanFunction.apply(msg, csr, index)
