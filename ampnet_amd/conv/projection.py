"""The per-node dense products of a layer call -- in-projection, masked out-projection, their weight / bias gradients
and input gradients -- behind one object, `Projections`, for the three autograd functions (functional.AMPConvFunction,
linear.LinearAMPConvFunction, partitioned._PartitionedFunction).  It is the one place that decides between libampconv's
own kernels (the proj_* wrappers below; csrc/proj_gemm.hip, csrc/proj_gemm_bf16.hip) and library GEMMs, and the one
place that calls ampconv_mask_rows / ampconv_masked_colsum.

What it replaces in the reference: torch functional.py:5785-5862 (`_in_projection_packed`, per edge there, per node
here), :6600 (out-projection) and their autograd backward."""
import contextlib
import ctypes
import os
import threading

import torch

from .. import _lib
from .._lib import ptr as _ptr
from ..graph import _stream

GEMM_PRECISIONS = ('native', 'fp32', 'bf16x3')
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


def _tn_matmul(a, b, chunks=128, out=None):
    """a^T @ b for tall operands a [M, p], b [M, q] (the weight-gradient GEMMs, reduction over
    the N*L node-token rows).  rocBLAS runs the single [p, M] x [M, q] product at 65-95 TFLOP/s
    at M = 2e7; splitting the reduction into `chunks` batched GEMMs + one sum runs at
    ~150 TFLOP/s (measured on MI355X, tools/bench_dw.py) and sums pairwise, i.e. more accurately.
    out: a contiguous [p, q] tensor (or row block of one) that receives the product."""
    M = a.size(0)
    if M < (1 << 18):
        return torch.mm(a.t(), b, out=out)
    per = M // chunks
    main = per * chunks
    out = torch.sum(torch.bmm(a[:main].view(chunks, per, -1).transpose(1, 2), b[:main].view(chunks, per, -1)), 0,
                    out=out)
    if main < M:
        out += a[main:].t().mm(b[main:])
    return out


# ---- the per-node projections in libampconv.so.  fp32 storage (csrc/proj_gemm.hip): operands scaled by a power of two
# and split into two fp16 planes, three partial products on v_mfma_f32_32x32x16_f16 (large operands; functional.PROJ_SCALED),
# or split exactly into three bf16 terms, six partial products on v_mfma_f32_32x32x16_bf16; fp32 accumulate.  bf16 storage
# (csrc/proj_gemm_bf16.hip): one product, fp32 accumulate, one rounding on the way out
def proj_native(gemm, dtype, D):
    """Does the 'native' mode serve this layer?  fp32 storage with embed_dim a multiple of 4, bf16 storage with a
    multiple of 8 (rows move in 16-byte pieces)."""
    return (gemm == 'native' and dtype in _lib.DTYPES
            and bool(_lib.load().ampconv_proj_supported(D, D, _lib.DTYPES[dtype])))


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
    code = _lib.DTYPES[wdt]
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
                                     _lib.DTYPES[wdt], _stream()), 'ampconv_proj_rows')
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
    code = _lib.DTYPES[a2.dtype]
    ids, cnt = (nodes[0].data_ptr(), nodes[1]) if nodes is not None else (None, 0)
    nws = lib.ampconv_proj_wgrad_workspace_bytes(cnt * L if nodes is not None else M, Na, Nb, code)
    ws = torch.empty(max(nws, 16) // 4, dtype=torch.float32, device=a2.device)
    _lib.check(lib.ampconv_proj_wgrad(a2.data_ptr(), a2.stride(0), b2.data_ptr(), b2.stride(0), M, Na, Nb,
                                      _ptr(rowptr), L, dw.data_ptr(), _ptr(colsum), ws.data_ptr(), nws, ids, cnt,
                                      _ptr(amax[0]) if amax else None, _ptr(amax[1]) if amax else None, code,
                                      _stream()), 'ampconv_proj_wgrad')


def mask_rows(t2, ptr, n_nodes, L):
    """Zero, in place, the L rows of every node whose segment of the CSR-shaped `ptr` is empty: a graph's rowptr (nodes
    without an in-edge) or the `ptr` of a node list (the nodes it leaves out: include/ampconv.h, ampconv_active_nodes)."""
    assert t2.is_contiguous()
    _lib.check(_lib.load().ampconv_mask_rows(t2.data_ptr(), ptr.data_ptr(), n_nodes, L * t2.size(1), _lib.DTYPES[t2.dtype],
                                             _stream()), 'ampconv_mask_rows')


def masked_colsum(dy2, rowptr, n_nodes, L, out):
    """out[D] = column sums of dy2 [n_nodes * L, D] over the rows of the nodes with an in-edge (summed in fp32; copied
    out of the call's scratch, so that `out` does not keep its (1 + COLSUM_BLOCKS) * D floats alive)."""
    assert dy2.is_contiguous()
    D = out.numel()
    scratch = torch.empty((1 + _lib.COLSUM_BLOCKS) * D, dtype=torch.float32, device=dy2.device)
    _lib.check(_lib.load().ampconv_masked_colsum(dy2.data_ptr(), rowptr.data_ptr(), n_nodes, L, D, scratch.data_ptr(),
                                                 _lib.DTYPES[dy2.dtype], _stream()), 'ampconv_masked_colsum')
    out.copy_(scratch[:D])


class Projections:
    """The dense products of one layer call over `weights` = [W_0, W_1, ...] (views such as w_in[:D] allowed), on
    libampconv's kernels (`native`) or as library GEMMs.  native: ONE launch builds the images of every weight and of
    its transpose; the object goes on ctx and so keeps that one buffer for the backward pass.

    Arguments the operations share.  mask = (ptr, n_nodes): rows of nodes whose `ptr` segment is empty are zeroed (rows
    product) or left out of the sums (weight_grad), L rows per node.  nodes: a node list of EdgeCSR.active_nodes (bf16
    storage, native only): only the listed nodes' rows are computed / summed; with `mask` (the list's own ptr) the other
    rows are zeroed, without it they stay unwritten.  amax / out_amax: the scaled mode's operand maxima (proj_rows,
    proj_wgrad; native only)."""

    def __init__(self, native, weights):
        self.native, self.weights = native, weights
        self.images = proj_images([(w, t) for t in (False, True) for w in weights]) if native else None

    def image(self, i, transpose=False):
        """Weight i's image (i = -1: the last, the out-projection), also for the plane-format entry points
        (functional.proj_rows_planes)."""
        n = len(self.weights)
        return self.images[i % n + n * transpose]

    def _rows(self, i, transpose, a2, bias, mask, nodes, L, amax, out_amax):
        if not self.native:
            assert nodes is None
            W = self.weights[i]
            y = a2.mm(W) if transpose else torch.addmm(bias, a2, W.t())
        elif nodes is None:      # bias and mask in the kernel's epilogue: masked rows are exactly 0
            return proj_rows(a2, self.image(i, transpose), bias, mask and mask[0], L, amax=amax, out_amax=out_amax)
        else:
            y = proj_rows(a2, self.image(i, transpose), bias, L=L, nodes=nodes, amax=amax, out_amax=out_amax)
        if mask:
            mask_rows(y, *mask, L)
        return y

    def forward(self, i, x2, bias, *, mask=None, nodes=None, L=0, amax=None, out_amax=None):
        """x2 @ W_i^T + bias."""
        return self._rows(i, False, x2, bias, mask, nodes, L, amax, out_amax)

    def input_grad(self, i, g2, *, mask=None, nodes=None, L=0, amax=None, out_amax=None, into=None):
        """g2 @ W_i; into: a gradient of the same input to add it to (in place; returned)."""
        if into is None:
            return self._rows(i, True, g2, None, mask, nodes, L, amax, out_amax)
        assert mask is None and nodes is None
        if self.native:
            return into.add_(proj_rows(g2, self.image(i, True), amax=amax))
        return into.addmm_(g2, self.weights[i])

    def weight_grad(self, terms, dw, colsum, *, mask=None, nodes=None, L=0):
        """Caller-owned dw = the products g2^T @ x2 of terms = [(g2, x2, amax = (g2's, x2's) or None), ...] stacked by
        rows (the parts of a packed weight), colsum = the column sums of the g2 likewise; colsum None on the GEMM side:
        the caller has the sums from elsewhere."""
        if self.native:
            r = 0
            for g2, x2, amax in terms:
                n = g2.size(1)
                proj_wgrad(g2, x2, dw[r:r + n], colsum[r:r + n], mask and mask[0], L, nodes, amax)
                r += n
            return
        assert nodes is None
        if len(terms) == 1:
            (g2, x2, _), = terms
            if mask and colsum is not None:
                masked_colsum(g2, *mask, L, colsum)
            _tn_matmul(g2, x2, out=dw)
            if not mask and colsum is not None:
                torch.sum(g2, 0, out=colsum)
        else:
            assert not mask
            torch.cat([_tn_matmul(g2, x2) for g2, x2, _ in terms], out=dw)
            if colsum is not None:
                torch.cat([g2.sum(dim=0) for g2, _, _ in terms], out=colsum)
