"""Fused AMPConv forward/backward on MI355X: projections as dense GEMMs on the
per-NODE rows (projection.py: one Projections object per call, libampconv's kernels or library GEMMs), edge phase in
hand-written HIP through the C ABI.  AMPConvFunction reads: plan -> scalars -> in-projection -> edge_fwd ->
out-projection; out-projection backward -> edge_bwd_dst / edge_bwd_src -> in-projection backward.

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
import dataclasses
import os

import torch

from .. import _lib
from .._lib import ptr as _ptr
from ..graph import EdgeCSR, _stream
from .projection import (Projections, _aligned, _tn_matmul, gemm_precision, mask_rows, masked_colsum,  # noqa: F401
                         proj_image, proj_images, proj_native, proj_rows, proj_wgrad)


def _view(buf2d, col_off, L, dh):
    """ampconv_view_t over columns [col_off, col_off + D) of a contiguous [rows*L, W] buffer."""
    assert buf2d.is_contiguous() and buf2d.dtype in (torch.float32, torch.bfloat16)
    W = buf2d.size(1)
    return _lib.View(buf2d.data_ptr() + buf2d.element_size() * col_off, L * W, W, dh)


# hand the softmax statistics of the destination pass to the source pass (AMPCONV_SOFTMAX_STATS=0:
# both passes reduce their own; used by the tests to cross-check the two ways)
SOFTMAX_STATS = os.environ.get('AMPCONV_SOFTMAX_STATS', '1') != '0'
# ---- the switches of the per-node projections (projection.py; their kernels: csrc/proj_gemm.hip, csrc/proj_gemm_bf16.hip)
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
    _lib.check(lib.ampconv_absmax(t2.data_ptr(), t2.stride(0), t2.size(0), t2.size(1), _lib.DTYPES[t2.dtype], out.data_ptr(),
                                  1 if reset else 0, _stream()), 'ampconv_absmax')
    return out


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
            # (weights: in-projection [, its K | V part], out-projection; native: every image this call and its
            # backward need, in one launch)
            proj = Projections(plan.native, [w_in, w_out] if shared else [w_in[:D], w_in[D:], w_out])
            sc = Scalars.for_forward(plan, maxima.get('x'), maxima.get('xkv'))
            lists = plan.lists
            kv = None
            if plan.edge == 'planes':
                # Q | K | V leave the in-projection as two fp16 planes scaled by a bound known before the product runs
                # (max |x| times the largest absolute row sum of W, plus max |b|)
                proj_out_bound(w_in, False, b_in, sc.x, sc.qkv_bound)
                qkv = proj_rows_planes(xq2, proj.image(0), sc.qkv_bound, b_in, amax=sc.x, out_amax=sc.obar,
                                       amax_col0=2 * D, dh=dh)
            elif shared:
                # (node lists: Q rows matter for nodes with in-edges, K / V rows for nodes with out-edges; the rows of
                # nodes with neither are never read by an edge pass and stay unwritten)
                qkv = proj.forward(0, xq2, b_in, nodes=lists and lists['any'], L=L, amax=sc.x,
                                   out_amax=sc.obar)                                      # [N*L, 3D]
            else:
                qkv = proj.forward(0, xq2, b_in[:D], amax=sc.x)                           # [Nq*L, D]
                kv = proj.forward(1, xkv2, b_in[D:], amax=sc.xkv, out_amax=sc.obar)       # [Nk*L, 2D]
            Qv, Kv, Vv = _qkv_views(qkv, kv, L, D, dh)
            obar = torch.empty(Nq * L, D, dtype=xq.dtype, device=xq.device)
            if plan.edge == 'views':
                sc.v_max.copy_(sc.qkv_bound)                 # (Scalars.for_forward)
            edge_fwd(plan, csr, Qv, Kv, Vv, Nq, obar, sc)
            # bias and the in-degree mask: rows nobody sends to stay exactly 0 (node lists: the rows of the nodes with
            # in-edges are computed, the others are zeroed without being read)
            dst = lists and lists['in']
            y = proj.forward(-1, obar, b_out, mask=(dst[2] if dst else csr.rowptr, Nq), nodes=dst, L=L, amax=sc.obar)
        ctx.set_materialize_grads(False)     # no zero-filled [N*L, 3D] gradient for the qkv side output
        ctx.save_for_backward(xq2, xkv2, w_in, w_out, qkv, kv, obar)
        ctx.csr, ctx.dims, ctx.plan, ctx.scalars, ctx.proj = csr, (Nq, Nk), plan, sc, proj
        ctx.mark_non_differentiable(qkv)
        if kv is not None:
            ctx.mark_non_differentiable(kv)
        if plan.edge == 'planes':           # plane format: the third output is what reads `qkv` back (planes_to_f32)
            ctx.mark_non_differentiable(sc.bounds)
            return y.view(Nq, L * D), qkv, sc.bounds
        return y.view(Nq, L * D), qkv, kv

    @staticmethod
    def backward(ctx, dy, _dqkv=None, _dkv=None):
        if dy is None:
            return (None,) * 11
        xq2, xkv2, w_in, w_out, qkv, kv, obar = ctx.saved_tensors
        csr, (Nq, Nk), plan, sc, proj = ctx.csr, ctx.dims, ctx.plan, ctx.scalars, ctx.proj
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
            dst, both = (plan.lists['in'], plan.lists['any']) if plan.lists else (None, None)
            # out-projection: rows with no in-edge contribute nothing (their obar is 0, and the bias gradient masks them
            # explicitly; node lists: the listed nodes ARE the ones that pass the mask)
            dw_out = torch.empty_like(w_out)
            db_out = torch.empty(D, dtype=dy2.dtype, device=dev)
            proj.weight_grad([(dy2, obar, (sc.dy, sc.obar))], dw_out, db_out, mask=None if dst else (csr.rowptr, Nq),
                             nodes=dst, L=L)
            if plan.edge == 'planes':   # dObar / in-degree as two fp16 planes (the edge passes then carry no per-edge
                proj_out_bound(w_out, True, None, sc.dy, sc.dobar_bound)                                  # weight)
                sc.dobar_max.zero_()
                dobar = proj_rows_planes(dy2, proj.image(-1, True), sc.dobar_bound, rowptr=csr.rowptr, L=L, row_scale=1,
                                         amax=sc.dy, out_amax=sc.dobar_max, dh=dh)
            elif plan.edge == 'views':  # fp32 dObar, its maximum recorded by the product that writes it
                sc.dobar_bound.zero_()
                dobar = proj.input_grad(-1, dy2, amax=sc.dy, out_amax=sc.dobar_bound)
                sc.dobar_max.copy_(sc.dobar_bound)       # (Scalars.for_forward)
            else:                       # (node lists: dObar is read for destinations only; the other rows stay unwritten)
                dobar = proj.input_grad(-1, dy2, nodes=dst, L=L, amax=sc.dy)         # [Nq*L, D]
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
            del dobar, stats
            # in-projection: weight and bias gradients in one pass each on the native side (the column sums ride on the
            # rows the product reads anyway: all three thirds of in_proj_bias.grad are the true sums, as autograd's
            # are; node lists: the dQKV rows of a node without any edge are zeros, both edge passes wrote them)
            dw_in = torch.empty_like(w_in)
            db_in = torch.empty(3 * D, dtype=dy2.dtype, device=dev)
            terms = [(dqkv, xq2, (sc.dqkv, sc.x))] + ([] if shared else [(dkv, xkv2, (sc.dkv, sc.xkv))])
            # fp32 library GEMMs, self-attention: in_proj_bias gradient without a pass over all of dQKV.  Softmax rows
            # sum to 1, so the column sum of dV over every source token equals the column sum of dObar over the rows
            # that receive messages, and dObar = dY Wo is linear in dY, so that sum is (masked column sum of dY) Wo =
            # db_out Wo: a [D] x [D, D] product instead of a second 20 GB reduction pass.  The K bias shifts every score
            # of a row equally, i.e. has gradient exactly 0 (torch's autograd returns ~1e-9 noise)
            shortcut = shared and dy2.dtype == torch.float32 and not plan.native
            db_v = db_out @ w_out if shortcut else None
            proj.weight_grad(terms, dw_in, None if shortcut else db_in, nodes=both, L=L)
            if shortcut:
                torch.cat([dqkv[:, :D].sum(dim=0), torch.zeros_like(db_v), db_v], out=db_in)
            dxq = dxkv = None
            if need_xq:
                dxq = proj.input_grad(0, dqkv, mask=both and (both[2], Nq), nodes=both, L=L,
                                      amax=sc.dqkv).view(Nq, L * D)
            if need_xkv and not shared:
                dxkv = proj.input_grad(1, dkv, amax=sc.dkv).view(Nk, L * D)
        return dxq, dxkv, dw_in, db_in, dw_out, db_out, None, None, None, None, None


def token_supported(L, D, H, dtype):
    """Do the one-query-token edge kernels (csrc/edge_token.hip) serve this shape at this storage dtype?"""
    return dtype in _lib.DTYPES and bool(_lib.load().ampconv_token_supported(L, D, H, _lib.DTYPES[dtype]))


def _token_view(buf2d, dh):
    """ampconv_view_t of a contiguous one-token tensor [N, D]: element (n, h, c) at n * D + h * dh + c."""
    assert buf2d.is_contiguous() and buf2d.dtype in (torch.float32, torch.bfloat16)
    return _lib.View(buf2d.data_ptr(), buf2d.size(1), buf2d.size(1), dh)


class AMPConvTokenFunction(torch.autograd.Function):
    """AMPConvFunction for ONE query token per node: y [N, D] = mask(deg>0) * (mean_in-edges(attention of the query row
    xq_tok[d] over the L tokens of xkv[s]) Wo^T + bo) -- what `AMPConvFunction(x, x, ...)[:, token]` computes when xq_tok is
    token `token` of x, without the Q projection, the out-projection and their gradients over the other L - 1 query rows,
    and without the [N, L*D] output.  Differentiable in xq_tok [N, D], xkv [N, L*D] and the four parameters.  The K | V
    projection and the per-edge gather of the source's K and V tiles are those of the full layer; the edge passes are
    ampconv_*_edge_token (include/ampconv.h).  Projections in the plain fp32 / bf16 modes (no scaled or plane operands);
    bf16 storage with 16 <= L <= 128: the N*L-row products run over the nodes with out-edges only (node lists)."""

    @staticmethod
    def forward(ctx, xq_tok, xkv, w_in, b_in, w_out, b_out, csr, num_heads, gemm='fp32'):
        D = w_out.size(0)
        H = int(num_heads)
        dh = D // H
        N, L = xkv.size(0), xkv.size(1) // D
        if w_in.dtype != xkv.dtype or w_out.dtype != xkv.dtype or xq_tok.dtype != xkv.dtype:
            raise ValueError(f'inputs are {xq_tok.dtype} / {xkv.dtype} but the parameters are {w_in.dtype}: storage is all '
                             f'float32 or all bfloat16 (layer.to(torch.bfloat16))')
        if xq_tok.shape != (N, D):
            raise ValueError(f'xq_tok must be [{N}, {D}], got {tuple(xq_tok.shape)}')
        if not token_supported(L, D, H, xkv.dtype):
            raise ValueError(f'the one-query-token kernels do not serve L = {L}, head dimension {dh}, {xkv.dtype} '
                             f'(ampconv_token_supported): use the full layer and a slice')
        code = _lib.DTYPES[xkv.dtype]
        lib = _lib.load()
        with torch.cuda.device(xkv.device), gemm_precision(gemm):
            xkv2 = xkv.contiguous().view(N * L, D)
            native = proj_native(gemm, xkv.dtype, D)
            out_nodes = None
            if NODE_LISTS and native and xkv.dtype == torch.bfloat16 and 16 <= L <= 128 and N == csr.num_nodes:
                lists = csr.active_nodes()
                out_nodes = lists and lists['out']
            proj = Projections(native, [w_in[:D], w_in[D:], w_out])
            q = proj.forward(0, xq_tok, b_in[:D])                                          # [N, D]
            # (node lists: K / V rows matter for nodes with out-edges; the others are never read and stay unwritten)
            kv = proj.forward(1, xkv2, b_in[D:], nodes=out_nodes, L=L)                     # [N*L, 2D]
            obar = torch.empty(N, D, dtype=xkv.dtype, device=xkv.device)
            hub, nch, ws = csr.hub_args('dst', 1, D, 1)
            _lib.check(lib.ampconv_fwd_edge_token(_token_view(q, dh), _view(kv, 0, L, dh), _view(kv, D, L, dh),
                                                  csr.rowptr.data_ptr(), csr.col.data_ptr(), N, L, D, H,
                                                  _token_view(obar, dh), hub, nch, _ptr(ws), code, _stream()),
                       'ampconv_fwd_edge_token')
            # bias and the in-degree mask: rows nobody sends to stay exactly 0
            y = proj.forward(-1, obar, b_out, mask=(csr.rowptr, N), L=1)
        ctx.save_for_backward(xq_tok, xkv2, w_in, w_out, q, kv, obar)
        ctx.csr, ctx.dims, ctx.proj, ctx.gemm, ctx.out_nodes, ctx.code = csr, (N, L, D, H), proj, gemm, out_nodes, code
        return y

    @staticmethod
    def backward(ctx, dy):
        xq_tok, xkv2, w_in, w_out, q, kv, obar = ctx.saved_tensors
        csr, (N, L, D, H), proj, out_nodes, code = ctx.csr, ctx.dims, ctx.proj, ctx.out_nodes, ctx.code
        dh = D // H
        dev = dy.device
        lib = _lib.load()
        with torch.cuda.device(dev), gemm_precision(ctx.gemm):
            dy2 = dy.contiguous()
            # out-projection: rows with no in-edge contribute nothing (their obar is 0, the bias gradient masks them)
            dw_out = torch.empty_like(w_out)
            db_out = torch.empty(D, dtype=dy2.dtype, device=dev)
            proj.weight_grad([(dy2, obar, None)], dw_out, db_out, mask=(csr.rowptr, N), L=1)
            dobar = proj.input_grad(-1, dy2)                                               # [N, D]
            dq = torch.empty(N, D, dtype=dy2.dtype, device=dev)
            dkv = torch.empty(N * L, 2 * D, dtype=dy2.dtype, device=dev)
            Qv, Kv, Vv, dOv = _token_view(q, dh), _view(kv, 0, L, dh), _view(kv, D, L, dh), _token_view(dobar, dh)
            hub, nch, ws = csr.hub_args('dst', 1, D, 1)
            _lib.check(lib.ampconv_bwd_edge_dst_token(Qv, Kv, Vv, dOv, csr.rowptr.data_ptr(), csr.col.data_ptr(), N, L, D, H,
                                                      _token_view(dq, dh), hub, nch, _ptr(ws), code, _stream()),
                       'ampconv_bwd_edge_dst_token')
            hub, nch, ws = csr.hub_args('src', L, D, 2)
            _lib.check(lib.ampconv_bwd_edge_src_token(Qv, Kv, Vv, dOv, csr.cscptr.data_ptr(), csr.crow.data_ptr(),
                                                      csr.cinv.data_ptr(), N, L, D, H, _view(dkv, 0, L, dh),
                                                      _view(dkv, D, L, dh), hub, nch, _ptr(ws), code, _stream()),
                       'ampconv_bwd_edge_src_token')
            del dobar, ws
            # in-projection: the Q third from the N-row term, the K | V thirds from the N*L-row term; all three thirds of
            # db_in are the true column sums (rows without edges are exact zeros, both passes wrote them)
            dw_in = torch.empty_like(w_in)
            db_in = torch.empty(3 * D, dtype=dy2.dtype, device=dev)
            proj.weight_grad([(dq, xq_tok, None)], dw_in[:D], db_in[:D])
            proj.weight_grad([(dkv, xkv2, None)], dw_in[D:], db_in[D:], nodes=out_nodes, L=L)
            dxq = dxkv = None
            if ctx.needs_input_grad[0]:
                dxq = proj.input_grad(0, dq)
            if ctx.needs_input_grad[1]:
                dxkv = proj.input_grad(1, dkv, mask=out_nodes and (out_nodes[2], N), nodes=out_nodes, L=L).view(N, L * D)
        return dxq, dxkv, dw_in, db_in, dw_out, db_out, None, None, None


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
