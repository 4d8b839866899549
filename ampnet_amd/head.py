"""The classifier head behind the token readout and the GraphSAINT-weighted NLL loss, fused (csrc/head.hip).

The reference's model ends in nn.Linear -> log_softmax (src/ampnet/module/amp_gcn.py:272-276; the sigmoid with
softmax_out=False) and every training loop follows it with
    loss = (F.nll_loss(out, y, reduction='none') * node_norm)[mask].sum()
    acc  = (out.argmax(1) == y)[mask].float().mean()
(experiments/cora_benchmark_graphsaint.py:105-128, once per mask): a dozen launches over [N, C], a `nonzero` behind every
boolean index -- a device synchronisation -- and two read-backs per step.  Here the head is one kernel per direction
(`classifier_head`), and the loss with the metrics of up to four masks is one kernel per direction (`saint_nll_loss`) that
never forms [N, C] in memory, takes the upstream gradient from the device and leaves its sums in a device buffer
(`HeadMetrics`) that the caller reads when it likes: no synchronisation per step.  The contract is include/ampconv.h,
"classifier head".  There is no eager fallback: what the kernels do not take raises ValueError.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr as _ptr
from .graph import _stream

OUTPUTS = {'log_softmax': 0, 'sigmoid': 1}                  # AMPCONV_HEAD_* of include/ampconv.h
MAX_CLASSES, MAX_MASKS, METRICS_SLOTS, LOSS_SHIFT = 64, 4, 13, 32
_SUPPORTED = ('supported: pooled [N, D] float32 or bfloat16 on the GPU, weight [C, D] and bias [C] float32 on the same '
              f'device, 1 <= C <= {MAX_CLASSES} (ampnet_amd has no CPU fallback)')


def _check_head(pooled, weight, bias, what):
    for name, t in (('pooled', pooled), ('weight', weight), ('bias', bias)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f'{what}: {name} has to be a tensor on the GPU; {_SUPPORTED}')
    if pooled.dtype not in _lib.DTYPES:
        raise ValueError(f'{what}: pooled is {pooled.dtype}; {_SUPPORTED}')
    if weight.dtype != torch.float32 or bias.dtype != torch.float32:
        raise ValueError(f'{what}: weight is {weight.dtype}, bias is {bias.dtype}; {_SUPPORTED}')
    if pooled.dim() != 2 or weight.dim() != 2 or bias.dim() != 1 or pooled.size(1) < 1 or \
            weight.size(1) != pooled.size(1) or bias.size(0) != weight.size(0):
        raise ValueError(f'{what}: shapes pooled {tuple(pooled.shape)}, weight {tuple(weight.shape)}, bias '
                         f'{tuple(bias.shape)} do not fit; {_SUPPORTED}')
    if not 1 <= weight.size(0) <= MAX_CLASSES:
        raise ValueError(f'{what}: {weight.size(0)} classes; {_SUPPORTED}')
    if weight.device != pooled.device or bias.device != pooled.device:
        raise ValueError(f'{what}: pooled, weight and bias are on different devices; {_SUPPORTED}')


def _rows(pooled):
    """(pooled as the kernels read it, its row stride): unit stride inside a row and rows at least D apart -- such a
    row-strided view is read in place, anything else is copied."""
    N, D = pooled.shape
    if N <= 1:
        return pooled.contiguous(), D
    if pooled.stride(1) != 1 or pooled.stride(0) < D:
        pooled = pooled.contiguous()
    return pooled, pooled.stride(0)


def _workspace(lib, N, D, C, device):
    return torch.empty(max(int(lib.ampconv_head_workspace_bytes(N, D, C)), 16), dtype=torch.uint8, device=device)


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, weight, bias, kind):
        lib = _lib.load()
        pooled, stride = _rows(pooled)
        weight, bias = weight.contiguous(), bias.contiguous()
        N, D = pooled.shape
        C = weight.size(0)
        out = torch.empty(N, C, dtype=torch.float32, device=pooled.device)
        with torch.cuda.device(pooled.device):
            _lib.check(lib.ampconv_head_fwd(pooled.data_ptr(), N, D, stride, weight.data_ptr(), bias.data_ptr(), C, kind,
                                            out.data_ptr(), _lib.DTYPES[pooled.dtype], _stream()), 'ampconv_head_fwd')
        ctx.save_for_backward(pooled, weight, out)
        ctx.args = (kind, stride)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        lib = _lib.load()
        pooled, weight, out = ctx.saved_tensors
        kind, stride = ctx.args
        N, D = pooled.shape
        C = weight.size(0)
        dout = dout.contiguous().float()
        dpooled = torch.empty(N, D, dtype=pooled.dtype, device=pooled.device) if ctx.needs_input_grad[0] else None
        dW, db = torch.empty_like(weight), torch.empty(C, dtype=torch.float32, device=weight.device)
        ws = _workspace(lib, N, D, C, pooled.device)
        with torch.cuda.device(pooled.device):
            _lib.check(lib.ampconv_head_bwd(pooled.data_ptr(), N, D, stride, weight.data_ptr(), C, kind, dout.data_ptr(),
                                            out.data_ptr(), _ptr(dpooled), dW.data_ptr(), db.data_ptr(), ws.data_ptr(),
                                            ws.numel(), _lib.DTYPES[pooled.dtype], _stream()), 'ampconv_head_bwd')
        return dpooled, dW, db, None


def classifier_head(pooled, weight, bias, output='log_softmax'):
    """log_softmax(pooled @ weight.T + bias, dim=1) (output='log_softmax') or the sigmoid of it (output='sigmoid'):
    [N, C] float32, one kernel per direction, gradients to pooled (in its dtype), weight and bias; dW and db are bitwise
    reproducible.  pooled [N, D] float32 or bfloat16 (a row-strided view is read in place), weight [C, D] and bias [C]
    float32, C <= 64."""
    _check_head(pooled, weight, bias, 'classifier_head')
    if output not in OUTPUTS:
        raise ValueError(f'output must be one of {sorted(OUTPUTS)}, got {output!r}')
    return _Head.apply(pooled, weight, bias, OUTPUTS[output])


class HeadMetrics:
    """The running sums of saint_nll_loss on the device: per mask the weighted loss sum, the number of selected nodes and
    the number of those the model classifies correctly, plus the labels outside [0, C) that were skipped.  Accumulated in
    place by every call it is handed to; `zero_()` clears it (once per epoch, say); `read()` is the one read-back."""

    def __init__(self, num_masks=1, device='cuda'):
        if not 1 <= int(num_masks) <= MAX_MASKS:
            raise ValueError(f'HeadMetrics holds 1 to {MAX_MASKS} masks, got {num_masks}')
        self.num_masks = int(num_masks)
        self.buffer = torch.zeros(METRICS_SLOTS, dtype=torch.int64, device=device)
        if not self.buffer.is_cuda:
            raise ValueError('HeadMetrics lives on the GPU (ampnet_amd has no CPU fallback)')

    def zero_(self):
        self.buffer.zero_()
        return self

    def read(self):
        """{'loss_sum': [...], 'count': [...], 'correct': [...], 'bad_labels': n} with one entry per mask; synchronises."""
        v = self.buffer.cpu().tolist()
        m = range(self.num_masks)
        return {'loss_sum': [v[3 * i] / float(1 << LOSS_SHIFT) for i in m], 'count': [v[3 * i + 1] for i in m],
                'correct': [v[3 * i + 2] for i in m], 'bad_labels': v[METRICS_SLOTS - 1]}


class _SaintNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pooled, weight, bias, y, w, masks, M, grad_mask, metrics, want_logp):
        lib = _lib.load()
        pooled, stride = _rows(pooled)
        weight, bias = weight.contiguous(), bias.contiguous()
        N, D = pooled.shape
        C = weight.size(0)
        dev = pooled.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        logp = torch.empty(N, C, dtype=torch.float32, device=dev) if want_logp else None
        scratch = torch.empty(METRICS_SLOTS, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ampconv_head_nll_fwd(pooled.data_ptr(), N, D, stride, weight.data_ptr(), bias.data_ptr(), C,
                                                y.data_ptr(), _ptr(w), _ptr(masks), M, grad_mask, _ptr(logp),
                                                _ptr(metrics), scratch.data_ptr(), loss.data_ptr(), _lib.DTYPES[pooled.dtype],
                                                _stream()), 'ampconv_head_nll_fwd')
        ctx.save_for_backward(pooled, weight, bias, y, w, masks)
        ctx.args = (stride, M, grad_mask)
        if logp is None:
            return loss
        ctx.mark_non_differentiable(logp)
        return loss, logp

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        lib = _lib.load()
        pooled, weight, bias, y, w, masks = ctx.saved_tensors
        stride, M, grad_mask = ctx.args
        N, D = pooled.shape
        C = weight.size(0)
        g = g.contiguous().float()                            # the upstream gradient stays on the device
        dpooled = torch.empty(N, D, dtype=pooled.dtype, device=pooled.device) if ctx.needs_input_grad[0] else None
        dW, db = torch.empty_like(weight), torch.empty(C, dtype=torch.float32, device=weight.device)
        ws = _workspace(lib, N, D, C, pooled.device)
        with torch.cuda.device(pooled.device):
            _lib.check(lib.ampconv_head_nll_bwd(pooled.data_ptr(), N, D, stride, weight.data_ptr(), bias.data_ptr(), C,
                                                y.data_ptr(), _ptr(w), _ptr(masks), M, grad_mask, g.data_ptr(),
                                                _ptr(dpooled), dW.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _lib.DTYPES[pooled.dtype], _stream()), 'ampconv_head_nll_bwd')
        return dpooled, dW, db, None, None, None, None, None, None, None


def _mask_rows(masks, N, device):
    """masks as [M, N] bytes, or None for the one all-true mask."""
    if masks is None:
        return None, 1
    if isinstance(masks, (tuple, list)):
        if not masks:
            raise ValueError('masks is empty: pass None for the one all-true mask')
        for m in masks:
            if not isinstance(m, torch.Tensor) or m.dim() != 1:
                raise ValueError('a tuple of masks holds [N] tensors')
        if len({m.dtype for m in masks}) != 1 or len({tuple(m.shape) for m in masks}) != 1:
            raise ValueError('the masks of a tuple need one dtype and one length')
        masks = torch.stack(tuple(masks))
    if not isinstance(masks, torch.Tensor) or not masks.is_cuda or masks.device != device:
        raise ValueError('masks have to be on the GPU of pooled (ampnet_amd has no CPU fallback)')
    if masks.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'masks are bool or uint8 tensors, got {masks.dtype}')
    if masks.dim() == 1:
        masks = masks.unsqueeze(0)
    if masks.dim() != 2 or masks.size(1) != N:
        raise ValueError(f'masks have to be [N] or [M, N] with N = {N}, got {tuple(masks.shape)}')
    if not 1 <= masks.size(0) <= MAX_MASKS:
        raise ValueError(f'1 to {MAX_MASKS} masks are supported, got {masks.size(0)}')
    masks = masks.contiguous()
    return (masks.view(torch.uint8) if masks.dtype == torch.bool else masks), masks.size(0)


def saint_nll_loss(pooled, weight, bias, y, node_norm=None, masks=None, grad_mask=0, metrics=None,
                   return_log_probs=False):
    """The reference's (F.nll_loss(log_softmax(pooled @ weight.T + bias), y, reduction='none') * node_norm)[mask].sum()
    for mask = masks[grad_mask], as a 0-dim float32 tensor on the device with gradients to pooled, weight and bias --
    one kernel per direction and no device synchronisation.
    y [N] int64 (-100 is ignored like torch's ignore_index; any other label outside [0, C) is skipped and counted in
    metrics' bad_labels); node_norm [N] float32 or None (1); masks: None (all nodes), a bool / uint8 tensor [N] or
    [M, N], or a tuple of [N] masks, M <= 4; metrics: a HeadMetrics that receives, for EVERY mask, loss sum, node count
    and correct count of this call on top of what it holds.  return_log_probs: also return the [N, C] log-probabilities."""
    _check_head(pooled, weight, bias, 'saint_nll_loss')
    N, dev = pooled.size(0), pooled.device
    if not isinstance(y, torch.Tensor) or y.device != dev or y.dtype != torch.int64 or y.shape != (N,):
        raise ValueError(f'saint_nll_loss: y has to be int64 [N = {N}] on the GPU of pooled')
    if node_norm is not None and (not isinstance(node_norm, torch.Tensor) or node_norm.device != dev or
                                  node_norm.dtype != torch.float32 or node_norm.shape != (N,)):
        raise ValueError(f'saint_nll_loss: node_norm has to be float32 [N = {N}] on the GPU of pooled, or None')
    masks, M = _mask_rows(masks, N, dev)
    if not 0 <= int(grad_mask) < M:
        raise ValueError(f'grad_mask {grad_mask} is outside the {M} mask(s)')
    buf = None
    if metrics is not None:
        if not isinstance(metrics, HeadMetrics) or metrics.buffer.device != dev:
            raise ValueError('metrics has to be a HeadMetrics on the GPU of pooled')
        if metrics.num_masks < M:
            raise ValueError(f'metrics holds {metrics.num_masks} mask(s), the call has {M}')
        buf = metrics.buffer
    return _SaintNLL.apply(pooled, weight, bias, y.contiguous(), None if node_norm is None else node_norm.contiguous(),
                           masks, M, int(grad_mask), buf, bool(return_log_probs))
