"""Masked feature modelling: fused token masking and the masked-value loss (csrc/mfm.hip).

The reference's predictive self-supervised script (experiments/predictive_ssl_AMPNet.py) stops at `criterion = None`.
What its authors meant is in the model classes: every one carries the masked-autoencoder parameter
`mask_token = nn.Parameter(torch.zeros(1, emb_dim))` with `nn.init.normal_(std=.02)` (gcn_one_layer.py:43-54),
gcn_classifier.py:138-151 replaces whole token vectors by it in a Python loop over nodes x features, and the duplicated-XOR
data makes a hidden value recoverable from its copies in the same node.  Here:
    build_masked_tokens   the featuriser's build with the masking fused in: tokens, the mask that was drawn (or replayed) and
                          the z-scored value of every token, one kernel; gradients to the table and the mask token
    masked_value_loss     mean((h[masked] @ weight.T + bias - target[masked]) ** 2) behind the last AMPConv layer: one
                          kernel per direction that reads the masked rows only, the upstream gradient and the count taken
                          from the device, no synchronisation; `MaskedMetrics` holds the running sums
    MaskedValueHead       nn.Linear(embed_dim, 1)'s parameters in front of that loss
As a torch composite the step is a boolean index over [N L, D] with its `nonzero`, a gathered copy of the masked rows, an
[N, L D] scatter for the gradient, a .sum() / count round trip and an index_put over the tokens on the way in.  The
contract is include/ampconv.h, "MASKED FEATURE MODELLING".  There is no eager fallback: what the kernels do not take raises.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr as _ptr
from .graph import _stream

MODES = {'token': 0, 'value': 1}                            # AMPCONV_MFM_* of include/ampconv.h
LOSS_SHIFT = 32                                             # AMPCONV_MFM_LOSS_SHIFT


def mask_threshold(rate):
    """round(rate * 65536), the threshold of THE TOKEN MASK; rate in [0, 1]."""
    rate = float(rate)
    if not 0.0 <= rate <= 1.0:
        raise ValueError(f'the mask rate has to be in [0, 1], got {rate}')
    return int(round(rate * 65536))


def _mode(mode):
    if mode not in MODES:
        raise ValueError(f'mask mode must be one of {sorted(MODES)}, got {mode!r}')
    return MODES[mode]


def _mask_bytes(masked, shape, device, what):
    """A [N, L] bool / uint8 mask on `device` as contiguous bytes."""
    if not isinstance(masked, torch.Tensor) or masked.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f'{what}: the token mask is a bool or uint8 tensor, got '
                         f'{masked.dtype if isinstance(masked, torch.Tensor) else type(masked).__name__}')
    if tuple(masked.shape) != tuple(shape):
        raise ValueError(f'{what}: the token mask has to be {tuple(shape)}, got {tuple(masked.shape)}')
    if not masked.is_cuda or masked.device != device:
        raise ValueError(f'{what}: the token mask has to be on the GPU of the tokens (ampnet_amd has no CPU fallback)')
    masked = masked.contiguous()
    return masked.view(torch.uint8) if masked.dtype == torch.bool else masked


def _workspace(lib, N, L, D, device):
    return torch.empty(max(int(lib.ampconv_mfm_workspace_bytes(N, L, D)), 16), dtype=torch.uint8, device=device)


class _BuildMaskedTokens(torch.autograd.Function):
    """(tokens [N, L, De + 1] in `dtype`, masked [N, L] uint8, target [N, L] fp32); gradients to `table` and `mask_token`
    (x is data).  Saves idx and masked only."""

    @staticmethod
    def forward(ctx, table, mask_token, x, mean, inv_std, idx, seed, threshold, mode, masked_in, dtype):
        lib = _lib.load()
        N, Fdim = x.shape
        L, De = idx.size(1), table.size(1)
        dev = x.device
        out = torch.empty(N, L, De + 1, dtype=dtype, device=dev)
        masked = torch.empty(N, L, dtype=torch.uint8, device=dev)
        target = torch.empty(N, L, dtype=torch.float32, device=dev)
        token = mask_token.detach().reshape(-1).contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.ampconv_mfm_build(x.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), idx.data_ptr(),
                                             table.data_ptr(), N, Fdim, L, De, token.data_ptr(), seed, threshold, mode,
                                             _ptr(masked_in), out.data_ptr(), masked.data_ptr(), target.data_ptr(),
                                             _lib.DTYPES[dtype], _stream()), 'ampconv_mfm_build')
        ctx.save_for_backward(idx, masked)
        ctx.dims = (N, L, De, table.size(0), mode, tuple(mask_token.shape))
        ctx.storage = dtype
        ctx.mark_non_differentiable(masked, target)
        return out, masked, target

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dmasked, _dtarget):
        lib = _lib.load()
        idx, masked = ctx.saved_tensors
        N, L, De, Fdim, mode, token_shape = ctx.dims
        dev = dout.device
        code = _lib.DTYPES[ctx.storage]
        dout = dout.to(ctx.storage).contiguous()
        dtable = dtoken = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                if De > 0 and N > 0:
                    # TOKEN: a masked token never read its table row; VALUE: it did
                    rows = idx.masked_fill(masked.view(torch.bool), -1) if mode == MODES['token'] else idx
                    dtable = torch.empty(Fdim, De, dtype=torch.float32, device=dev)
                    _lib.check(lib.ampconv_feat_table_grad_from(dout.data_ptr(), rows.data_ptr(), N, L, De, Fdim,
                                                                dtable.data_ptr(), code, _stream()),
                               'ampconv_feat_table_grad_from')
                else:
                    dtable = torch.zeros(Fdim, De, dtype=torch.float32, device=dev)
            if ctx.needs_input_grad[1]:
                dtoken = torch.empty(De + 1, dtype=torch.float32, device=dev)
                ws = _workspace(lib, N, L, De + 1, dev)
                _lib.check(lib.ampconv_mfm_token_grad(dout.data_ptr(), masked.data_ptr(), N, L, De, mode, dtoken.data_ptr(),
                                                      ws.data_ptr(), ws.numel(), code, _stream()), 'ampconv_mfm_token_grad')
                dtoken = dtoken.view(token_shape)
        return dtable, dtoken, None, None, None, None, None, None, None, None, None


def build_masked_tokens(table, mask_token, x, mean, inv_std, idx, *, seed, rate, mode='token', masked=None,
                        dtype=torch.float32):
    """tokens [N, L, De + 1] = concat(table[idx], zscore(x)[n, idx]) with the masked tokens replaced (mode 'token': by
    mask_token as a whole; 'value': their value slot by mask_token[De]), the mask [N, L] uint8 and target [N, L] fp32, the
    z-scored value of every token.  The mask is drawn from (seed, n, l) at `rate` (THE TOKEN MASK of include/ampconv.h), or
    `masked` [N, L] bool / uint8 is replayed.  table [F, De] and mask_token (De + 1 elements) float32 with gradients;
    x [N, F], mean, inv_std [F] float32; idx [N, L] int32."""
    if dtype not in _lib.DTYPES:
        raise ValueError(f'tokens are written as float32 or bfloat16, not {dtype}')
    for name, t in (('table', table), ('mask_token', mask_token), ('x', x), ('mean', mean), ('inv_std', inv_std)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f'build_masked_tokens: {name} has to be a float32 tensor on the GPU (ampnet_amd has no CPU '
                             f'fallback; the table and the mask token stay float32 under bf16 storage)')
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int32 or idx.dim() != 2 or idx.size(0) != x.size(0) or \
            idx.size(1) < 1 or idx.device != x.device:
        raise ValueError(f'build_masked_tokens: idx has to be int32 [{x.size(0)}, L >= 1] on the GPU of x')
    if table.dim() != 2 or mask_token.numel() != table.size(1) + 1:
        raise ValueError(f'build_masked_tokens: mask_token has {mask_token.numel()} elements, a token has '
                         f'{table.size(1) + 1 if table.dim() == 2 else "?"} (table {tuple(table.shape)})')
    threshold, code = mask_threshold(rate), _mode(mode)
    if masked is not None:
        masked = _mask_bytes(masked, idx.shape, x.device, 'build_masked_tokens')
    return _BuildMaskedTokens.apply(table.contiguous(), mask_token, x.contiguous(), mean, inv_std, idx.contiguous(),
                                    int(seed) & (2 ** 64 - 1), threshold, code, masked, dtype)


class MaskedMetrics:
    """The running sums of masked_value_loss on the device: the sum of the squared residuals (64-bit fixed point) and the
    number of masked tokens, accumulated in place by every call it is handed to.  `mse()` is the one read-back,
    `reset()` clears it (once per epoch, say)."""

    def __init__(self, device='cuda'):
        self.buffer = torch.zeros(2, dtype=torch.int64, device=device)
        if not self.buffer.is_cuda:
            raise ValueError('MaskedMetrics lives on the GPU (ampnet_amd has no CPU fallback)')

    def reset(self):
        self.buffer.zero_()
        return self

    def read(self):
        """{'sq_sum': sum of squared residuals, 'count': masked tokens}; synchronises."""
        sq, count = self.buffer.cpu().tolist()
        return {'sq_sum': sq / float(1 << LOSS_SHIFT), 'count': count}

    def mse(self):
        """The mean squared residual over every masked token since the last reset (0 without any); synchronises."""
        v = self.read()
        return v['sq_sum'] / max(v['count'], 1)


class _MaskedValueLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, masked, target, sums):
        lib = _lib.load()
        N, L = masked.shape
        D = weight.size(1)
        dev = h.device
        h, weight, bias = h.contiguous(), weight.contiguous(), bias.contiguous()
        resid = torch.empty(N, L, dtype=torch.float32, device=dev)
        state = torch.empty(2, dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ampconv_mfm_loss_fwd(h.data_ptr(), masked.data_ptr(), target.data_ptr(), weight.data_ptr(),
                                                bias.data_ptr(), N, L, D, resid.data_ptr(), _ptr(sums), state.data_ptr(),
                                                loss.data_ptr(), _lib.DTYPES[h.dtype], _stream()), 'ampconv_mfm_loss_fwd')
        ctx.save_for_backward(h, weight, masked, resid, state)
        ctx.h_shape = tuple(h.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        h, weight, masked, resid, state = ctx.saved_tensors
        N, L = masked.shape
        D = weight.size(1)
        dev = h.device
        g = g.contiguous().float()                            # the upstream gradient stays on the device
        dh = torch.empty(ctx.h_shape, dtype=h.dtype, device=dev) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(weight)
        db = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _workspace(lib, N, L, D, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ampconv_mfm_loss_bwd(h.data_ptr(), masked.data_ptr(), resid.data_ptr(), weight.data_ptr(),
                                                state.data_ptr(), g.data_ptr(), N, L, D, _ptr(dh), dw.data_ptr(),
                                                db.data_ptr(), ws.data_ptr(), ws.numel(), _lib.DTYPES[h.dtype], _stream()),
                       'ampconv_mfm_loss_bwd')
        return dh, dw, db, None, None, None


def masked_value_loss(h, masked, target, weight, bias, sums=None):
    """mean((h[masked] @ weight.T + bias - target[masked]) ** 2) over the masked tokens, a 0-dim float32 tensor on the
    device (0 without a masked token) with gradients to h (in its dtype), weight and bias -- one kernel per direction that
    reads the masked rows of h only, no device synchronisation; dw and db are bitwise reproducible.
    h [N, L * D] or [N, L, D] float32 or bfloat16; masked [N, L] bool / uint8; target [N, L] float32; weight [1, D] and
    bias [1] float32, the shapes of nn.Linear(D, 1); sums: a MaskedMetrics that receives this call's sums on top of what it
    holds."""
    what = 'masked_value_loss'
    for name, t in (('h', h), ('target', target), ('weight', weight), ('bias', bias)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f'{what}: {name} has to be a tensor on the GPU (ampnet_amd has no CPU fallback)')
    if h.dtype not in _lib.DTYPES:
        raise ValueError(f'{what}: h is {h.dtype}; float32 and bfloat16 are supported')
    if weight.dtype != torch.float32 or bias.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f'{what}: weight is {weight.dtype}, bias is {bias.dtype}, target is {target.dtype}: all three '
                         f'are float32 (also under bf16 storage)')
    if weight.dim() != 2 or weight.size(0) != 1 or weight.size(1) < 1 or tuple(bias.shape) != (1,):
        raise ValueError(f'{what}: weight has to be [1, D] and bias [1] (nn.Linear(D, 1)), got {tuple(weight.shape)} and '
                         f'{tuple(bias.shape)}')
    if target.dim() != 2 or target.size(1) < 1:
        raise ValueError(f'{what}: target has to be [N, L], got {tuple(target.shape)}')
    N, L = target.shape
    D = weight.size(1)
    if tuple(h.shape) not in ((N, L * D), (N, L, D)):
        raise ValueError(f'{what}: h has to be [{N}, {L * D}] or [{N}, {L}, {D}], got {tuple(h.shape)}')
    if len({h.device, target.device, weight.device, bias.device}) != 1:
        raise ValueError(f'{what}: h, target, weight and bias are on different devices')
    masked = _mask_bytes(masked, (N, L), h.device, what)
    buf = None
    if sums is not None:
        if not isinstance(sums, MaskedMetrics) or sums.buffer.device != h.device:
            raise ValueError(f'{what}: sums has to be a MaskedMetrics on the GPU of h')
        buf = sums.buffer
    return _MaskedValueLoss.apply(h, weight, bias, masked, target.contiguous(), buf)


class MaskedValueHead(nn.Linear):
    """The value decoder of masked feature modelling: the weight [1, embed_dim] and bias [1] of nn.Linear(embed_dim, 1),
    with its init.  `head(h, masked, target, sums=None)` is masked_value_loss on them."""

    def __init__(self, embed_dim):
        super().__init__(embed_dim, 1)

    def forward(self, h, masked, target, sums=None):
        return masked_value_loss(h, masked, target, self.weight, self.bias, sums)
