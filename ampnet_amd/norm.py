"""Per-token LayerNorm sites around the AMPConv layers as fused HIP passes (csrc/norm.hip): LayerNorm over the
embed_dim channels of every token -> activation -> dropout, and the same followed by the token pooling.

The reference's deeper model (experiments/cora_overfit_one_subgraph.py:46-107) puts
    reshape [N, L, D] -> nn.LayerNorm(D) -> ReLU -> reshape back
behind each of its AMPConv layers and the token pooling behind the last.  As separate ops every one of these is a pass
over [N, L*D] per direction and the normalisation saves a tensor of that shape.  Here a site is ONE kernel per direction:
the mask is regenerated from (seed, element index) -- include/ampconv.h, "THE MASK": the same elements an act_dropout
site with that seed drops --, the activation derivative is recomputed from x, the row statistics, weight and bias, and
what is saved is x (the layer output the model keeps anyway) and 8 bytes of statistics per token.  weight and bias
gradients are fixed-order sums: bitwise reproducible.

Rows of up to MAX_EMBED_DIM channels.  The seed is a launch argument: capturing these sites in a HIP graph is out of
scope, as for the glue.
"""
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr as _ptr
from .glue import ACTIVATIONS, POOLINGS, _MASK64, _SeededSite, _check, _code, _fresh_seed, mask_params
from .graph import _stream

MAX_EMBED_DIM = 1024                                        # AMPCONV_NORM_MAX_D of include/ampconv.h


def _workspace(lib, tokens, D, device):
    return torch.empty(lib.ampconv_norm_workspace_bytes(tokens, D), dtype=torch.uint8, device=device)


def _param_grads(weight, D, device):
    if weight is None:
        return None, None
    return torch.empty(D, dtype=torch.float32, device=device), torch.empty(D, dtype=torch.float32, device=device)


class _NormActDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, D, eps, act, thr, scale, seed):
        lib = _lib.load()
        x = x.contiguous()
        T = x.numel() // D
        y = torch.empty_like(x)
        stats = torch.empty(T, 2, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_norm_fwd(x.data_ptr(), T, D, _ptr(weight), _ptr(bias), eps, act, seed, thr, scale,
                                            y.data_ptr(), stats.data_ptr(), _lib.DTYPES[x.dtype], _stream()),
                       'ampconv_norm_fwd')
        ctx.save_for_backward(x, stats, weight, bias)         # x: the layer output (the model's convN_embedding)
        ctx.args = (T, D, act, thr, scale, seed)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        x, stats, weight, bias = ctx.saved_tensors
        T, D, act, thr, scale, seed = ctx.args
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dw, db = _param_grads(weight, D, x.device)
        ws = None if dw is None else _workspace(lib, T, D, x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_norm_bwd(x.data_ptr(), dy.data_ptr(), stats.data_ptr(), T, D, _ptr(weight), _ptr(bias),
                                            act, seed, thr, scale, dx.data_ptr(), _ptr(dw), _ptr(db), _ptr(ws),
                                            0 if ws is None else ws.numel(), _lib.DTYPES[x.dtype], _stream()),
                       'ampconv_norm_bwd')
        return dx, dw, db, None, None, None, None, None, None


class _NormActDropoutPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, L, D, eps, act, pooling, thr, scale, seed):
        lib = _lib.load()
        x = x.contiguous()
        N = x.numel() // (L * D)
        pooled = torch.empty(N, D, dtype=x.dtype, device=x.device)
        stats = torch.empty(N * (1 if pooling == POOLINGS['token0'] else L), 2, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_norm_pool_fwd(x.data_ptr(), N, L, D, _ptr(weight), _ptr(bias), eps, act, pooling, seed,
                                                 thr, scale, pooled.data_ptr(), stats.data_ptr(), _lib.DTYPES[x.dtype],
                                                 _stream()), 'ampconv_norm_pool_fwd')
        ctx.save_for_backward(x, stats, weight, bias)
        ctx.args = (N, L, D, act, pooling, thr, scale, seed)
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, dpooled):
        lib = _lib.load()
        x, stats, weight, bias = ctx.saved_tensors
        N, L, D, act, pooling, thr, scale, seed = ctx.args
        dpooled = dpooled.contiguous()
        dx = torch.empty_like(x)
        dw, db = _param_grads(weight, D, x.device)
        ws = None if dw is None else _workspace(lib, N * L, D, x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_norm_pool_bwd(x.data_ptr(), dpooled.data_ptr(), stats.data_ptr(), N, L, D, _ptr(weight),
                                                 _ptr(bias), act, pooling, seed, thr, scale, dx.data_ptr(), _ptr(dw),
                                                 _ptr(db), _ptr(ws), 0 if ws is None else ws.numel(), _lib.DTYPES[x.dtype],
                                                 _stream()), 'ampconv_norm_pool_bwd')
        return dx, dw, db, None, None, None, None, None, None, None, None


def _site_args(x, embed_dim, weight, bias, eps, p, activation, training, seed, what):
    """Validated (D, weight, bias, eps, act, thr, scale, seed) of a call.  What can be said without a device is checked
    first, the device last."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f'{what} needs a tensor, got {type(x).__name__}')
    if x.dtype not in _lib.DTYPES:
        raise ValueError(f'{what} takes float32 or bfloat16, got {x.dtype}')
    act = _code(ACTIVATIONS, activation, 'activation')
    D = int(embed_dim)
    if D > MAX_EMBED_DIM:
        raise ValueError(f'{what} supports embed_dim <= {MAX_EMBED_DIM}, got {embed_dim}')
    row = math.prod(x.shape[1:]) if x.dim() >= 2 else 0
    if D <= 0 or row == 0 or row % D != 0:
        raise ValueError(f'{what} needs [N, L * embed_dim] rows with L >= 1, got {tuple(x.shape)} with embed_dim {embed_dim}')
    if not eps > 0:
        raise ValueError(f'eps has to be positive, got {eps}')
    thr, scale = mask_params(p, training)
    _check(x, what)
    if (weight is None) != (bias is None):
        raise ValueError(f'{what} takes weight and bias together or neither')
    for name, t in (('weight', weight), ('bias', bias)):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.device != x.device or t.dtype != torch.float32 or t.shape != (D,):
            raise ValueError(f'{name} has to be a float32 tensor of shape ({D},) on the device of x, got '
                             f'{getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))}')
    if seed is None:
        seed = _fresh_seed() if thr else 0
    if weight is not None:
        weight, bias = weight.contiguous(), bias.contiguous()
    return D, weight, bias, float(eps), act, thr, scale, int(seed) & _MASK64


def norm_act_dropout(x, embed_dim, weight=None, bias=None, eps=1e-5, p=0.0, activation='identity', training=True,
                     seed=None):
    """dropout(act(layer_norm(x))) in one pass, the normalisation over the embed_dim channels of every token (biased
    variance, nn.LayerNorm's): x is [N, L * embed_dim] or [N, L, embed_dim], the result has its shape and dtype.  weight and
    bias: float32 [embed_dim] (None: 1 and 0).  p, activation, training, seed as act_dropout: a site with the same seed
    drops the same elements.  Gradients flow to x, weight and bias."""
    D, weight, bias, eps, act, thr, scale, seed = _site_args(x, embed_dim, weight, bias, eps, p, activation, training, seed,
                                                             'norm_act_dropout')
    return _NormActDropout.apply(x, weight, bias, D, eps, act, thr, scale, seed)


def norm_act_dropout_pool(x, embed_dim, weight=None, bias=None, eps=1e-5, p=0.0, activation='identity', pooling='mean',
                          training=True, seed=None):
    """Token pooling of norm_act_dropout(x) in one pass: [N, embed_dim] = the mean over the L tokens (pooling='mean',
    ascending fp32 sum) or token 0 (pooling='token0': only that token is normalised)."""
    pool = _code(POOLINGS, pooling, 'pooling')
    D, weight, bias, eps, act, thr, scale, seed = _site_args(x, embed_dim, weight, bias, eps, p, activation, training, seed,
                                                             'norm_act_dropout_pool')
    L = math.prod(x.shape[1:]) // D
    return _NormActDropoutPool.apply(x, weight, bias, L, D, eps, act, pool, thr, scale, seed)


class TokenLayerNorm(_SeededSite):
    """nn.LayerNorm(embed_dim) on every token -> activation -> nn.Dropout(p), fused (norm_act_dropout).  `weight` (ones)
    and `bias` (zeros) are nn.LayerNorm's parameters: same state-dict keys, shapes and initialisation."""

    def __init__(self, embed_dim, eps=1e-5, elementwise_affine=True, p=0.0, activation='identity', seed=0, site=0):
        super().__init__(p, activation, seed, site)
        if not 1 <= int(embed_dim) <= MAX_EMBED_DIM:
            raise ValueError(f'{type(self).__name__} supports 1 <= embed_dim <= {MAX_EMBED_DIM}, got {embed_dim}')
        if not eps > 0:
            raise ValueError(f'eps has to be positive, got {eps}')
        self.embed_dim, self.eps, self.elementwise_affine = int(embed_dim), float(eps), bool(elementwise_affine)
        if self.elementwise_affine:
            self.weight = nn.Parameter(torch.ones(self.embed_dim))
            self.bias = nn.Parameter(torch.zeros(self.embed_dim))
        else:
            self.register_parameter('weight', None)
            self.register_parameter('bias', None)

    def forward(self, x):
        return norm_act_dropout(x, self.embed_dim, self.weight, self.bias, self.eps, self.p, self.activation, self.training,
                                self._next_seed())

    def activate(self, x):
        """The site with dropout off (and, in NormTokenReadout, without the pooling); advances no counter."""
        return norm_act_dropout(x, self.embed_dim, self.weight, self.bias, self.eps, 0.0, self.activation, False)

    def extra_repr(self):
        return (f'embed_dim={self.embed_dim}, eps={self.eps}, elementwise_affine={self.elementwise_affine}, p={self.p}, '
                f'activation={self.activation!r}')


class NormTokenReadout(TokenLayerNorm):
    """TokenLayerNorm followed by the token pooling, fused (norm_act_dropout_pool): [N, L * embed_dim] -> [N, embed_dim]."""

    def __init__(self, embed_dim, eps=1e-5, elementwise_affine=True, p=0.0, activation='identity', pooling='mean', seed=0,
                 site=0):
        super().__init__(embed_dim, eps, elementwise_affine, p, activation, seed, site)
        _code(POOLINGS, pooling, 'pooling')
        self.pooling = pooling

    def forward(self, x):
        return norm_act_dropout_pool(x, self.embed_dim, self.weight, self.bias, self.eps, self.p, self.activation,
                                     self.pooling, self.training, self._next_seed())

    def extra_repr(self):
        return super().extra_repr() + f', pooling={self.pooling!r}'
