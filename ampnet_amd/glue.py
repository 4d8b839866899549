"""The glue around the AMPConv layers as fused HIP passes (csrc/glue.hip): activation + dropout between the layers,
activation + dropout + token pooling behind the last one.

The reference's model (src/ampnet/module/amp_gcn.py:239-276) is
    drop1 -> conv1 -> ReLU -> drop2 -> conv2 -> ReLU -> drop3 -> token pooling -> Linear -> log_softmax
(amp_net_classifier_Rahul.py:45-57: the same with ELU and p = 0.6).  As separate PyTorch ops every step is a full pass
over [N, L*D], every dropout saves a mask of that shape and every activation its output.  Here each site is ONE kernel
per direction, the mask is regenerated from (seed, element index) -- the contract of include/ampconv.h, "THE MASK" --
and the only tensor saved is one that is alive anyway: the output the next layer keeps as its input (act_dropout), the
layer output the model keeps as `conv2_embedding` (act_dropout_pool).

The random stream is this library's, not torch's: a model with `fused_glue=True` draws other masks than nn.Dropout does
under the same torch seed.  Under HIP-graph capture (GraphedAMPConv) the seed is a launch argument, so a replay would
repeat the captured mask; capturing these sites is out of scope.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .graph import _stream

ACTIVATIONS = {'identity': 0, 'relu': 1, 'elu': 2}          # AMPCONV_ACT_* of include/ampconv.h
POOLINGS = {'mean': 0, 'token0': 1}                         # AMPCONV_POOL_*
_MASK64 = 2 ** 64 - 1


def mask_params(p, training=True):
    """(threshold, scale) of the mask contract: threshold = round(p * 65536), scale = 65536 / (65536 - threshold), the
    inverse of the EFFECTIVE keep probability.  Not training, or p == 0: (0, 1.0) -- nothing is dropped."""
    if not 0.0 <= p < 1.0:
        raise ValueError(f'dropout probability has to be in [0, 1), got {p}')
    if not training or p == 0:
        return 0, 1.0
    thr = int(round(p * 65536))
    if thr > 65535:
        raise ValueError(f'dropout probability {p} rounds to 1: nothing would be kept')
    return thr, 65536.0 / (65536 - thr)


def _check(x, what):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f'{what} needs a tensor on the GPU (ampnet_amd has no CPU fallback)')
    if x.dtype not in _lib.DTYPES:
        raise ValueError(f'{what} takes float32 or bfloat16, got {x.dtype}')


def _code(table, key, what):
    try:
        return table[key]
    except KeyError:
        raise ValueError(f'{what} must be one of {sorted(table)}, got {key!r}') from None


def _fresh_seed():
    return int(torch.randint(0, 2 ** 62, (1,)).item())      # from torch's CPU generator: follows torch.manual_seed


class _ActDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, act, thr, scale, seed):
        lib = _lib.load()
        x = x.contiguous()
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_act_dropout_fwd(x.data_ptr(), x.numel(), act, seed, thr, scale, y.data_ptr(),
                                                   _lib.DTYPES[x.dtype], _stream()), 'ampconv_act_dropout_fwd')
        if act != ACTIVATIONS['identity']:
            ctx.save_for_backward(y)                          # the OUTPUT: what the next layer saves as its input anyway
        ctx.args = (act, thr, scale, seed)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        lib = _lib.load()
        act, thr, scale, seed = ctx.args
        y = ctx.saved_tensors[0] if ctx.saved_tensors else None
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        with torch.cuda.device(dy.device):
            _lib.check(lib.ampconv_act_dropout_bwd(dy.data_ptr(), None if y is None else y.data_ptr(), dy.numel(), act,
                                                   seed, thr, scale, dx.data_ptr(), _lib.DTYPES[dy.dtype], _stream()),
                       'ampconv_act_dropout_bwd')
        return dx, None, None, None, None


class _ActDropoutPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, L, D, act, pooling, thr, scale, seed):
        lib = _lib.load()
        x = x.contiguous()
        N = x.numel() // (L * D)
        pooled = torch.empty(N, D, dtype=x.dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_pool_fwd(x.data_ptr(), N, L, D, act, pooling, seed, thr, scale, pooled.data_ptr(),
                                            _lib.DTYPES[x.dtype], _stream()), 'ampconv_pool_fwd')
        if act != ACTIVATIONS['identity']:
            ctx.save_for_backward(x)                          # the layer output (the model's conv2_embedding)
        ctx.args = (N, L, D, act, pooling, thr, scale, seed, x.shape)
        return pooled

    @staticmethod
    @once_differentiable
    def backward(ctx, dpooled):
        lib = _lib.load()
        N, L, D, act, pooling, thr, scale, seed, shape = ctx.args
        x = ctx.saved_tensors[0] if ctx.saved_tensors else None
        dpooled = dpooled.contiguous()
        dx = torch.empty(shape, dtype=dpooled.dtype, device=dpooled.device)
        with torch.cuda.device(dpooled.device):
            _lib.check(lib.ampconv_pool_bwd(None if x is None else x.data_ptr(), dpooled.data_ptr(), N, L, D, act, pooling,
                                            seed, thr, scale, dx.data_ptr(), _lib.DTYPES[dpooled.dtype], _stream()),
                       'ampconv_pool_bwd')
        return dx, None, None, None, None, None, None, None


def act_dropout(x, p=0.0, activation='relu', training=True, seed=None):
    """dropout(act(x)) in one pass: y = keep ? act(x) / q : 0 with q the effective keep probability; same shape and dtype
    as x.  activation: 'identity', 'relu', 'elu' (alpha = 1).  Not training or p == 0: the activation alone (bit-identical
    to it); the identity then returns x itself.  seed: 64-bit mask seed (None: drawn from torch's CPU generator)."""
    _check(x, 'act_dropout')
    act = _code(ACTIVATIONS, activation, 'activation')
    thr, scale = mask_params(p, training)
    if thr == 0 and act == ACTIVATIONS['identity']:
        return x
    if seed is None:
        seed = _fresh_seed() if thr else 0
    return _ActDropout.apply(x, act, thr, scale, int(seed) & _MASK64)


def act_dropout_pool(x, embed_dim, p=0.0, activation='relu', pooling='mean', training=True, seed=None):
    """Token pooling of dropout(act(x)) in one pass: x is [N, L * embed_dim] (or [N, L, embed_dim]), the result
    [N, embed_dim] = the mean over the L tokens (pooling='mean', ascending fp32 sum: bitwise reproducible) or token 0
    (pooling='token0').  Other arguments as act_dropout."""
    _check(x, 'act_dropout_pool')
    act = _code(ACTIVATIONS, activation, 'activation')
    pool = _code(POOLINGS, pooling, 'pooling')
    D = int(embed_dim)
    if x.dim() < 2 or D <= 0 or (x.numel() // max(x.size(0), 1)) % D != 0:
        raise ValueError(f'act_dropout_pool needs [N, L * embed_dim] rows, got {tuple(x.shape)} with embed_dim {embed_dim}')
    L = x.numel() // max(x.size(0), 1) // D
    if L == 0:
        raise ValueError(f'act_dropout_pool needs at least one token per node, got {tuple(x.shape)}')
    thr, scale = mask_params(p, training)
    if seed is None:
        seed = _fresh_seed() if thr else 0
    return _ActDropoutPool.apply(x, L, D, act, pool, thr, scale, int(seed) & _MASK64)


class _SeededSite(nn.Module):
    """A dropout site with its own seed stream: the seed of a training call is a function of (seed, site, call counter),
    the way FeatureTokens.sample draws its own; `last_seed` is the one of the last training call (None before it)."""

    def __init__(self, p, activation, seed, site):
        super().__init__()
        mask_params(p)
        _code(ACTIVATIONS, activation, 'activation')
        self.p, self.activation = float(p), activation
        self._seed, self._site, self._calls = int(seed), int(site), 0
        self.last_seed = None

    def _next_seed(self):
        if not (self.training and self.p > 0):
            return 0
        self._calls += 1
        self.last_seed = ((self._seed * 1000003 + self._site) * 1000003 + self._calls) & _MASK64
        return self.last_seed


class ActDropout(_SeededSite):
    """nn.Dropout(p) behind an activation, fused (act_dropout).  No parameters."""

    def __init__(self, p=0.0, activation='relu', seed=0, site=0):
        super().__init__(p, activation, seed, site)

    def forward(self, x):
        return act_dropout(x, self.p, self.activation, self.training, self._next_seed())

    def activate(self, x):
        """The site with dropout off, whatever `training` says; advances no counter."""
        return act_dropout(x, 0.0, self.activation, False)

    def extra_repr(self):
        return f'p={self.p}, activation={self.activation!r}'


class TokenReadout(_SeededSite):
    """activation -> nn.Dropout(p) -> token pooling, fused (act_dropout_pool).  No parameters."""

    def __init__(self, embed_dim, p=0.0, activation='relu', pooling='mean', seed=0, site=0):
        super().__init__(p, activation, seed, site)
        _code(POOLINGS, pooling, 'pooling')
        self.embed_dim, self.pooling = int(embed_dim), pooling

    def forward(self, x):
        return act_dropout_pool(x, self.embed_dim, self.p, self.activation, self.pooling, self.training,
                                self._next_seed())

    def activate(self, x):
        """The site with dropout off and without the pooling: [N, L * embed_dim]; advances no counter."""
        return act_dropout(x, 0.0, self.activation, False)

    def extra_repr(self):
        return f'embed_dim={self.embed_dim}, p={self.p}, activation={self.activation!r}, pooling={self.pooling!r}'
