"""The optimizer step as fused HIP passes (csrc/optim.hip): a multi-tensor Adam / AdamW update, one launch per parameter
group, with the global gradient norm taken -- and clipped by -- on the device.

Every training script of the reference runs torch.optim.Adam with L2 weight decay, most under
CosineAnnealingWarmRestarts (experiments/cora_benchmark_graphsaint.py:84-85).  AMPGCN's 11-15 parameter tensors are a few
MB, so the step is launch-bound: FusedAdam replaces the dozen multi-tensor launches of the stock optimizer, the separate
zero_grad(), and under data parallelism the unpack and 1/world multiply of GradientAllReducer with one launch (two more
for the norm).  The tensor descriptors are rebuilt on the host every step and travel as kernel arguments: nothing is
copied to the device, nothing is read back, the step counts stay host integers.

    opt = FusedAdam(model.parameters(), lr=0.1, weight_decay=1e-4, max_grad_norm=1.0)
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=400, T_mult=2)
    loss.backward(); opt.step(set_to_none=True); sched.step()
    # data parallel: reducer.allreduce(unpack=False); opt.step(grads=reducer.views, grad_scale=1 / world, set_to_none=True)

Contiguous float32 or bfloat16 parameters on the GPU only; no amsgrad, maximize or capturable; no CPU or eager fallback.

bf16 STORAGE.  A bfloat16 parameter (AMPGCN(storage_dtype=torch.bfloat16)) is stepped on an fp32 master copy,
state[p]['master']: an update of lr = 1e-3 on a bf16 weight near 1 is below half a bf16 ulp and torch.optim.Adam on the
bf16 tensor loses every one of them.  The moments are fp32, gradients may be fp32 or bf16, the arithmetic is the fp32
step's on the master, and the parameter is rewritten as the rounded master in the same launch.  An all-fp32 set runs the
fp32 entry points exactly as before.
"""
import ctypes
import math

import torch

from . import _lib
from .graph import _stream

CHUNK = _lib.ADAM_CHUNK                  # elements per workgroup (AMPCONV_ADAM_CHUNK)
MAX_TENSORS = _lib.ADAM_MAX_TENSORS      # descriptors per launch (AMPCONV_ADAM_MAX_TENSORS)

_SUPPORTED = ('FusedAdam supports contiguous float32 or bfloat16 parameters on the GPU with dense float32 or bfloat16 gradients '
              'of the same shape and device, without amsgrad, maximize or capturable (ampnet_amd has no CPU or eager fallback)')
_FP32_STATE = ('exp_avg', 'exp_avg_sq', 'master')
_REFUSED = ('amsgrad', 'maximize', 'capturable')
_ENTRY = ctypes.sizeof(_lib.AdamTensor)
_MIXED_ENTRY = ctypes.sizeof(_lib.AdamMixedTensor)


class FusedAdam(torch.optim.Optimizer):
    """Drop-in for torch.optim.Adam (decoupled=False: L2 weight decay) and torch.optim.AdamW (decoupled=True) on the
    formulas of include/ampconv.h, "optimizer step".  A real Optimizer: param_groups with a python-float lr (torch's LR
    schedulers drive it unchanged), per-parameter state `step` (a host integer), `exp_avg`, `exp_avg_sq` created at the
    first step in which the parameter has a gradient; state dicts go to and come from torch.optim.Adam / AdamW.  A bfloat16
    parameter also has `master`, its fp32 value (from p.float() at that first step, or when a loaded state lacks it); the
    moments and the master stay fp32 through state_dict() / load_state_dict().

    max_grad_norm: clip the global gradient norm over ALL groups to it, as torch.nn.utils.clip_grad_norm_ before the step;
    the norm and the coefficient never leave the device.  track_grad_norm: take the norm without clipping.  With either,
    `grad_norm` is a 0-dim float32 device tensor after each step: the norm of that step's gradients after grad_scale,
    before clipping (a fresh tensor per step); None otherwise."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                 max_grad_norm=None, track_grad_norm=False, **refused):
        for k, v in refused.items():
            if k not in _REFUSED:
                raise TypeError(f'FusedAdam got an unexpected keyword argument {k!r}')
            if v:
                raise ValueError(f'{k}={v!r} was requested; {_SUPPORTED}')
        if isinstance(lr, torch.Tensor):
            raise ValueError(f'lr has to be a python float, not a tensor; {_SUPPORTED}')
        if not lr >= 0.0:
            raise ValueError(f'lr has to be >= 0, got {lr}')
        if not eps > 0.0:
            raise ValueError(f'eps has to be positive, got {eps}')
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f'betas have to lie in [0, 1), got {betas}')
        if not weight_decay >= 0.0:
            raise ValueError(f'weight_decay has to be >= 0, got {weight_decay}')
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f'max_grad_norm has to be positive or None, got {max_grad_norm}')
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.track_grad_norm = bool(track_grad_norm)
        self.grad_norm = None
        # the group key of the decoupled decay is torch.optim.Adam's own, so that it survives a state dict either way
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled), amsgrad=False, maximize=False,
                                      capturable=False))

    def __setstate__(self, state):
        """Also the tail of load_state_dict, whose groups are the SAVED ones: a torch.optim.Adam checkpoint brings 0-dim
        `step` tensors (read back here, once) and possibly float64 or strided moments."""
        super().__setstate__(state)
        self.__dict__.setdefault('max_grad_norm', None)
        self.__dict__.setdefault('track_grad_norm', False)
        self.__dict__.setdefault('grad_norm', None)
        for group in self.param_groups:
            group.setdefault('decoupled_weight_decay', False)
            for k in _REFUSED:
                group.setdefault(k, False)
        for st in self.state.values():
            if 'step' in st:
                st['step'] = int(st['step'].item()) if isinstance(st['step'], torch.Tensor) else int(st['step'])
            for k in _FP32_STATE:
                if k in st:
                    st[k] = st[k].to(torch.float32).contiguous()

    def load_state_dict(self, state_dict):
        """torch casts loaded state to the parameter's dtype, which would round the moments and the master of a bfloat16
        parameter to bf16: they are taken from `state_dict` again, in fp32."""
        super().load_state_dict(state_dict)
        ids = [i for group in state_dict['param_groups'] for i in group['params']]
        params = [p for group in self.param_groups for p in group['params']]
        for i, p in zip(ids, params):
            saved = state_dict['state'].get(i)
            if saved is None or p.dtype == torch.float32:
                continue
            for k in _FP32_STATE:
                if k in saved:
                    self.state[p][k] = saved[k].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()

    def full_precision_state_dict(self, model):
        """model.state_dict() with every bfloat16 parameter of this optimizer replaced by its fp32 master (p.float() where it
        has none yet): the keys are the model's own -- for AMPGCN the reference's --, so the checkpoint loads into an fp32
        model.  Copies; nothing is shared with the model or the state."""
        named = dict(model.named_parameters())
        out = {}
        for k, t in model.state_dict().items():
            p = named.get(k)
            if p is not None and p.dtype == torch.bfloat16:
                master = self.state.get(p, {}).get('master')
                out[k] = (master if master is not None else p.detach().float()).clone()
            else:
                out[k] = t.detach().clone()
        return out

    @torch.no_grad()
    def load_full_precision_state_dict(self, model, state_dict):
        """The way back: every entry is copied into the model (a bfloat16 parameter receives the rounded value) and the
        exact fp32 value becomes the master of a bfloat16 parameter.  The keys have to be the model's."""
        own = model.state_dict()
        if set(own) != set(state_dict):
            raise KeyError(f'state dict keys differ from the model\'s: missing {sorted(set(own) - set(state_dict))}, '
                           f'unexpected {sorted(set(state_dict) - set(own))}')
        named = dict(model.named_parameters())
        for k, t in own.items():
            src = state_dict[k].detach().to(t.device)
            if src.shape != t.shape:
                raise ValueError(f'{k}: shape {tuple(src.shape)} for a {tuple(t.shape)} tensor')
            t.copy_(src)
            p = named.get(k)
            if p is not None and p.dtype == torch.bfloat16:
                self.state[p]['master'] = src.to(torch.float32, copy=True).contiguous()

    @staticmethod
    def _check_group(group):
        for k in _REFUSED:
            if group.get(k):
                raise ValueError(f'a parameter group asks for {k}; {_SUPPORTED}')
        if isinstance(group['lr'], torch.Tensor):
            raise ValueError(f'lr has to be a python float, not a tensor; {_SUPPORTED}')

    @staticmethod
    def _check_pair(p, g):
        if p.dtype not in _lib.DTYPES:
            raise ValueError(f'a parameter is {p.dtype}; {_SUPPORTED}')
        if not p.is_cuda:
            raise ValueError(f'a parameter is on {p.device}, not on the GPU; {_SUPPORTED}')
        if not p.is_contiguous():
            raise ValueError(f'a parameter of shape {tuple(p.shape)} is not contiguous; {_SUPPORTED}')
        if not isinstance(g, torch.Tensor) or g.is_sparse or g.layout != torch.strided:
            raise ValueError(f'a gradient is {"sparse" if isinstance(g, torch.Tensor) else type(g).__name__}; {_SUPPORTED}')
        if g.dtype not in _lib.DTYPES or g.device != p.device or g.shape != p.shape:
            raise ValueError(f'a gradient is {g.dtype} {tuple(g.shape)} on {g.device} for a {tuple(p.shape)} parameter on '
                             f'{p.device}; {_SUPPORTED}')

    @torch.no_grad()
    def step(self, closure=None, *, grads=None, grad_scale=1.0, set_to_none=False):
        """One update of every parameter that has a gradient; a parameter without one is skipped entirely (its state and
        step count do not advance).  grads: a list parallel to the flattened parameter list (None entries allowed), read
        INSTEAD of p.grad -- e.g. GradientAllReducer.views.  grad_scale multiplies every gradient in the pass (the 1/world
        of data parallelism).  set_to_none: every p.grad is set to None once the launches are enqueued -- the allocator is
        stream-ordered, so the kernels still read valid memory --, which folds zero_grad() into the step.  Nothing
        synchronises."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        params = [p for group in self.param_groups for p in group['params']]
        if grads is not None:
            grads = list(grads)
            if len(grads) != len(params):
                raise ValueError(f'grads has {len(grads)} entries for {len(params)} parameters')
        work, keep, device, at = [], [], None, 0                 # checked first: a refused call changes no state
        for group in self.param_groups:
            self._check_group(group)
            pairs = []
            for p in group['params']:
                g = p.grad if grads is None else grads[at]
                at += 1
                if g is None:
                    continue
                self._check_pair(p, g)
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise ValueError(f'parameters on {device} and {p.device}: one FusedAdam steps one device')
                if not g.is_contiguous():
                    g = g.contiguous()
                    keep.append(g)
                pairs.append((p, g))
            work.append(pairs)
        # an all-fp32 step runs the fp32 entry points, as it always has; a bfloat16 parameter or gradient the mixed ones
        mixed = any(p.dtype != torch.float32 or g.dtype != torch.float32 for pairs in work for p, g in pairs)
        entries, spans = [], []
        for group, pairs in zip(self.param_groups, work):
            lr, (beta1, beta2) = float(group['lr']), group['betas']
            spans.append((len(entries), len(pairs)))
            for p, g in pairs:
                st = self.state[p]
                if 'step' not in st:
                    st['step'] = 0
                    st['exp_avg'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
                if p.dtype == torch.bfloat16 and 'master' not in st:
                    st['master'] = p.detach().to(torch.float32, memory_format=torch.contiguous_format)
                st['step'] += 1
                t = st['step']
                row = (p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr())
                tail = (p.numel(), lr / (1.0 - beta1 ** t), 1.0 / math.sqrt(1.0 - beta2 ** t))
                if mixed:
                    master = st['master'].data_ptr() if p.dtype == torch.bfloat16 and p.numel() else None
                    entries.append(row + (master,) + tail + (_lib.DTYPES[p.dtype], _lib.DTYPES[g.dtype]))
                else:
                    entries.append(row + tail)
        want_norm = self.max_grad_norm is not None or self.track_grad_norm
        if entries or (want_norm and params and params[0].is_cuda):
            device = device if device is not None else params[0].device
            lib = _lib.load()
            kind, size = (_lib.AdamMixedTensor, _MIXED_ENTRY) if mixed else (_lib.AdamTensor, _ENTRY)
            prefix = 'ampconv_adam_mixed_' if mixed else 'ampconv_adam_'
            table = (kind * len(entries))(*entries)
            norm = None
            with torch.cuda.device(device):
                stream = _stream()
                if want_norm:
                    norm = torch.empty((), dtype=torch.float32, device=device)
                    ws = torch.empty(getattr(lib, prefix + 'workspace_bytes')(table, len(entries)), dtype=torch.uint8,
                                     device=device)
                    _lib.check(getattr(lib, prefix + 'grad_norm')(table, len(entries), grad_scale, norm.data_ptr(),
                                                                  ws.data_ptr(), ws.numel(), stream), prefix + 'grad_norm')
                    self.grad_norm = norm
                clip = norm.data_ptr() if self.max_grad_norm is not None else None
                for group, (first, count) in zip(self.param_groups, spans):
                    if count == 0:
                        continue
                    rows = ctypes.cast(ctypes.byref(table, first * size), ctypes.POINTER(kind))
                    _lib.check(getattr(lib, prefix + 'step')(rows, count, float(group['lr']), group['betas'][0],
                                                             group['betas'][1], group['eps'], group['weight_decay'],
                                                             int(bool(group['decoupled_weight_decay'])), grad_scale, clip,
                                                             self.max_grad_norm or 0.0, stream), prefix + 'step')
        if set_to_none:
            for p in params:
                p.grad = None
        return loss
