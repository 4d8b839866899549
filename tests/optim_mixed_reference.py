"""numpy model of include/ampconv.h, "mixed-precision optimizer step", on top of tests/optim_reference.py (imported
unchanged): the float64 Adam of that file runs on the MASTER values, a bf16 parameter is the round-to-nearest-even bf16 of
its master, a bf16 gradient is widened (exactly) before anything else.  Shared by tests/test_bf16_model_cpu.py (the rounding
helper held against torch, the stall that motivates the master) and tests/test_gpu_optim_mixed.py (the bar for launches
of more than one batch of descriptors)."""
import numpy as np

import optim_reference as ref

F32, BF16 = 'f32', 'bf16'


def bf16_round(a):
    """float32 values -> the float32 values of their round-to-nearest-even bfloat16 (what torch's .to(torch.bfloat16)
    stores): add 0x7FFF plus the lowest kept bit to the bit pattern and drop the low half.  +-inf stay, the largest
    finite floats round to inf, a NaN stays a (quiet) NaN."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    r = np.where(np.isnan(a), np.uint32(0x7FC00000), r).astype(np.uint32)
    return r.view(np.float32).reshape(a.shape)


class MixedAdam:
    """ref.Adam over the masters.  params: float32 arrays; dtypes: F32 / BF16 per tensor -- a BF16 tensor starts from the
    rounded parameter, as FusedAdam creates the master from p.float().  `master`: float64 arrays; `p`: what the
    parameter tensors hold (float32 arrays, bf16-valued where the storage is bf16)."""

    def __init__(self, params, dtypes, **kw):
        self.dtypes = list(dtypes)
        self.adam = ref.Adam([bf16_round(a) if d == BF16 else a for a, d in zip(params, self.dtypes)], **kw)

    def step(self, grads, grad_scale=1.0):
        self.adam.step(grads, grad_scale)
        return self

    @property
    def master(self):
        return self.adam.p

    @property
    def p(self):
        return [bf16_round(a.astype(np.float32)) if d == BF16 else a.astype(np.float32)
                for a, d in zip(self.adam.p, self.dtypes)]

    m = property(lambda self: self.adam.m)
    v = property(lambda self: self.adam.v)
    norm = property(lambda self: self.adam.norm)
