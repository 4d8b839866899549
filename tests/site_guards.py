"""What tests/test_gpu_glue_kernels.py, test_gpu_norm_kernels.py and test_gpu_head_kernels.py share: device buffers
inside guard bands, the header's constants, and the comparison that refuses a value nobody wrote.

A Guarded buffer is `numel` elements of a dtype that begin BAND + offset bytes into an allocation whose every byte is
FILL = 0xFF: fp32 0xFFFFFFFF and bf16 0xFFFF are NaNs, every other type sees a fixed byte.  torch's allocator returns
512-byte aligned blocks and BAND is a multiple of 16, so `offset` alone decides the alignment class of the base: 0 for the
16-byte paths, 4 (fp32) or 2 (bf16) for the element-wise ones.  After a call `intact()` says whether every byte outside
the buffer still holds FILL -- a masked lane that stores, a bound that is off by one, a zero fill that runs a row too far --
and, for an output, `written()` whether no element inside still does."""
import os
import re

import numpy as np
import torch

from conftest import ROOT, assert_close_scaled

BAND = 8192                                     # bytes on either side: two of the widest rows (1024 fp32 channels)
FILL = 0xFF
BF16_TOL = dict(atol=2e-2, rtol=2e-2)           # bf16 storage: the bar of test_gpu_glue.py, test_gpu_norm.py, test_gpu_head.py
TOL = {'f32': {}, 'bf16': BF16_TOL}
TORCH_DTYPE = {'f32': torch.float32, 'bf16': torch.bfloat16}
MISALIGN = {'f32': 4, 'bf16': 2}                # bytes: the smallest offset that keeps the element aligned and the piece not


def header_constant(name):
    """An integer #define of include/ampconv.h."""
    text = open(os.path.join(ROOT, 'include', 'ampconv.h')).read()
    return int(re.search(rf'#define\s+{name}\s+\(?(-?\d+)\)?', text).group(1))


class Guarded:
    def __init__(self, dev, dtype, numel, offset=0):
        self.nbytes = numel * torch.empty((), dtype=dtype).element_size()
        self.backing = torch.full((2 * BAND + 16 + self.nbytes,), FILL, dtype=torch.uint8, device=dev)
        assert self.backing.data_ptr() % 16 == 0 and 0 <= offset < 16
        self.lo = BAND + offset
        self.t = self.backing[self.lo:self.lo + self.nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == offset

    @classmethod
    def of(cls, dev, tensor, offset=0):
        """An input: a copy of a CPU tensor between the bands (a read past either end meets NaN)."""
        g = cls(dev, tensor.dtype, tensor.numel(), offset)
        g.t.copy_(tensor.reshape(-1))
        return g

    @property
    def ptr(self):
        return self.t.data_ptr() if self.nbytes else self.backing.data_ptr() + self.lo

    def refill(self):
        self.backing.fill_(FILL)
        return self

    def intact(self):
        return bool((self.backing[:self.lo] == FILL).all()) and bool((self.backing[self.lo + self.nbytes:] == FILL).all())

    def written(self):
        """No element still holds the fill (floats: no NaN pattern of all ones; integers: no element of all ones)."""
        size = self.t.element_size()
        raw = self.backing[self.lo:self.lo + self.nbytes].view(-1, size)
        return not bool((raw == FILL).all(dim=1).any())

    def np(self, *shape):
        a = self.t.detach().float().cpu().numpy() if self.t.is_floating_point() else self.t.cpu().numpy()
        return a.reshape(shape) if shape else a


def bits(t):
    """The bit pattern of a float tensor, for equality that tells -0 from 0 and compares NaNs."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 1: torch.uint8, 8: torch.int64}[t.element_size()])


def close(got, want, name, **tol):
    """assert_close_scaled, after making sure that every value is finite: NaN > tol is False."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f'{name}: {int((~np.isfinite(got)).sum())} values are not finite'
    assert_close_scaled(got, want, name, **tol)


def draw(gen, dtype, *size):
    """Seeded standard normal values without anything within 1e-3 of zero, rounded to the storage dtype."""
    t = torch.randn(*size, generator=gen)
    t = torch.where(t.abs() < 1e-3, torch.full_like(t, 0.5), t).to(TORCH_DTYPE[dtype])
    return t
