"""numpy float64 model of include/ampconv.h, "optimizer step": the Adam / AdamW update, the clipping coefficient and the
global gradient norm, written from the header's formulas.  Shared by tests/test_optim_cpu.py (held against
torch.optim.Adam / AdamW and clip_grad_norm_ in float64) and tests/test_gpu_optim.py (the bar for the fp32 kernels)."""
import numpy as np


def grad_norm(grads, grad_scale=1.0):
    """sqrt(sum over all tensors of (g * grad_scale)^2); None entries have no gradient."""
    return float(np.sqrt(sum(float(np.sum((np.asarray(g, np.float64) * grad_scale) ** 2)) for g in grads if g is not None)))


def clip_coefficient(norm, max_grad_norm):
    """c = norm given ? min(1, max_grad_norm / (norm + 1e-6)) : 1"""
    return 1.0 if max_grad_norm is None else min(1.0, max_grad_norm / (norm + 1e-6))


def adam_tensor(p, g, m, v, t, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False, grad_scale=1.0,
                c=1.0):
    """One update of one tensor at step count t (1 for its first update): returns the new (p, m, v)."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    step_size = lr / (1.0 - beta1 ** t)
    inv_bc2_sqrt = 1.0 / np.sqrt(1.0 - beta2 ** t)
    g = g * grad_scale * c
    if decoupled:
        p = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
    m = m + (1.0 - beta1) * (g - m)
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - step_size * m / (np.sqrt(v) * inv_bc2_sqrt + eps)
    return p, m, v


class Adam:
    """The optimizer over a list of float64 arrays: per-tensor step counts, state created at a tensor's first gradient,
    a tensor whose gradient is None skipped entirely.  `norm` is the last step's global gradient norm (after grad_scale,
    before clipping)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, max_grad_norm=None):
        self.p = [np.array(a, np.float64) for a in params]
        self.m = [None] * len(self.p)
        self.v = [None] * len(self.p)
        self.t = [0] * len(self.p)
        self.lr, self.betas, self.eps, self.weight_decay, self.decoupled = lr, betas, eps, weight_decay, decoupled
        self.max_grad_norm, self.norm = max_grad_norm, None

    def step(self, grads, grad_scale=1.0):
        self.norm = grad_norm(grads, grad_scale)
        c = clip_coefficient(self.norm, self.max_grad_norm)
        for i, g in enumerate(grads):
            if g is None:
                continue
            if self.m[i] is None:
                self.m[i], self.v[i] = np.zeros_like(self.p[i]), np.zeros_like(self.p[i])
            self.t[i] += 1
            self.p[i], self.m[i], self.v[i] = adam_tensor(self.p[i], g, self.m[i], self.v[i], self.t[i], self.lr, *self.betas,
                                                          self.eps, self.weight_decay, self.decoupled, grad_scale, c)
        return self


SIZES = [(1,), (3,), (7,), (1024,), (1025,), (4100,), (7, 100)]      # the tensor set of the tests (the GPU file adds a slice)


def make_grads(shapes, seed):
    """One gradient per shape: magnitudes log-uniform in [1e-6, 1e2], random sign, about 10 % exact zeros (float32
    values, so that g * g * (1 - beta2) stays in fp32's normal range)."""
    rng = np.random.default_rng(seed)
    out = []
    for s in shapes:
        g = 10.0 ** rng.uniform(-6.0, 2.0, s) * rng.choice([-1.0, 1.0], s)
        g[rng.random(s) < 0.1] = 0.0
        out.append(g.astype(np.float32))
    return out


def make_params(shapes, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]
