"""numpy fp64 model of the classifier head and of the GraphSAINT-weighted NLL loss with its metrics, written from the
contract in include/ampconv.h ("classifier head").  It never calls the library: tests/test_head_cpu.py holds it to torch's
CPU composite and autograd, tests/test_gpu_head.py holds the kernels to it.  make_inputs: the seeded test inputs of both."""
import numpy as np

IGNORE_INDEX = -100


def _f64(*arrays):
    return [np.asarray(a, dtype=np.float64) for a in arrays]


def logits(pooled, W, b):
    pooled, W, b = _f64(pooled, W, b)
    return pooled @ W.T + b


def log_softmax(z):
    z = z - z.max(axis=1, keepdims=True) if z.shape[0] else z
    return z - np.log(np.exp(z).sum(axis=1, keepdims=True))


def head_fwd(pooled, W, b, kind='log_softmax'):
    z = logits(pooled, W, b)
    return log_softmax(z) if kind == 'log_softmax' else 1.0 / (1.0 + np.exp(-z))


def _param_grads(pooled, W, dz):
    pooled, W = _f64(pooled, W)
    return dz @ W, dz.T @ pooled, dz.sum(axis=0)


def head_bwd(pooled, W, dout, out, kind='log_softmax'):
    """(dpooled, dW, db) from the saved output."""
    dout, out = _f64(dout, out)
    if kind == 'log_softmax':
        dz = dout - np.exp(out) * dout.sum(axis=1, keepdims=True)
    else:
        dz = dout * out * (1.0 - out)
    return _param_grads(pooled, W, dz)


def _masks(masks, N):
    if masks is None:
        return np.ones((1, N), dtype=bool)
    masks = np.asarray(masks)
    return (masks[None, :] if masks.ndim == 1 else masks) != 0


def selection(y, masks, C):
    """(used [M, N]: selected by the mask with a label in [0, C); bad: nodes some mask selects whose label is neither
    ignore_index nor in range)."""
    y = np.asarray(y, dtype=np.int64)
    masks = _masks(masks, y.shape[0])
    sel = masks & (y != IGNORE_INDEX)[None, :]
    in_range = (y >= 0) & (y < C)
    return sel & in_range[None, :], int((sel.any(axis=0) & ~in_range).sum())


def nll_fwd(pooled, W, b, y, w=None, masks=None):
    """{'logp' [N, C], 'loss_sum' [M], 'count' [M], 'correct' [M], 'bad_labels'}."""
    y = np.asarray(y, dtype=np.int64)
    N, C = y.shape[0], np.asarray(W).shape[0]
    logp = head_fwd(pooled, W, b)
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    used, bad = selection(y, masks, C)
    safe = np.where((y >= 0) & (y < C), y, 0)
    nll = -logp[np.arange(N), safe] * w
    hit = logp.argmax(axis=1) == y if N else np.zeros(0, dtype=bool)       # numpy's argmax: the first maximum
    return {'logp': logp, 'loss_sum': [float(nll[u].sum()) for u in used], 'count': [int(u.sum()) for u in used],
            'correct': [int((hit & u).sum()) for u in used], 'bad_labels': bad}


def nll_bwd(pooled, W, b, y, w=None, masks=None, grad_mask=0, g=1.0):
    """(dpooled, dW, db) of g * loss_sum[grad_mask]."""
    y = np.asarray(y, dtype=np.int64)
    N, C = y.shape[0], np.asarray(W).shape[0]
    soft = np.exp(head_fwd(pooled, W, b))
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64)
    used, _ = selection(y, masks, C)
    onehot = np.zeros((N, C))
    rows = np.nonzero(used[grad_mask])[0]
    onehot[rows, y[rows]] = 1.0
    dz = float(g) * (w * used[grad_mask])[:, None] * (soft - onehot)
    return _param_grads(pooled, W, dz)


def make_inputs(N, D, C, seed=0):
    """Seeded randn pooled, W and b uniform in +-1/sqrt(D) (logits O(1)), labels, weights and two overlapping masks."""
    import torch
    g = torch.Generator().manual_seed(seed + 1000 * N + 10 * D + C)
    pooled = torch.randn(N, D, generator=g)
    W = (torch.rand(C, D, generator=g) * 2 - 1) / D ** 0.5
    b = (torch.rand(C, generator=g) * 2 - 1) / D ** 0.5
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(N, generator=g) * 3 + 0.1
    masks = torch.stack([torch.rand(N, generator=g) < 0.6, torch.rand(N, generator=g) < 0.5])
    return pooled, W, b, y, w, masks
