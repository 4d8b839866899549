"""numpy model of the dropout mask and of the four glue operations, written from the definition in include/ampconv.h
("THE MASK" and the lines below it) with np.uint64 arithmetic.  It never calls the library: the GPU tests compare the
kernels against it, the CPU test holds it to the statistical bar the kernels then inherit by exact equality."""
import numpy as np

_U = np.uint64


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = x + _U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U(27))) * _U(0x94D049BB133111EB)
    return x ^ (x >> _U(31))


def mask_params(p):
    """(threshold, scale as the float32 the host passes) for dropout probability p."""
    thr = int(round(p * 65536))
    assert 0 <= thr <= 65535
    return thr, np.float32(65536.0 / (65536 - thr))


def fields(seed, n):
    """The 16-bit field of each of the first n flat element indices."""
    i = np.arange(n, dtype=np.uint64)
    h = splitmix64(_U(seed & (2 ** 64 - 1)) ^ splitmix64(i >> _U(2)))
    return (h >> (_U(16) * (i & _U(3)))) & _U(0xFFFF)


def keep_mask(seed, thr, shape):
    """Boolean array of `shape` (row-major = flat index i): True where the element is kept (field >= threshold)."""
    n = int(np.prod(shape))
    if thr == 0:                                                 # every field is >= 0
        return np.ones(shape, dtype=bool)
    return (fields(seed, n) >= _U(thr)).reshape(shape)


def act(x, activation):
    x = np.asarray(x, dtype=np.float64)
    if activation == 'relu':
        return np.where(x > 0, x, 0.0)
    if activation == 'elu':
        return np.where(x > 0, x, np.expm1(np.minimum(x, 0.0)))
    assert activation == 'identity'
    return x


def act_slope(x, activation):
    x = np.asarray(x, dtype=np.float64)
    if activation == 'relu':
        return (x > 0).astype(np.float64)
    if activation == 'elu':
        return np.where(x > 0, 1.0, np.exp(np.minimum(x, 0.0)))
    return np.ones_like(x)


def act_dropout_fwd(x, activation, seed, p, keep=None):
    """keep: keep_mask(seed, threshold of p, x.shape) where the caller already has it (one mask serves many calls)."""
    thr, scale = mask_params(p)
    keep = keep_mask(seed, thr, x.shape) if keep is None else keep
    return np.where(keep, act(x, activation) * float(scale), 0.0)


def act_dropout_bwd(x, dy, activation, seed, p, keep=None):
    thr, scale = mask_params(p)
    keep = keep_mask(seed, thr, x.shape) if keep is None else keep
    return np.where(keep, np.asarray(dy, np.float64) * float(scale) * act_slope(x, activation), 0.0)


def pool_fwd(x, L, D, activation, pooling, seed, p):
    """x [N, L * D] -> [N, D]"""
    y = act_dropout_fwd(x, activation, seed, p).reshape(-1, L, D)
    return y.mean(axis=1) if pooling == 'mean' else y[:, 0]


def pool_bwd(x, dpooled, L, D, activation, pooling, seed, p):
    """gradient of pool_fwd w.r.t. x, shape of x"""
    g = np.zeros((x.shape[0], L, D))
    if pooling == 'mean':
        g[:] = np.asarray(dpooled, np.float64)[:, None, :] / L
    else:
        g[:, 0] = dpooled
    return act_dropout_bwd(x, g.reshape(x.shape), activation, seed, p)
