"""numpy model of include/ampconv.h, "tensor statistics", written from the header: elements classified from their BITS,
fp64 moments over the finite ones, THE BIN RULE in np.float32 arithmetic with the header's roundings, and selection by the
order-preserving key of the bits.  Shared by tests/test_stats_cpu.py (held against numpy / torch implementations that know
nothing of it) and tests/test_gpu_stats.py, tests/test_gpu_diagnostics.py (where it is the bar for the kernels: counts,
extrema, bins and order statistics are exact, the moments fp64).

A tensor comes in as a float32 array, or as a uint16 array of bfloat16 bit patterns (numpy has no bfloat16)."""
import numpy as np


def bits32(x):
    """The fp32 bit patterns of a tensor: float32 as it is, uint16 (bfloat16 patterns) shifted into the upper half; -0
    rewritten to +0."""
    x = np.ascontiguousarray(x).reshape(-1)
    if x.dtype == np.uint16:
        u = x.astype(np.uint32) << np.uint32(16)
    else:
        assert x.dtype == np.float32, x.dtype
        u = x.view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0
    return u


def bf16_bits(x):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even; NaN stays NaN, infinities stay."""
    u = np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint32)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r[nan] = 0x7FC0
    return r.astype(np.uint16)


def key_of(u):
    """The unsigned key whose order is the values' order: sign bit set -> ~bits, else bits | 0x80000000."""
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def finite_values(x):
    """(float32 values of the finite elements in their order, nan count, inf count)."""
    u = bits32(x)
    special = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    frac = (u & np.uint32(0x007FFFFF)) != 0
    return u[~special].view(np.float32), int((special & frac).sum()), int((special & ~frac).sum())


def rank_of(q, finite):
    """floor(q * (finite - 1)) in float64: numpy's method 'lower'; q = 0.5 is (finite - 1) // 2."""
    return int(np.floor(np.float64(q) * np.float64(finite - 1)))


def select(v, ranks):
    """The elements of the given ranks of the finite float32 values v in ascending KEY order."""
    if v.size == 0:
        return [float('nan')] * len(ranks)
    k = np.sort(key_of(v.view(np.uint32)))
    out = []
    for r in ranks:
        kk = np.uint32(k[r])
        u = (kk & np.uint32(0x7FFFFFFF)) if kk & np.uint32(0x80000000) else ~kk
        out.append(np.array([u], np.uint32).view(np.float32)[0])
    return out


def bin_index(v, lo, hi, bins):
    """THE BIN RULE: (bin of every in-range finite value, below count, above count), all arithmetic in float32 with one
    rounding per operation."""
    lo, hi = np.float32(lo), np.float32(hi)
    below, above = v < lo, v > hi
    w = v[~(below | above)]
    if hi == lo:
        b = np.zeros(w.size, np.int64)
    else:
        with np.errstate(over='ignore'):
            scale = np.float32(bins) / (hi - lo)                       # float32 / float32: one rounding
            t = (w - lo) * scale                                       # float32 array ops: one rounding each
        b = np.minimum(np.floor(np.minimum(t, np.float32(bins - 1))).astype(np.int64), bins - 1)
    return b, int(below.sum()), int(above.sum())


def histogram(v, lo, hi, bins):
    b, below, above = bin_index(v, lo, hi, bins)
    return np.bincount(b, minlength=bins).astype(np.uint64), below, above


def stats(x, bins=0, range=None, median=False, quantiles=()):
    """What TensorStats.read() returns for one tensor."""
    v, n_nan, n_inf = finite_values(x)
    n = v.size
    d = v.astype(np.float64)
    nan = float('nan')
    out = {'numel': int(np.asarray(x).size), 'finite': n, 'nan': n_nan, 'inf': n_inf,
           'zeros': int((v == 0).sum()), 'negative': int((v < 0).sum()),
           'min': float(v.min()) if n else nan, 'max': float(v.max()) if n else nan,
           'absmax': float(np.abs(v).max()) if n else nan,
           'mean': float(d.mean()) if n else nan, 'absmean': float(np.abs(d).mean()) if n else nan,
           'std': float(d.std(ddof=1)) if n > 1 else nan}
    if bins:
        lo, hi = (out['min'], out['max']) if range is None else range
        if n:
            out['hist'], out['below'], out['above'] = histogram(v, lo, hi, bins)
        else:
            out['hist'], out['below'], out['above'] = np.zeros(bins, np.uint64), 0, 0
    if median:
        out['median'] = float(select(v, [rank_of(0.5, n)])[0]) if n else nan
    if quantiles:
        out['quantiles'] = [float(a) for a in select(v, [rank_of(q, n) for q in quantiles])] if n else [nan] * len(quantiles)
    return out


# ---- inputs
def normal(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def log_uniform(n, seed):
    """Magnitudes log-uniform in [1e-6, 1e2] with random sign, about 10 % exact zeros: the gradient generator of
    tests/optim_reference.py."""
    import optim_reference
    return optim_reference.make_grads([(n,)], seed)[0]


def sprinkle(x, seed, share=0.01):
    """A copy of float32 x with about `share` of the elements replaced by NaN, +inf and -inf (a third each)."""
    rng = np.random.default_rng(seed)
    x = x.copy()
    at = rng.random(x.size) < share
    what = rng.integers(0, 3, x.size)
    x[at & (what == 0)] = np.nan
    x[at & (what == 1)] = np.inf
    x[at & (what == 2)] = -np.inf
    return x
