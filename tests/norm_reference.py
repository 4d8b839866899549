"""numpy fp64 model of the four per-token LayerNorm operations, written from the text of include/ampconv.h ("per-token
LayerNorm sites").  The mask and the activations are those of tests/glue_reference.py.  It never calls the library.

x is [N, L * D] (or any shape whose rows hold whole tokens); T = N L tokens of D channels; gamma, beta [D] or None."""
import functools

import numpy as np

import glue_reference as glue

_keep_mask = functools.lru_cache(maxsize=4)(glue.keep_mask)          # read-only: the same mask serves many calls of a test


def _affine(gamma, beta, D):
    g = np.ones(D) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros(D) if beta is None else np.asarray(beta, np.float64)
    return g, b


def token_stats(x, D, eps):
    """(mu, rstd, xhat) of the tokens of x: [T], [T], [T, D]"""
    t = np.asarray(x, np.float64).reshape(-1, D)
    mu = t.mean(axis=1)
    var = ((t - mu[:, None]) ** 2).mean(axis=1)               # biased, from the centred values
    rstd = 1.0 / np.sqrt(var + eps)
    return mu, rstd, (t - mu[:, None]) * rstd[:, None]


def norm_fwd(x, D, gamma, beta, eps, activation, seed, p):
    """y (shape of x), stats [T, 2] = (mu, rstd)"""
    g, b = _affine(gamma, beta, D)
    mu, rstd, xhat = token_stats(x, D, eps)
    thr, scale = glue.mask_params(p)
    keep = _keep_mask(seed, thr, tuple(x.shape))
    y = np.where(keep, glue.act(xhat * g + b, activation).reshape(x.shape) * float(scale), 0.0)
    return y, np.stack([mu, rstd], axis=1)


def norm_bwd(x, dy, D, gamma, beta, eps, activation, seed, p):
    """dx (shape of x), dgamma [D], dbeta [D]"""
    g, b = _affine(gamma, beta, D)
    mu, rstd, xhat = token_stats(x, D, eps)
    thr, scale = glue.mask_params(p)
    keep = _keep_mask(seed, thr, tuple(x.shape)).reshape(-1, D)
    dz = np.where(keep, float(scale) * glue.act_slope(xhat * g + b, activation) * np.asarray(dy, np.float64).reshape(-1, D), 0.0)
    dxhat = dz * g
    dx = rstd[:, None] * (dxhat - dxhat.mean(axis=1, keepdims=True) - xhat * (dxhat * xhat).mean(axis=1, keepdims=True))
    return dx.reshape(x.shape), (dz * xhat).sum(axis=0), dz.sum(axis=0)


def norm_pool_fwd(x, L, D, gamma, beta, eps, activation, pooling, seed, p):
    """x [N, L * D] -> pooled [N, D], stats [N L, 2] (mean) or [N, 2] (token 0: only that token is normalised)"""
    y, stats = norm_fwd(x, D, gamma, beta, eps, activation, seed, p)
    y = y.reshape(-1, L, D)
    if pooling == 'mean':
        return y.mean(axis=1), stats
    return y[:, 0], stats.reshape(-1, L, 2)[:, 0]


def norm_pool_bwd(x, dpooled, L, D, gamma, beta, eps, activation, pooling, seed, p):
    """dx (shape of x), dgamma, dbeta: norm_bwd under dy[n, l] = dpooled[n] / L (mean) or dpooled[n] at l = 0 alone"""
    dy = np.zeros((x.shape[0], L, D))
    if pooling == 'mean':
        dy[:] = np.asarray(dpooled, np.float64)[:, None, :] / L
    else:
        dy[:, 0] = dpooled
    return norm_bwd(x, dy.reshape(x.shape), D, gamma, beta, eps, activation, seed, p)
