"""numpy fp64 model of masked feature modelling, written from the contract in include/ampconv.h ("MASKED FEATURE
MODELLING").  It never calls the library: tests/test_mfm_cpu.py holds it to torch's CPU composite and autograd in double,
tests/test_gpu_mfm_kernels.py and tests/test_gpu_mfm.py hold the kernels to it."""
import numpy as np

from pipeline_reference import build_tokens_f32, draw

TOKEN, VALUE = 0, 1                                        # AMPCONV_MFM_*
SHIFT = 32                                                 # AMPCONV_MFM_LOSS_SHIFT
U32 = 2.0 ** -24                                           # unit roundoff of fp32


def threshold_of(rate):
    return int(round(float(rate) * 65536))


def token_mask(idx, seed, threshold):
    """THE TOKEN MASK: bool [N, L]; token (n, l) is masked iff idx[n, l] >= 0 and (draw(seed, n, l) >> 48) < threshold."""
    idx = np.asarray(idx)
    N, L = idx.shape
    if N == 0:
        return np.zeros((0, L), dtype=bool)
    r = draw(seed, np.arange(N)[:, None], np.arange(L)[None, :])
    return ((r >> np.uint64(48)).astype(np.int64) < int(threshold)) & (idx >= 0)


def build(x, mean, inv_std, idx, table, mask_token, masked, mode):
    """(out float32 [N, L, De + 1] before any rounding to the storage, masked bool [N, L] -- the given one ANDed with
    idx >= 0 --, target float32 [N, L]).  Unmasked tokens are the featuriser's (pipeline_reference.build_tokens_f32)."""
    idx = np.asarray(idx)
    token = np.asarray(mask_token, np.float32).reshape(-1)
    out = build_tokens_f32(x, mean, inv_std, idx, table)
    De = out.shape[-1] - 1
    target = out[..., De].copy()                           # z of every token; 0 where idx == -1
    masked = np.asarray(masked).astype(bool) & (idx >= 0)
    if mode == TOKEN:
        out[masked] = token
    else:
        out[masked, De] = token[De]
    return out, masked, target


def token_grad(dout, masked, mode):
    """(dmask_token [De + 1] fp64, S: the sum of the absolute values of its terms)."""
    dout, masked = np.asarray(dout, np.float64), np.asarray(masked).astype(bool)
    rows = dout[masked]                                    # [count, De + 1]
    g, S = rows.sum(axis=0), np.abs(rows).sum(axis=0)
    if mode == VALUE:
        g[:-1], S[:-1] = 0.0, 0.0
    return g, S


def fixed_sum(resid32):
    """state[0] of loss_fwd from ITS fp32 residuals: sum of rint(r * r * 2^32), the square taken in fp64 (exact)."""
    r = np.asarray(resid32, np.float32).astype(np.float64).reshape(-1)
    return int(np.rint(r * r * 2.0 ** SHIFT).astype(np.int64).sum())


def loss_fwd(h, masked, target, w, b):
    """{'resid' fp64 [N, L] (0 for unmasked tokens), 'count', 'loss'}; rows of unmasked tokens are never touched."""
    masked = np.asarray(masked).astype(bool)
    N, L = masked.shape
    w = np.asarray(w, np.float64).reshape(-1)
    h = np.asarray(h).reshape(N, L, w.size)
    resid = np.zeros((N, L))
    rows = h[masked].astype(np.float64)
    resid[masked] = rows @ w + float(np.asarray(b).reshape(-1)[0]) - np.asarray(target, np.float64)[masked]
    count = int(masked.sum())
    return {'resid': resid, 'count': count, 'loss': float((resid[masked] ** 2).sum() / max(count, 1))}


def loss_bwd(h, masked, resid, w, count, g=1.0):
    """{'dh' [N, L, D], 'dw' [D], 'db', 'S_dw' [D], 'S_db': the sums of the absolute values of the terms of dw and db} for
    c = 2 g / max(count, 1) and the given residuals."""
    masked = np.asarray(masked).astype(bool)
    N, L = masked.shape
    w = np.asarray(w, np.float64).reshape(-1)
    h = np.asarray(h).reshape(N, L, w.size)
    coef = 2.0 * float(g) / max(int(count), 1) * np.asarray(resid, np.float64)[masked]      # [count]
    rows = h[masked].astype(np.float64)
    dh = np.zeros((N, L, w.size))
    dh[masked] = coef[:, None] * w[None, :]
    terms = coef[:, None] * rows
    return {'dh': dh, 'dw': terms.sum(axis=0), 'db': float(coef.sum()), 'S_dw': np.abs(terms).sum(axis=0),
            'S_db': float(np.abs(coef).sum())}
