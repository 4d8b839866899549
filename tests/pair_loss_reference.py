"""numpy fp64 model of the pair loss (include/ampconv.h, "pair loss"): forward, backward and walk_pairs."""
import numpy as np


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def clamp_ids(ids, N):
    return np.clip(np.asarray(ids, dtype=np.int64), 0, N - 1)


def forward(z, anchor, positive, negative, weight=None, kind='skipgram', scale=1.0, neg_weight=1.0, exclude_anchor=False):
    """(loss, aff [B], neg_term [B], pi [B, S], c [B]) in fp64; pi and c are what backward() needs."""
    z = np.asarray(z, dtype=np.float64)
    N = z.shape[0]
    B = len(anchor)
    if B == 0:
        return 0.0, np.zeros(0), np.zeros(0), np.zeros((0, len(negative))), np.zeros(0)
    ia, ip, ineg = clamp_ids(anchor, N), clamp_ids(positive, N), clamp_ids(negative, N)
    a, p, n = z[ia], z[ip], z[ineg]
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64)
    aff = scale * (a * p).sum(1)
    g = scale * (a @ n.T)
    kept = np.ones(g.shape, dtype=bool)
    if exclude_anchor:
        kept = ineg[None, :] != ia[:, None]
    if kind == 'skipgram':
        m = np.where(kept, g, -np.inf).max(1)
        any_kept = np.isfinite(m)
        m = np.where(any_kept, m, 0.0)
        e = np.where(kept, np.exp(np.where(kept, g - m[:, None], 0.0)), 0.0)
        s = e.sum(1)
        neg_term = np.where(any_kept, m + np.log(np.where(any_kept, s, 1.0)), 0.0)     # no kept negative: 0
        pi = e / np.where(any_kept, s, 1.0)[:, None]
        c = -np.ones(B)
        rows = neg_term - aff
    elif kind == 'xent':
        neg_term = np.where(kept, softplus(g), 0.0).sum(1)
        pi = np.where(kept, neg_weight * sigmoid(g), 0.0)
        c = -sigmoid(-aff)
        rows = softplus(-aff) + neg_weight * neg_term
    else:
        raise ValueError(kind)
    return float((w * rows).sum()), aff, neg_term, pi, c


def backward(z, anchor, positive, negative, weight=None, kind='skipgram', scale=1.0, neg_weight=1.0, exclude_anchor=False,
             g0=1.0):
    """dz [N, D] in fp64 for the upstream gradient g0 of the summed loss."""
    z = np.asarray(z, dtype=np.float64)
    N = z.shape[0]
    dz = np.zeros_like(z)
    B = len(anchor)
    if B == 0:
        return dz
    _, _, _, pi, c = forward(z, anchor, positive, negative, weight, kind, scale, neg_weight, exclude_anchor)
    ia, ip, ineg = clamp_ids(anchor, N), clamp_ids(positive, N), clamp_ids(negative, N)
    a, p, n = z[ia], z[ip], z[ineg]
    w = np.ones(B) if weight is None else np.asarray(weight, dtype=np.float64)
    np.add.at(dz, ia, g0 * scale * w[:, None] * (pi @ n + c[:, None] * p))
    np.add.at(dz, ip, g0 * scale * (w * c)[:, None] * a)
    np.add.at(dz, ineg, g0 * scale * ((pi * w[:, None]).T @ a))
    return dz


def walk_pairs(walks, node_idx=None, window=1, symmetric=False):
    """The pairs (walks[w, i], walks[w, i + k]), k-major, then walk, then i -- as a Python loop."""
    walks = np.asarray(walks)
    a, p = [], []
    for k in range(1, window + 1):
        for w in range(walks.shape[0]):
            for i in range(walks.shape[1] - k):
                a.append(int(walks[w, i]))
                p.append(int(walks[w, i + k]))
    if node_idx is not None:
        where = {int(v): j for j, v in enumerate(np.asarray(node_idx))}
        a, p = [where[v] for v in a], [where[v] for v in p]
    if symmetric:
        a, p = a + p, p + a
    return np.asarray(a, dtype=np.int64), np.asarray(p, dtype=np.int64)


def make_inputs(N, D, B, S, amp=1.0, seed=0):
    """z ~ N(0, 1) amp / D^0.25 (fp32), uniform ids, weights in [0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((N, D)) * amp / D ** 0.25).astype(np.float32)
    anchor = rng.integers(0, N, B, dtype=np.int64)
    positive = rng.integers(0, N, B, dtype=np.int64)
    negative = rng.integers(0, N, S, dtype=np.int64)
    weight = (0.5 + rng.random(B)).astype(np.float32)
    return z, anchor, positive, negative, weight
