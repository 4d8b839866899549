"""numpy fp64 model of the nearest-neighbour search (include/ampconv.h, "nearest neighbours"): the three metrics, the
candidate rule, the strict order through the 64-bit key encoding, the empty slots, and the three wrappers."""
import os

import numpy as np

METRICS = {'dot': 0, 'cosine': 1, 'l2': 2}
KNN_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'knn')


def clamp_ids(ids, N):
    return np.clip(np.asarray(ids, dtype=np.int64), 0, N - 1)


def goodness(x, qid, kid, metric):
    """g [Q, S] in fp64 of the rows as given; NaN where the contract's g (L2: the value before the max) is NaN."""
    x = np.asarray(x, dtype=np.float64)
    a, b = x[qid], x[kid]
    with np.errstate(invalid='ignore', over='ignore'):
        dot = a @ b.T
        if metric == 'dot':
            return dot
        sa, sb = (a * a).sum(1), (b * b).sum(1)
        if metric == 'cosine':
            ra, rb = 1.0 / np.maximum(np.sqrt(sa), 1e-12), 1.0 / np.maximum(np.sqrt(sb), 1e-12)
            return dot * ra[:, None] * rb[None, :]
        if metric == 'l2':
            e = sa[:, None] + sb[None, :] - 2.0 * dot
            return np.where(np.isnan(e), np.nan, -np.maximum(e, 0.0))
    raise ValueError(metric)


def float_image(g32):
    """The order-preserving unsigned image of float32 values (-0 as +0); NaN has none and must be masked by the caller."""
    u = np.asarray(g32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = np.where(u == 0x80000000, 0, u)
    return np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000).astype(np.uint64)


def encode_keys(g32, s):
    """64-bit keys: high word the image of g, low word ~s.  A larger key is a better pair under (g descending, s ascending)."""
    return (float_image(g32) << np.uint64(32)) | ((~np.asarray(s, dtype=np.uint64)) & np.uint64(0xFFFFFFFF))


def candidates(g, qid, kid, exclude_self):
    cand = ~np.isnan(g)
    if exclude_self:
        cand &= kid[None, :] != qid[:, None]
    return cand


def knn(x, k, queries=None, keys=None, metric='dot', exclude_self=False):
    """(idx int64 [Q, k], score fp64 [Q, k], g [Q, S], cand [Q, S], pos int64 [Q, k]): the contract in fp64.  Ties in the
    fp64 g go to the earlier key position.  pos is the key position of every slot (-1: empty)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    qid = np.arange(N) if queries is None else clamp_ids(queries, N)
    kid = np.arange(N) if keys is None else clamp_ids(keys, N)
    Q, S = len(qid), len(kid)
    g = goodness(x, qid, kid, metric) if Q and S else np.zeros((Q, S))
    cand = candidates(g, qid, kid, exclude_self)
    idx = np.full((Q, k), -1, dtype=np.int64)
    pos = np.full((Q, k), -1, dtype=np.int64)
    score = np.full((Q, k), np.inf if metric == 'l2' else -np.inf)
    for q in range(Q):
        c = np.flatnonzero(cand[q])
        gq = g[q, c] + 0.0                                     # -0 counts as +0
        order = c[np.lexsort((c, -gq))][:k]                    # g descending, then position ascending
        idx[q, :len(order)] = kid[order]
        pos[q, :len(order)] = order
        score[q, :len(order)] = -g[q, order] + 0.0 if metric == 'l2' else g[q, order]
    return idx, score, g, cand, pos


def knn_graph(x, k, metric='l2', loop=True):
    N = np.asarray(x).shape[0]
    m = k + 1 if loop else k
    idx = knn(x, m, metric=metric, exclude_self=not loop)[0]
    return np.stack((np.repeat(np.arange(N), m), np.sort(idx, axis=1).reshape(-1)))


def vote(idx, y, num_classes):
    out = np.full(idx.shape[0], -1, dtype=np.int64)
    for q in range(idx.shape[0]):
        lab = y[idx[q][idx[q] >= 0]]
        if len(lab):
            out[q] = np.bincount(lab, minlength=num_classes).argmax()      # the first maximum: the smaller class id
    return out


def knn_classify(z, y, k, queries=None, keys=None, metric='cosine', exclude_self=True, num_classes=None):
    y = np.asarray(y, dtype=np.int64)
    C = int(y.max()) + 1 if num_classes is None else num_classes
    return vote(knn(z, k, queries, keys, metric, exclude_self)[0], y, C)


def check_rows(got_idx, got_score, x, k, queries, keys, metric, exclude_self, tol_of, tag=''):
    """The four checks of tests/test_gpu_knn.py on EVERY row of a result against the fp64 model of the same inputs.
    tol_of(want, scale) -> tolerance; scale: 1 (cosine), max(1, max |score|) (dot), max(1, max(|a|^2 + |b|^2)) (l2).
    Returns the largest share of the tolerance a score used."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    qid = np.arange(N) if queries is None else clamp_ids(queries, N)
    kid = np.arange(N) if keys is None else clamp_ids(keys, N)
    Q, S = len(qid), len(kid)
    got_idx, got_score = np.asarray(got_idx), np.asarray(got_score)
    assert got_idx.shape == (Q, k) and got_score.shape == (Q, k), f'{tag}: shapes {got_idx.shape}, {got_score.shape}'
    want_idx, want_score, g, cand, _ = knn(x, k, queries, keys, metric, exclude_self)
    if Q == 0:
        return 0.0
    if metric == 'cosine':
        scale = 1.0
    elif metric == 'dot':
        scale = max(1.0, float(np.abs(np.where(cand, g, 0.0)).max()) if S else 1.0)
    else:
        sq = (x * x).sum(1)
        with np.errstate(invalid='ignore'):
            both = sq[qid][:, None] + sq[kid][None, :]
        scale = max(1.0, float(np.nanmax(np.where(cand, both, 0.0))) if S else 1.0)
    unique_keys = len(np.unique(kid)) == S
    where = np.full(N, -1, dtype=np.int64)                     # node -> its key position, where no node repeats
    where[kid] = np.arange(S)
    sign = -1.0 if metric == 'l2' else 1.0
    empty_score = np.inf if metric == 'l2' else -np.inf
    used = 0.0
    for q in range(Q):
        n_cand = int(cand[q].sum())
        n = min(k, n_cand)
        ids, sc = got_idx[q], got_score[q]
        # 1. the empty slots are exactly the trailing k - #candidates; the others are distinct candidates
        assert (ids[n:] == -1).all() and (sc[n:] == empty_score).all(), f'{tag} row {q}: empty slots {ids}, {sc}'
        assert (ids[:n] >= 0).all(), f'{tag} row {q}: {ids} with {n_cand} candidates'
        # a node id may repeat in the key list: a returned slot is identified by its key POSITION, recovered as the
        # not yet used position of that node whose fp64 goodness is nearest the returned score
        pos = np.full(n, -1, dtype=np.int64)
        taken = np.zeros(S, dtype=bool)
        if unique_keys:
            assert (ids[:n] < N).all(), f'{tag} row {q}: node ids {ids}'
            pos = where[ids[:n]]
            assert (pos >= 0).all() and cand[q, pos].all() and len(set(pos.tolist())) == n, \
                f'{tag} row {q}: {ids} are not distinct candidates'
            taken[pos] = True
        else:
            for j in range(n):
                at = np.flatnonzero((kid == ids[j]) & cand[q] & ~taken)
                assert len(at), f'{tag} row {q} slot {j}: node {ids[j]} is no (further) candidate'
                pos[j] = at[0]                                 # equal node, equal row, equal g: the earliest one left
                taken[pos[j]] = True
        # 2. the scores are those of the pairs
        want = sign * g[q, pos]
        tol = tol_of(want, scale)
        err = np.abs(sc[:n].astype(np.float64) - want)
        assert (err <= tol).all(), f'{tag} row {q}: score error {err.max():.3e} over {tol[err.argmax()]:.3e}'
        if n:
            used = max(used, float((err / tol).max()))
        # 3. the kernel's own (score, position) sequence is strictly ordered by the rule, bitwise on the fp32 values
        keys64 = encode_keys(sign * sc[:n].astype(np.float32), pos)
        assert (keys64[:-1] > keys64[1:]).all(), f'{tag} row {q}: not strictly ordered: {sc[:n]}, positions {pos}'
        # 4. optimality within 2 tol
        if n:
            gq = g[q, pos]
            kth = sign * want_score[q, n - 1]
            assert (gq >= kth - 2 * tol_of(np.full(n, kth), scale)).all(), f'{tag} row {q}: a neighbour worse than the k-th best'
            rest = cand[q] & ~taken
            if rest.any():
                worst = gq.min()
                assert (g[q, rest] <= worst + 2 * tol_of(g[q, rest], scale)).all(), \
                    f'{tag} row {q}: a candidate better than the worst returned was left out'
    return used
