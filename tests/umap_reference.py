"""fp64 numpy models of ampnet_amd.umap (include/ampconv.h, "UMAP"): the curve fit, the smooth-kNN calibration with the
memberships, the fuzzy union, the schedule and the layout epoch in BOTH its forms -- umap-learn's scatter (head and tail
of a fired entry both move) with the positions frozen for the epoch, and the gather the kernels run (every row walks its
own CSR row, the attraction doubled).  No umap source exists on any machine: this file and the header ARE the
specification, umap-learn 0.5's defaults restated.  TEST INFRASTRUCTURE: numpy only, nothing here runs on the device.
tests/test_umap_cpu.py holds the models to their invariants (and the fit to scipy where it is installed);
tests/test_gpu_umap.py holds the kernels to the models.

What is integer-exact -- firing decisions, the number of negative samples m, the drawn ids, and the float32 schedule
state next / nextneg / drawn -- is computed here in the kernels' own number formats (np.float32 operations round once
each, as the header's statements do); the positions are fp64."""
import math

import numpy as np

from pipeline_reference import draw
from tsne_reference import U, exact_neighbors, neighbor_preservation_model      # noqa: F401  (the tests take them from here)

MAX_K, MAX_DIM, PART, MAX_NEGATIVES = 256, 32, 1024, 65536       # AMPCONV_UMAP_*
NEGATIVE_SAMPLE_RATE = np.float32(5)
F32 = np.float32

# The relative error of the kernels' two coefficients against fp64 over d2 in [1e-12, 1e4] at the default curve, as
# tools/bench_umap.py measured it on an MI355X (profiles/umap.md, "coefficients": 3.736e-6, the attraction at d2 ~ 1e-12,
# where b log2(d2) ~ -36 carries the float32 rounding of the product into the exponent); the epoch test's margin is 4 x this.
R_COEFF = 3.74e-6
R_MARGIN = 4.0


# ---------------------------------------------------------------------------------------------------------- the curve
def find_ab_params(spread=1.0, min_dist=0.1):
    """(a, b): Gauss-Newton with step halving from (1, 1) on the 300 points of the header's curve."""
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    xs = x[1:]                                                # x = 0: the curve is 1 for every (a, b), no residual
    lx = np.log(xs)

    def resid(p):
        return y[1:] - 1.0 / (1.0 + p[0] * xs ** (2.0 * p[1]))

    p = np.array([1.0, 1.0])
    for _ in range(200):
        t = xs ** (2.0 * p[1])
        f = 1.0 / (1.0 + p[0] * t)
        J = np.stack((-t * f * f, -p[0] * t * 2.0 * lx * f * f), 1)
        step = np.linalg.lstsq(J, resid(p), rcond=None)[0]
        scale, cost = 1.0, float((resid(p) ** 2).sum())
        while scale > 1e-10 and not ((p + scale * step > 0).all() and float((resid(p + scale * step) ** 2).sum()) <= cost):
            scale /= 2.0
        if scale <= 1e-10:
            break
        p = p + scale * step
        if np.abs(scale * step).max() <= 1e-14 * np.abs(p).max():
            break
    return float(p[0]), float(p[1])


# ----------------------------------------------------------------------------------------------- neighbours, memberships
def neighbors_with_self(X, k):
    """(idx int64 [M, k], dist float32 [M, k]): column 0 the sample itself at distance 0, then the k - 1 nearest other
    samples (fp64, exact), float32 sqrt of the float32 squared distance."""
    idx, d2 = exact_neighbors(X, k - 1)
    M = idx.shape[0]
    return (np.concatenate((np.arange(M, dtype=np.int64)[:, None], idx), 1),
            np.concatenate((np.zeros((M, 1), F32), np.sqrt(d2.astype(F32))), 1))


def smooth_knn(dist):
    """(sigma, rho, psum, floored): the header's calibration of float32 distances [M, k] in fp64, row by row; psum is
    the sum of the last round and floored says where the floor replaced the search's sigma."""
    dist = np.asarray(dist, F32).astype(np.float64)
    M, k = dist.shape
    target = math.log2(k)
    total = 0.0
    for i in range(M):                                        # a fixed order: the rows' sums, then the rows
        total += float(dist[i].sum())
    mean_all = total / (float(M) * float(k))
    sigma, rho, psum, floored = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M, bool)
    for i in range(M):
        d = dist[i]
        pos = d[d > 0]
        r = float(pos.min()) if pos.size else 0.0
        lo, hi, mid = 0.0, math.inf, 1.0
        x = d[1:] - r
        for _ in range(64):
            with np.errstate(over='ignore'):
                ps = float(np.where(x > 0, np.exp(-(x / mid)), 1.0).sum())
            if abs(ps - target) < 1e-5:
                break
            if ps > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == math.inf else (lo + hi) / 2.0
        floor = 1e-3 * (float(d.sum()) / k if r > 0 else mean_all)
        sigma[i], rho[i], psum[i], floored[i] = max(mid, floor), r, ps, floor > mid
    return sigma, rho, psum, floored


def memberships_model(idx, dist):
    """(memb float64 [M, k], sigma, rho): the header's memberships before the rounding to float32."""
    sigma, rho, _, _ = smooth_knn(dist)
    d = np.asarray(dist, F32).astype(np.float64)
    x = d - rho[:, None]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        memb = np.where((x <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(x / sigma[:, None])))
    memb[np.asarray(idx) == np.arange(d.shape[0])[:, None]] = 0.0
    return memb, sigma, rho


def fuzzy_model(idx, memb32):
    """(indptr, indices, val float32): the CSR of P + P^T - P o P^T from float32 memberships, each value (p + q) - p q
    in float32, exact zeros dropped, indices ascending.  A dict walk: nothing here is the code under test's sort."""
    idx, memb32 = np.asarray(idx), np.asarray(memb32, F32)
    M, k = idx.shape
    P = {}
    for i in range(M):
        for j in range(k):
            P[(i, int(idx[i, j]))] = memb32[i, j]
    rows = [[] for _ in range(M)]
    for (i, j) in set(P) | {(j, i) for (i, j) in P}:
        p, q = P.get((i, j), F32(0)), P.get((j, i), F32(0))
        w = F32(F32(p + q) - F32(p * q))
        if w != 0:
            rows[i].append((j, w))
    indptr, indices, val = [0], [], []
    for i in range(M):
        for j, w in sorted(rows[i]):
            indices.append(j)
            val.append(w)
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int64), np.array(val, F32)


# ------------------------------------------------------------------------------------------------------- the schedule
def schedule_model(indptr, indices, val, n_epochs):
    """(indptr, indices, eps float32) of the sampled entries: w >= max(w) / n_epochs, eps = max(w) / w in float32."""
    val = np.asarray(val, F32)
    wmax = val.max()
    keep = ~(val < wmax / F32(n_epochs))
    kept = np.concatenate(([0], np.cumsum(keep)))
    return kept[np.asarray(indptr)].astype(np.int64), np.asarray(indices)[keep].astype(np.int64), (wmax / val[keep]).astype(F32)


class State:
    """The schedule state of the sampled entries: next, nextneg float32, drawn int32, and the rows of the entries."""

    def __init__(self, indptr, indices, eps):
        self.indptr, self.indices, self.eps = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(eps, F32)
        self.rows = np.repeat(np.arange(len(self.indptr) - 1), np.diff(self.indptr))
        self.next = self.eps.copy()
        self.nextneg = (self.eps / NEGATIVE_SAMPLE_RATE).astype(F32)
        self.drawn = np.zeros(self.eps.size, np.int32)

    def copy(self):
        s = State.__new__(State)
        s.indptr, s.indices, s.eps, s.rows = self.indptr, self.indices, self.eps, self.rows
        s.next, s.nextneg, s.drawn = self.next.copy(), self.nextneg.copy(), self.drawn.copy()
        return s


def attract_coeff(d2, a, b):
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return np.where(d2 > 0, -2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0), 0.0)


def repel_coeff(d2, a, b, gamma=1.0):
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        return np.where(d2 > 0, 2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0)), 0.0)


def fired(st, n):
    """(the entries that fire in epoch n, their number of negative samples m): float32 statements, as the header's."""
    nf = F32(n)
    e = np.nonzero(st.next <= nf)[0]
    epn = (st.eps[e] / NEGATIVE_SAMPLE_RATE).astype(F32)
    with np.errstate(divide='ignore', invalid='ignore'):
        m = np.clip(np.trunc((nf - st.nextneg[e]).astype(F32) / epn), 0, MAX_NEGATIVES).astype(np.int64)
    return e, epn, m


def advance(st, e, epn, m):
    st.next[e] = (st.next[e] + st.eps[e]).astype(F32)
    st.nextneg[e] = (st.nextneg[e] + (m.astype(F32) * epn).astype(F32)).astype(F32)
    st.drawn[e] += m.astype(np.int32)


def epoch_gather(Y, st, n, n_epochs, a, b, seed, gamma=1.0):
    """One epoch in the kernels' form, positions in fp64: (Y_out, info).  Row j of a fired entry (j -> k) receives
    2 clip(c (Y_j - Y_k)) alpha and its negatives clip(c (Y_j - Y_s)) alpha; st moves on.  a, b, gamma and alpha are the
    float32 values the C call receives.  info: per row the number of unit contributions (an attraction counts 2), the
    sum of the terms' magnitudes per coordinate, and how often d2 = 0 met an edge and a negative sample."""
    Y = np.asarray(Y, np.float64)
    M = Y.shape[0]
    a, b, gamma = float(F32(a)), float(F32(b)), float(F32(gamma))
    alpha = float(F32(1.0 - n / n_epochs))
    e, epn, m = fired(st, n)
    rows, cols = st.rows[e], st.indices[e]
    out, mag, count = np.zeros_like(Y), np.zeros_like(Y), np.zeros(M)
    d = Y[rows] - Y[cols]
    d2 = (d * d).sum(1)
    t = 2.0 * np.clip(attract_coeff(d2, a, b)[:, None] * d, -4.0, 4.0) * alpha
    np.add.at(out, rows, t)
    np.add.at(mag, rows, np.abs(t))
    np.add.at(count, rows, 2.0)
    zero_edges, zero_negatives, ids = int((d2 == 0).sum()), 0, []
    for p in range(int(m.max()) if m.size else 0):
        sel = m > p
        ee = e[sel]
        s = (draw(seed, ee, st.drawn[ee].astype(np.int64) + p) % np.uint64(M)).astype(np.int64)
        ids.append((ee, np.full(ee.size, p), s))
        d = Y[st.rows[ee]] - Y[s]
        d2 = (d * d).sum(1)
        zero_negatives += int((d2 == 0).sum())
        t = np.clip(repel_coeff(d2, a, b, gamma)[:, None] * d, -4.0, 4.0) * alpha
        np.add.at(out, st.rows[ee], t)
        np.add.at(mag, st.rows[ee], np.abs(t))
        np.add.at(count, st.rows[ee], 1.0)
    advance(st, e, epn, m)
    return Y + out, dict(count=count, mag=mag, fired=e, m=m, zero_edges=zero_edges, zero_negatives=zero_negatives, ids=ids,
                         alpha=alpha)


def epoch_scatter(Y, st, n, n_epochs, a, b, seed, gamma=1.0):
    """The same epoch in umap-learn's form with the positions FROZEN for the epoch: a fired entry (j -> k) moves its head
    j by clip(c (Y_j - Y_k)) alpha and its tail k by minus that (move_other); the negatives move the head only.  An
    explicit loop over the fired entries.  Returns Y_out; st moves on."""
    Y = np.asarray(Y, np.float64)
    M = Y.shape[0]
    a, b, gamma = float(F32(a)), float(F32(b)), float(F32(gamma))
    alpha = float(F32(1.0 - n / n_epochs))
    e, epn, m = fired(st, n)
    out = Y.copy()
    for t, ent in enumerate(e):
        j, k = int(st.rows[ent]), int(st.indices[ent])
        d = Y[j] - Y[k]
        g = np.clip(float(attract_coeff((d * d).sum(), a, b)) * d, -4.0, 4.0)
        out[j] += g * alpha
        out[k] -= g * alpha
        for p in range(int(m[t])):
            s = int(draw(seed, int(ent), int(st.drawn[ent]) + p) % np.uint64(M))
            d = Y[j] - Y[s]
            out[j] += np.clip(float(repel_coeff((d * d).sum(), a, b, gamma)) * d, -4.0, 4.0) * alpha
    advance(st, e, epn, m)
    return out


def epoch_bound(info, y_out, dim, b, r=R_COEFF):
    """The elementwise bound on the kernel's Y_out against epoch_gather's.  With T the row's unit contributions, each at
    most 4 alpha in magnitude, and S the sum of the terms' magnitudes:
      T 4 alpha (R_MARGIN r + kappa (dim + 3) u)   the coefficients: r is their measured relative error (R_COEFF) under
                                                   the issue's margin of 4, and d2 itself is a float32 sum of dim
                                                   squares of differences rounded once each ((dim + 3) u relative),
                                                   which moves a coefficient by at most kappa = 1 + max(b, 1) times
                                                   that (|d ln c / d ln d2| <= 1 + b for both);
      (T + 16) u S                                 the sums: a lane adds at most T terms in order in float32, each an FMA
                                                   of a product rounded twice (clip argument, doubling exact), the
                                                   butterfly has six levels, the groups are added in fp64;
      2 u |y_out|                                  the final rounding to float32 (and the float32 input exactly read)."""
    T = info['count'][:, None]
    kappa = 1.0 + max(float(b), 1.0)
    return T * 4.0 * info['alpha'] * (R_MARGIN * r + kappa * (dim + 3) * U) + (T + 16.0) * U * info['mag'] + 2.0 * U * np.abs(y_out)


def scaled_start_model(y):
    """float32 [M, d]: every column mapped to [0, 10] in float32 statements, 0 where a column is constant."""
    y = np.asarray(y, F32)
    lo, hi = y.min(0), y.max(0)
    span = (hi - lo).astype(F32)
    safe = np.where(span > 0, span, F32(1))
    return np.where(span > 0, (F32(10) * (y - lo).astype(F32)).astype(F32) / safe, F32(0)).astype(F32)


def pca_start_model(X, dim):
    """float32 [M, dim]: the first dim PCA scores of X (fp64 SVD, signs as scikit-learn's svd_flip on u), scaled."""
    X = np.asarray(X, np.float64)
    Xc = X - X.mean(0)
    u, s, vt = np.linalg.svd(Xc, full_matrices=False)
    return scaled_start_model((u[:, :dim] * s[:dim]).astype(F32))


def layout_model(y0, indptr, indices, val, a, b, n_epochs, seed, upto=None):
    """(Y fp64 after `upto` epochs (all if None) of epoch_gather from the scaled start y0, the state)."""
    st = State(*schedule_model(indptr, indices, val, n_epochs))
    Y = np.asarray(y0, np.float64)
    for n in range(n_epochs if upto is None else upto):
        Y, _ = epoch_gather(Y, st, n, n_epochs, a, b, seed)
    return Y, st


def fit_model(X, dim=2, n_neighbors=15, n_epochs=None, seed=0, y0=None, min_dist=0.1, spread=1.0):
    """The whole model pipeline on exact neighbours: a dict with embedding, y0, the graph, sigma, rho, a, b."""
    X = np.asarray(X, np.float64)
    idx, dist = neighbors_with_self(X, n_neighbors)
    memb, sigma, rho = memberships_model(idx, dist)
    indptr, indices, val = fuzzy_model(idx, memb.astype(F32))
    a, b = find_ab_params(spread, min_dist)
    n_epochs = (500 if X.shape[0] <= 10000 else 200) if n_epochs is None else n_epochs
    y0 = pca_start_model(X, dim) if y0 is None else scaled_start_model(y0)
    Y, _ = layout_model(y0, indptr, indices, val, a, b, n_epochs, seed)
    return dict(embedding=Y, y0=y0, graph=(indptr, indices, val), sigma=sigma, rho=rho, a=a, b=b, n_epochs=n_epochs)


# ------------------------------------------------------------------------------------------------------------- cases
def clusters_case(seed=7):
    """float32 [300, 16]: six well-separated unit Gaussian clusters whose centres lie so that the first two principal
    axes cannot tell two pairs of them apart: centres 0 / 1 and 2 / 3 differ only along axes of small variance (12 apart
    in coordinates 2 and 3), while coordinates 0 and 1 carry the large spread (40) between the three groups."""
    rng = np.random.default_rng(seed)
    c = np.zeros((6, 16))
    c[0, :2], c[1, :2] = (0, 0), (0, 0)
    c[2, :2], c[3, :2] = (40, 0), (40, 0)
    c[4, :2], c[5, :2] = (0, 40), (40, 40)
    c[1, 2], c[3, 3] = 12, 12
    lab = np.arange(300) % 6
    rng.shuffle(lab)
    return (c[lab] + rng.normal(0.0, 1.0, (300, 16))).astype(F32), lab


def hub_neighbors(M, k, seed, D=5):
    """(X float32 [M, D], idx, dist): exact neighbours of random points, then sample 0 made every other row's NEAREST
    neighbour (at half the row's smallest distance; where 0 was a neighbour already its old column goes, else the last):
    row 0 of the fuzzy graph has M - 1 entries of weight 1, more than a part of 64 from M = 66 on.  Rows keep distinct
    ids and ascending distances."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (M, D)).astype(F32)
    idx, dist = neighbors_with_self(X, k)
    for i in range(1, M):
        others = [(int(j), float(d)) for j, d in zip(idx[i, 1:], dist[i, 1:]) if j != 0][:k - 2]
        idx[i, 1:] = [0] + [j for j, _ in others]
        dist[i, 1:] = [0.5 * dist[i, 1]] + [d for _, d in others]
    return X, idx, dist
