"""fp64 numpy models of ampnet_amd.tsne (include/ampconv.h, "t-SNE"): the perplexity search, the joint probabilities,
the gradient with its error, one gains / momentum step and the whole loop -- scikit-learn 1.7.2's
_binary_search_perplexity, _joint_probabilities_nn, _kl_divergence_bh(angle=0) and _gradient_descent restated.
TEST INFRASTRUCTURE: numpy only, nothing here runs on the device.  tests/test_tsne_cpu.py holds these models to
scikit-learn's recordings (tests/golden/tsne/, tools/make_golden_tsne.py); tests/test_gpu_tsne.py holds the kernels to
the models."""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tsne')
U = 2.0 ** -24                       # unit roundoff of fp32
EPS64 = float(np.finfo(np.float64).eps)
TINY32 = float(np.finfo(np.float32).tiny)
TOL = float(np.float32(1e-5))        # scikit-learn keeps both as C floats
EPS_SUM = float(np.float32(1e-8))
RUN, TILE, CHUNK, PART = 256, 1024, 4096, 1024       # AMPCONV_TSNE_*

#         name               shape     perplexity samples  seed head (rows whose probabilities are recorded)
CASES = (('tsne_rows_70x12', (70, 12), 5.0, 'rows', 115, 70),
         ('tsne_rows_300x40', (300, 40), 10.0, 'rows', 114, 120),
         ('tsne_rows_200x8', (200, 8), 30.0, 'rows', 76, 32),
         ('tsne_columns_40x64', (40, 64), 5.0, 'columns', 55, 64))


def load(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, name + '.npz')))


def blobs(n, d, seed, centers=5, spread=4.0):
    """float32 [n, d]: seeded Gaussian blobs, unit variance around `centers` centres drawn at scale `spread`; the
    samples are shuffled, so a blob is no contiguous run of ids."""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, spread, (centers, d))
    x = c[rng.integers(0, centers, n)] + rng.normal(0.0, 1.0, (n, d))
    return x.astype(np.float32)


def exact_neighbors(X, k):
    """(idx int64 [M, k], dist2 float64 [M, k]): the k nearest other rows of X (fp64), nearest first, ties to the
    smaller id."""
    X = np.asarray(X, np.float64)
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind='stable')[:, :k]
    return idx.astype(np.int64), np.take_along_axis(d2, idx, 1)


def search_model(dist2, perplexity):
    """_binary_search_perplexity on float32 distances [N, K], every column taking part: (P float64 [N, K], beta [N],
    margin) with margin = the smallest | |H - log perplexity| - 1e-5f | over all steps of all rows: how far the stop
    decision ever was from flipping.  The rows run side by side; each row's sums are added in order, as scikit-learn's
    loops add them."""
    d = np.asarray(dist2, np.float32).astype(np.float64)
    N, K = d.shape
    target = np.log(float(np.float32(perplexity)))
    P, at = np.zeros((N, K)), np.ones(N)
    beta, lo, hi = np.ones(N), np.full(N, -np.inf), np.full(N, np.inf)
    live = np.arange(N)
    margin = np.inf
    with np.errstate(under='ignore', over='ignore', invalid='ignore', divide='ignore'):
        for _ in range(100):
            b = beta[live]
            p = np.exp(-d[live] * b[:, None])
            s = np.cumsum(p, axis=1)[:, -1]
            s = np.where(s == 0.0, EPS_SUM, s)
            p = p / s[:, None]
            diff = (np.log(s) + b * np.cumsum(d[live] * p, axis=1)[:, -1]) - target
            P[live], at[live] = p, b
            fin = np.isfinite(diff)
            if fin.any():
                margin = min(margin, float(np.abs(np.abs(diff[fin]) - TOL).min()))
            stop = np.abs(diff) <= TOL
            up = diff > 0.0
            l, h = lo[live], hi[live]
            l = np.where(up, b, l)
            h = np.where(up, h, b)
            nb = np.where(up, np.where(h == np.inf, b * 2.0, (b + h) / 2.0), np.where(l == -np.inf, b / 2.0, (b + l) / 2.0))
            lo[live], hi[live], beta[live] = l, h, nb
            live = live[~stop]
            if live.size == 0:
                break
    return P, at, float(margin)


def cond_f32(P):
    """float32 of the conditional probabilities as ampconv_tsne_affinities writes them: rounded, but a positive value
    never to 0 (the smallest denormal instead): whether a pair is an entry of P is decided in fp64."""
    f = np.asarray(P, np.float64).astype(np.float32)
    f[(np.asarray(P) > 0) & (f == 0)] = np.float32(2.0 ** -149)
    return f


def recorded_cond(f, X):
    """float32 [M, K] in the kernel's format: scikit-learn's recorded conditional probabilities for the first `head`
    rows and, where a fixture records only those, the search model on the exact distances for the rest; with it
    `pinned` (bool per entry of the recorded CSR): the entries whose row AND column are recorded rows, i.e. whose value
    follows from scikit-learn's own probabilities alone (all of them where head = M)."""
    head, k = int(f['head']), int(f['k'])
    _, d2 = exact_neighbors(X, k)
    cond = cond_f32(search_model(d2.astype(np.float32), float(f['perplexity']))[0])
    cond[:head] = f['cond_p']
    indptr = f['indptr'].astype(np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return cond, (rows < head) & (f['indices'].astype(np.int64) < head)


def joint_bound(rec):
    """|float32 val - scikit-learn's float32 val| from float32 conditional probabilities: each of p_ij, p_ji is
    scikit-learn's fp64 value rounded once (u = 2^-24 relative), so is their sum; the total over all pairs, a sum of
    positive terms, is off by at most u relative; the quotient by 2u; our rounding to float32 adds u, the recording's own
    rounding another: 4u = 2^-22 relative.  Below the normal range a float32 rounding is absolute, 2^-150 each:
    2^-148 covers the four."""
    return 2.0 ** -22 * np.asarray(rec, np.float64) + 2.0 ** -148


def search_sensitivity(dist2, perplexity, B):
    """float64 [N, K]: per conditional probability, a first-order bound (doubled for the second order) on its RELATIVE
    difference between two searches whose distances differ by at most B and that both stop inside the tolerance.
    At fixed beta, d ln p_j = -beta dd_j + beta sum_k p_k dd_k, at most 2 beta B.  H moves by dH / dd_j = -beta^2 p_j
    (d_j - dbar), at most beta^2 B sd in all; both searches end with |H - log perplexity| <= 1e-5 and dH / dbeta =
    -beta var, so |dbeta| <= (2e-5 + beta^2 B sd) / (beta var); d ln p_j / dbeta = -(d_j - dbar).  The bound is large
    for the far tail of a row (|d_j - dbar| of many sd), and rightly so: those probabilities do move by that much
    when a stop decision falls the other way; they are small in absolute terms."""
    P, beta, _ = search_model(dist2, perplexity)
    d = np.asarray(dist2, np.float32).astype(np.float64)
    mean = (P * d).sum(1)
    var = (P * (d - mean[:, None]) ** 2).sum(1)
    dbeta = (2.0 * TOL + beta ** 2 * B * np.sqrt(var)) / (beta * var)
    return 2.0 * ((2.0 * beta * B)[:, None] + dbeta[:, None] * np.abs(d - mean[:, None]))


def joint_sensitivity(idx, dist2, perplexity, B):
    """float64 [N, N]: the ABSOLUTE bound on an entry (i, j) of the joint P that search_sensitivity implies: P_ij =
    (p_ij + p_ji) / 2N (every row of p sums to 1 whatever the search did), so (p_ij e_ij + p_ji e_ji) / 2N."""
    P, _, _ = search_model(dist2, perplexity)
    A = P * search_sensitivity(dist2, perplexity, B)
    N = P.shape[0]
    S = np.zeros((N, N))
    np.put_along_axis(S, np.asarray(idx, np.int64), A, 1)
    return (S + S.T) / (2.0 * N)


def joint_model(idx, cond):
    """The CSR of (P + P^T) / max(sum, eps) from neighbour ids [N, K] and conditional probabilities [N, K]:
    (indptr int64 [N + 1], indices int64, values float64), indices ascending within a row; a pair whose fp64 sum is
    exactly 0 (both exponentials underflowed) is no entry."""
    idx = np.asarray(idx, np.int64)
    N, K = idx.shape
    rows = np.repeat(np.arange(N, dtype=np.int64), K)
    cols = idx.reshape(-1)
    v = np.asarray(cond, np.float64).reshape(-1)
    key = np.concatenate((rows * N + cols, cols * N + rows))
    val = np.concatenate((v, v))
    uniq, inv = np.unique(key, return_inverse=True)
    out = np.zeros(uniq.size)
    np.add.at(out, inv, val)
    uniq, out = uniq[out != 0.0], out[out != 0.0]      # scipy's P + P.T stores no entry whose sum is exactly 0
    out /= max(out.sum(), EPS64)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(uniq // N, minlength=N), out=indptr[1:])
    return indptr, (uniq % N).astype(np.int64), out


def repulsion_model(y):
    """fp64: (neg_f [N, 2], Z, abs_f [N, 2] = sum_j |q^2 (y_i - y_j)|, zrow [N]) with j = i excluded by index."""
    y = np.asarray(y, np.float64)
    N = y.shape[0]
    neg, absf, zrow = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros(N)
    for b in range(0, N, 512):
        d = y[b:b + 512, None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(2))
        q[np.arange(b, min(b + 512, N)) - b, np.arange(b, min(b + 512, N))] = 0.0
        t = (q * q)[:, :, None] * d
        neg[b:b + 512], absf[b:b + 512], zrow[b:b + 512] = t.sum(1), np.abs(t).sum(1), q.sum(1)
    return neg, float(zrow.sum()), absf, zrow


def attraction_model(y, indptr, indices, val, exaggeration, Z):
    """fp64: (pos_f [N, 2], abs_f [N, 2], error, abs_error); the values are float32(exaggeration * float32 val) as the
    kernel forms them."""
    y = np.asarray(y, np.float64)
    N = y.shape[0]
    p = (np.float32(exaggeration) * np.asarray(val, np.float32)).astype(np.float64)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    d = y[rows] - y[indices]
    q = 1.0 / (1.0 + (d * d).sum(1))
    t = (p * q)[:, None] * d
    pos, absf = np.zeros((N, 2)), np.zeros((N, 2))
    np.add.at(pos, rows, t)
    np.add.at(absf, rows, np.abs(t))
    with np.errstate(divide='ignore', invalid='ignore'):
        e = p * np.log(np.maximum(p, TINY32) / np.maximum(q / Z, TINY32))
    return pos, absf, float(e.sum()), float(np.abs(e).sum())


def gradient_model(y, indptr, indices, val, exaggeration=1.0):
    """_kl_divergence_bh(angle=0) in fp64: (error, grad [N, 2])."""
    neg, Z, _, _ = repulsion_model(y)
    pos, _, err, _ = attraction_model(y, indptr, indices, val, exaggeration, max(Z, EPS64))
    return err, 4.0 * (pos - neg / max(Z, EPS64))


def gains_fp32(update, grad, gains, min_gain=0.01):
    """The gains statement of _gradient_descent in float32, as numpy and the kernel both evaluate it."""
    update, grad, gains = (np.asarray(a, np.float32) for a in (update, grad, gains))
    inc = update * grad < 0
    g = np.where(inc, gains + np.float32(0.2), gains * np.float32(0.8)).astype(np.float32)
    return np.maximum(g, np.float32(min_gain))


def step_model(y, update, gains, grad, momentum, learning_rate, min_gain=0.01):
    """One _gradient_descent update in fp64 from a given gradient: (y_out, update, gains, sum (gains grad)^2).  The
    gain DECISION is the fp64 sign of update * grad."""
    y, update, gains, grad = (np.asarray(a, np.float64) for a in (y, update, gains, grad))
    g = np.where(update * grad < 0, gains + np.float64(np.float32(0.2)), gains * np.float64(np.float32(0.8)))
    g = np.maximum(g, float(np.float32(min_gain)))
    gg = grad * g
    un = momentum * update - learning_rate * gg
    return y + un, un, g, float((gg * gg).sum())


def descend(objective, it, max_iter, n_iter_without_progress, min_grad_norm, n_iter_check=50):
    """_gradient_descent's control flow around objective(i, want_error) -> (error, grad_norm): (error, i)."""
    error, best_error, best_iter, i = np.inf, np.inf, it, it
    for i in range(it, max_iter):
        check = (i + 1) % n_iter_check == 0
        want = check or i == max_iter - 1
        e, gn = objective(i, want)
        if want:
            error = e
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if gn <= min_grad_norm:
                break
    return error, i


def loop_model(y0, indptr, indices, val, learning_rate, early_exaggeration=12.0, max_iter=1000,
               n_iter_without_progress=300, min_grad_norm=1e-7, dtype=np.float64):
    """TSNE._tsne: 250 iterations at momentum 0.5 on early_exaggeration P, the rest at 0.8 on P, update and gains
    reset in between; the state in `dtype`, the gradient in fp64.  Returns (y, error, n_iter)."""
    state = {'y': np.asarray(y0, dtype).copy()}

    def stage(exag, momentum):
        state['u'], state['g'] = np.zeros_like(state['y']), np.ones_like(state['y'])

        def objective(i, want):
            err, grad = gradient_model(state['y'], indptr, indices, val, exag)
            y, u, g, gn2 = step_model(state['y'], state['u'], state['g'], grad, momentum, learning_rate)
            state['y'], state['u'], state['g'] = y.astype(dtype), u.astype(dtype), g.astype(dtype)
            return err, np.sqrt(gn2)
        return objective

    error, it = descend(stage(early_exaggeration, 0.5), 0, 250, 250, min_grad_norm)
    e2, it = descend(stage(1.0, 0.8), it + 1, max_iter, n_iter_without_progress, min_grad_norm)
    return state['y'], (e2 if np.isfinite(e2) else error), it


def kl_model(y, indptr, indices, val):
    """The final KL divergence of an embedding under P, in fp64."""
    return gradient_model(y, indptr, indices, val, 1.0)[0]


def neighbor_preservation_model(x, y, k):
    """The mean share of each row's k nearest in x that are among its k nearest in y (fp64, exact)."""
    a, _ = exact_neighbors(x, k)
    b, _ = exact_neighbors(y, k)
    return float(np.mean([len(set(a[i]) & set(b[i])) / k for i in range(a.shape[0])]))


# ---- bounds of the kernels' summation structure (docstrings of tests/test_gpu_tsne.py derive the constants)
C_NEG = RUN + 16
C_Z = RUN + 8
C_POS = 32


def step_bounds(pos_abs, t, gains, grad, update, y_out, momentum, learning_rate):
    """(E_grad, E_update, E_y): elementwise bounds on the kernel's gradient, update and y_out against the fp64 model
    given the same inputs.  pos_abs = sum |terms| of the attractive sum, t = pos - neg / Z."""
    e_grad = 4.0 * (C_POS * U * pos_abs + 2.0 * U * np.abs(t))
    gg = np.abs(gains * grad)
    e_upd = learning_rate * (gains * e_grad + 3.0 * U * (gg + gains * e_grad)) + 3.0 * U * np.abs(momentum * update) + U * np.abs(
        momentum * update - learning_rate * gains * grad)
    return e_grad, e_upd, e_upd + 2.0 * U * (np.abs(y_out) + e_upd)


# ---- the inputs of the call-by-call GPU tests (tests/test_gpu_tsne.py); tests/test_tsne_cpu.py asserts the conditions on
# them that those tests rely on
AFFINITY_SWEEP = ((2, 1), (2, 2), (3, 2), (3, 31), (63, 31), (63, 64), (64, 63), (64, 65), (65, 64), (65, 91), (257, 65),
                  (257, 256), (2, 256), (64, 1))


def affinity_case(N, K):
    """(dist2 float32 [N, K], perplexity): sorted gamma-distributed rows; row 0 is all zeros, row N - 1 underflows
    every exponential at beta = 1 (exp(-800) = 0 in fp64)."""
    rng = np.random.default_rng(1000 * N + K)
    d = np.sort(rng.gamma(4.0, 1.0, (N, K)), axis=1).astype(np.float32)
    d[0] = 0.0
    d[N - 1] = 800.0 + np.arange(K)
    return d, (1.0 if K == 1 else 1.5 if K < 6 else K / 3.0)


def embedding_case(N, kind, seed=0):
    """float32 [N, 2] without coincident points: 'start' (scale 1e-4), 'wide' (scale 50), 'outlier' (scale 3 and one
    point at 1e4)."""
    rng = np.random.default_rng(77 * N + seed)
    y = rng.normal(0.0, {'start': 1e-4, 'wide': 50.0, 'outlier': 3.0}[kind], (N, 2)).astype(np.float32)
    if kind == 'outlier':
        y[N // 2] = (1e4, -1e4)
    assert np.unique(y, axis=0).shape[0] == N
    return y


STEP_N = 2300
STEP_ROWS = (0, 1, 63, 64, 65, STEP_N - 1, 5, 0, 1100)       # two rows longer than a part: three parts and two


def step_case(seed):
    """Random y, update, gains and a CSR with the row lengths STEP_ROWS, then random lengths below 40: a dict of numpy
    arrays (val sums to 1, neg_f float32 and Z from repulsion_model)."""
    rng = np.random.default_rng(seed)
    N = STEP_N
    lens = np.concatenate((STEP_ROWS, rng.integers(0, 40, N - len(STEP_ROWS))))
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    cols = []
    for i, n in enumerate(lens):
        c = np.sort(rng.choice(N - 1, int(n), replace=False))
        cols.append(c + (c >= i))
    indices = np.concatenate(cols).astype(np.int64)
    val = rng.uniform(0.2, 1.0, indices.size)
    val = (val / val.sum()).astype(np.float32)
    y = rng.normal(0.0, 3.0, (N, 2)).astype(np.float32)
    update = rng.normal(0.0, 0.5, (N, 2)).astype(np.float32)
    gains = rng.uniform(0.01, 3.0, (N, 2)).astype(np.float32)
    neg, Z, _, _ = repulsion_model(y)
    return dict(N=N, indptr=indptr, indices=indices, val=val, y=y, update=update, gains=gains, neg=neg.astype(np.float32), Z=Z)


def step_expectation(c, exaggeration, momentum, learning_rate, min_gain=0.01):
    """The fp64 model of one ampconv_tsne_step on a case (neg_f and Z as given) with its bounds: a dict with grad, gains,
    update, y_out, error, norm2, the elementwise bounds e_grad, e_update, e_y, e_error, and `band`, the elements whose
    gain decision the bound cannot tell (|grad| <= e_grad)."""
    Z = max(c['Z'], EPS64)
    pos, pabs, err, err_abs = attraction_model(c['y'], c['indptr'], c['indices'], c['val'], exaggeration, Z)
    t = pos - c['neg'].astype(np.float64) / Z
    grad = 4.0 * t
    y_out, un, g, norm2 = step_model(c['y'], c['update'], c['gains'], grad, momentum, learning_rate, min_gain)
    e_grad, e_upd, e_y = step_bounds(pabs, t, g, grad, c['update'].astype(np.float64), y_out, momentum, learning_rate)
    p = (np.float32(exaggeration) * c['val']).astype(np.float64)
    e_err = U * (25.0 * err_abs + 12.0 * p.sum())
    gg = np.abs(g * grad)
    d = g * e_grad + 2.0 * U * gg
    return dict(grad=grad, gains=g, update=un, y_out=y_out, error=err, norm2=norm2, e_grad=e_grad, e_update=e_upd, e_y=e_y,
                e_error=e_err, e_norm2=float((2.0 * gg * d + d * d).sum()), band=np.abs(grad) <= e_grad)
