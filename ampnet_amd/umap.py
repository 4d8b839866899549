"""UMAP of node embeddings and features (csrc/umap.hip): the reference's visualization/UMAP_testing.ipynb,
`umap.UMAP(n_neighbors=15, n_components=2, min_dist=0.1, metric='euclidean').fit_transform(x)`, and its UMAP featuriser
(src/ampnet/utils/preprocess.py, `UMAP(n_neighbors=15, n_components=30, min_dist=0.1).fit_transform(x.T)`).

`umap(x, ...)` follows umap-learn 0.5's defaults as include/ampconv.h ("UMAP") restates them; that text and the fp64
model in tests/umap_reference.py are the specification, parity with umap-learn's bits is unpinned.  The neighbours come
from `tsne.nearest` (samples='rows': knn; samples='columns': pca.gram, the transpose is never formed), the smooth-kNN
calibration and the memberships from ampconv_umap_memberships, the fuzzy union from one library sort, the curve
parameters from a numpy fit on the host, and every epoch of the layout is one call, ampconv_umap_epoch: a SYNCHRONOUS
epoch in which every row gathers over its own CSR row (no scatter, no atomics), negative samples from the library's
counter-based stream.  The host reads nothing back during the layout; two runs give the same bits and another seed gives
other bits.  The start is PCA (there is no spectral start) or a given tensor.  There is no autograd and no CPU fallback:
what the kernels do not take raises ValueError.
"""
import math

import numpy as np
import torch

from . import _lib
from .graph import _stream
from .head import _rows
from .knn import MAX_D as KNN_MAX_D
from .pca import MAX_K as PCA_MAX_K, MAX_W as PCA_MAX_W, pca
from .tsne import SAMPLES, nearest

MAX_K, MAX_DIM, PART = _lib.UMAP_MAX_K, _lib.UMAP_MAX_DIM, _lib.UMAP_PART
NEGATIVE_SAMPLE_RATE, GAMMA = 5, 1.0                     # umap-learn's negative_sample_rate, repulsion_strength
_SUPPORTED = (f"supported: x [N, D] float32 or bfloat16 on the GPU, D <= {KNN_MAX_D} (samples='rows') or at most "
              f"{PCA_MAX_W} columns (samples='columns'), 2 <= n_neighbors <= min(samples, {MAX_K}), "
              f'2 <= n_components <= {MAX_DIM} (ampnet_amd has no CPU fallback)')


def find_ab_params(spread=1.0, min_dist=0.1):
    """(a, b): the least-squares fit of 1 / (1 + a x^(2b)) to y(x) = 1 for x < min_dist, else
    exp(-(x - min_dist) / spread), on x = linspace(0, 3 spread, 300) -- umap-learn's find_ab_params.  Levenberg-Marquardt
    from (1, 1) in numpy on the host (no scipy)."""
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
    lx = np.log(np.where(x > 0, x, 1.0))

    def curve(p):
        return 1.0 / (1.0 + p[0] * np.where(x > 0, x, 0.0) ** (2.0 * p[1]))

    p, lam = np.array([1.0, 1.0]), 1e-3
    cost = float(((y - curve(p)) ** 2).sum())
    for _ in range(500):
        f = curve(p)
        xp = np.where(x > 0, x, 0.0) ** (2.0 * p[1])
        J = np.stack((-xp * f * f, -p[0] * xp * 2.0 * lx * f * f), 1)
        A, g = J.T @ J, J.T @ (y - f)
        step = np.linalg.solve(A + lam * np.diag(np.diag(A)), g)
        new = p + step
        new_cost = float(((y - curve(new)) ** 2).sum()) if (new > 0).all() else math.inf
        if new_cost <= cost:
            done = np.abs(step).max() <= 1e-13 * np.abs(p).max()
            p, cost, lam = new, new_cost, max(lam / 10.0, 1e-15)
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


def memberships(idx, dist):
    """(memb float32 [M, k], sigma float64 [M], rho float64 [M]): umap-learn's smooth_knn_dist and
    compute_membership_strengths on idx int64 [M, k], dist float32 [M, k] (Euclidean distances, column 0 the sample
    itself at distance 0, nearest first; row-strided views are read in place), in fp64 on the device."""
    lib = _lib.load()
    idx, ldi = _rows(idx)
    dist, ldd = _rows(dist)
    M, k = dist.shape
    dev = dist.device
    memb = torch.empty(M, k, dtype=torch.float32, device=dev)
    sigma, rho = torch.empty(M, dtype=torch.float64, device=dev), torch.empty(M, dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib.ampconv_umap_memberships_workspace_bytes(M)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ampconv_umap_memberships(idx.data_ptr(), ldi, dist.data_ptr(), ldd, M, k, memb.data_ptr(), sigma.data_ptr(),
                                                rho.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), 'ampconv_umap_memberships')
    return memb, sigma, rho


def fuzzy_graph(idx, memb):
    """(indptr int64 [M + 1], indices int64 [nnz], val float32 [nnz]): the CSR of W = P + P^T - P o P^T for
    P[i, idx[i, j]] = memb[i, j] -- umap-learn's fuzzy union at set_op_mix_ratio = 1.  indices ascend within a row; exact
    zeros are no entries (the sample itself, whose membership is 0, among them); each value is (p + q) - p q in float32
    from the two float32 memberships, a missing one taken as 0, so W[i, j] and W[j, i] are the same bits.  The
    neighbours of a row have to be distinct ids.  One stable library sort of the 2 M k (row, column) keys."""
    M, k = idx.shape
    dev = idx.device
    rows = torch.arange(M, device=dev).repeat_interleave(k)
    cols = idx.reshape(-1)
    v = memb.reshape(-1)
    key, order = torch.sort(torch.cat((rows * M + cols, cols * M + rows)), stable=True)
    v = torch.cat((v, v))[order]
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    twice = torch.zeros_like(first)
    twice[:-1] = ~first[1:]                                   # the next key is the same pair from the other side
    q = torch.where(twice, torch.cat((v[1:], v.new_zeros(1))), v.new_zeros(()))
    w = (v + q) - v * q
    first &= w != 0
    key, w = key[first], w[first]
    indptr = torch.searchsorted(key, torch.arange(M + 1, device=dev) * M)
    return indptr, key % M, w.contiguous()


def _quotient(num, den):
    """float32 num / den, correctly rounded: the division in fp64 (53 >= 2 x 24 + 2 bits: rounding twice is harmless)."""
    return (num.double() / den.double()).float()


def schedule(indptr, indices, val, n_epochs):
    """(indptr, indices, eps float32): the entries that the layout samples -- those with w >= max(w) / n_epochs -- and
    their epochs per sample eps = max(w) / w (float32 divisions)."""
    wmax = val.max()
    keep = ~(val < _quotient(wmax, torch.tensor(float(n_epochs), device=val.device)))
    kept = torch.cat((indptr.new_zeros(1), torch.cumsum(keep, 0)))
    return kept[indptr].contiguous(), indices[keep].contiguous(), _quotient(wmax, val[keep]).contiguous()


def scaled_start(y):
    """float32 [M, d]: every column of y mapped to [0, 10], 10 (y - min) / (max - min) in float32 (0 where a column is
    constant), as umap-learn does before its optimiser."""
    y = y.float()
    lo, hi = y.min(dim=0).values, y.max(dim=0).values
    span = hi - lo
    scaled = _quotient(10.0 * (y - lo), torch.where(span > 0, span, torch.ones_like(span)))
    return torch.where(span > 0, scaled, torch.zeros_like(y)).contiguous()


class Layout:
    """The device state of the optimiser: y in two buffers, the sampled CSR with eps, next, nextneg, drawn.  epoch(n)
    is ampconv_umap_epoch for epoch n of n_epochs; part (tests): the part length, through ampconv_umap_epoch_split."""

    def __init__(self, y0, indptr, indices, eps, a, b, n_epochs, seed, gamma=GAMMA, part=None):
        self.lib = _lib.load()
        dev = y0.device
        self.M, self.dim, self.nnz = y0.size(0), y0.size(1), indices.numel()
        self.y = [y0.clone().contiguous(), torch.empty_like(y0)]
        self.indptr, self.indices, self.eps = indptr.contiguous(), indices.contiguous(), eps.contiguous()
        self.next = self.eps.clone()
        self.nextneg = _quotient(self.eps, torch.tensor(float(NEGATIVE_SAMPLE_RATE), device=dev)).contiguous()
        self.drawn = torch.zeros(self.nnz, dtype=torch.int32, device=dev)
        self.a, self.b, self.gamma, self.n_epochs, self.seed, self.part = float(a), float(b), float(gamma), int(n_epochs), int(seed), part
        self.ws = torch.empty(max(int(self.lib.ampconv_umap_epoch_workspace_bytes(self.M, self.nnz, self.dim)), 256),
                              dtype=torch.uint8, device=dev)

    def epoch(self, n):
        lib, (y_in, y_out) = self.lib, self.y
        alpha = 1.0 - n / self.n_epochs
        head = (y_in.data_ptr(), y_out.data_ptr(), self.M, self.dim, self.indptr.data_ptr(), self.indices.data_ptr(), self.nnz,
                self.eps.data_ptr(), self.next.data_ptr(), self.nextneg.data_ptr(), self.drawn.data_ptr(), self.a, self.b,
                self.gamma, alpha, n, self.seed & (2 ** 64 - 1))
        with torch.cuda.device(y_in.device):
            tail = (self.ws.data_ptr(), self.ws.numel(), _stream())
            if self.part is None:
                _lib.check(lib.ampconv_umap_epoch(*head, *tail), 'ampconv_umap_epoch')
            else:
                _lib.check(lib.ampconv_umap_epoch_split(*head, int(self.part), *tail), 'ampconv_umap_epoch_split')
        self.y = [y_out, y_in]


class UMAPResult:
    """embedding float32 [M, n_components]; graph = (indptr, indices, val), the CSR of the fuzzy union W; sigma, rho
    float64 [M], the calibration; a, b, the curve; n_epochs as run."""

    def __init__(self, embedding, graph, sigma, rho, a, b, n_epochs):
        self.embedding, self.graph, self.sigma, self.rho = embedding, graph, sigma, rho
        self.a, self.b, self.n_epochs = a, b, n_epochs


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def _check(x, n_components, n_neighbors, min_dist, spread, n_epochs, init, samples, seed, a, b, neighbors_):
    if samples not in SAMPLES:
        raise ValueError(f'umap: samples must be one of {SAMPLES}, got {samples!r}')
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f'umap: x has to be a 2-d tensor; {_SUPPORTED}')
    if x.dtype not in _lib.DTYPES:
        raise ValueError(f'umap: x is {x.dtype}; {_SUPPORTED}')
    if x.requires_grad:
        raise ValueError('umap: x requires grad, and UMAP has no autograd: its inputs are data (pass x.detach())')
    R, W = x.shape
    M = R if samples == 'rows' else W
    if samples == 'rows' and W > KNN_MAX_D:
        raise ValueError(f'umap: x has {W} columns, the neighbour search takes at most {KNN_MAX_D}: reduce them first, '
                         f"e.g. ampnet_amd.pca(x, 50).scores (samples='rows')")
    if samples == 'columns' and not 1 <= W <= PCA_MAX_W:
        raise ValueError(f'umap: x has {W} columns; {_SUPPORTED}')
    if M < 2 or R < 1 or W < 1:
        raise ValueError(f'umap: {M} samples; at least 2 are needed')
    if isinstance(n_components, bool) or not isinstance(n_components, int) or not 2 <= n_components <= MAX_DIM:
        raise ValueError(f'umap: n_components = {n_components!r} has to be an integer in [2, {MAX_DIM}]')
    if isinstance(n_neighbors, bool) or not isinstance(n_neighbors, int) or not 2 <= n_neighbors <= min(M, MAX_K):
        raise ValueError(f'umap: n_neighbors = {n_neighbors!r} has to be an integer in [2, min({M} samples, {MAX_K})] '
                         '(the sample itself counts as its first neighbour)')
    if not _number(spread) or not spread > 0:
        raise ValueError(f'umap: spread = {spread!r} has to be a positive number')
    if not _number(min_dist) or not 0 <= min_dist <= spread:
        raise ValueError(f'umap: min_dist = {min_dist!r} has to lie in [0, spread = {spread}]')
    if n_epochs is not None and (isinstance(n_epochs, bool) or not isinstance(n_epochs, int) or not 1 <= n_epochs <= 1 << 24):
        raise ValueError(f'umap: n_epochs = {n_epochs!r} has to be None or a positive integer')
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f'umap: seed = {seed!r} has to be an integer')
    if (a is None) != (b is None) or (a is not None and not (_number(a) and _number(b) and a > 0 and b > 0)):
        raise ValueError(f'umap: a = {a!r}, b = {b!r} have to be both None (fitted from spread and min_dist) or both positive')
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32 or tuple(init.shape) != (M, n_components) or init.device != x.device:
            raise ValueError(f'umap: init has to be a float32 [{M}, {n_components}] tensor on the device of x, got {init.dtype} '
                             f'{tuple(init.shape)} on {init.device}')
    elif not isinstance(init, str) or init != 'pca':
        raise ValueError(f"umap: init = {init!r} has to be 'pca' or a float32 [{M}, {n_components}] tensor (there is no "
                         'spectral and no random start)')
    elif n_components > min(R, W, PCA_MAX_K):
        raise ValueError(f"umap: init='pca' gives at most min(samples, features) = {min(R, W)} components, n_components is "
                         f'{n_components}: pass an init tensor')
    if neighbors_ is not None:
        ok = isinstance(neighbors_, (tuple, list)) and len(neighbors_) == 2 and all(isinstance(t, torch.Tensor) for t in neighbors_)
        if ok:
            idx, dist = neighbors_
            ok = (idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.dim() == 2 and idx.shape == dist.shape
                  and idx.size(0) == M and 2 <= idx.size(1) <= min(M, MAX_K) and idx.device == x.device == dist.device)
        if not ok:
            raise ValueError(f'umap: neighbors has to be (idx int64 [{M}, k], dist float32 [{M}, k]) on the device of x, column 0 '
                             f'the sample itself at distance 0, 2 <= k <= min({M}, {MAX_K})')
    if not x.is_cuda:
        raise ValueError(f'umap: x has to be on the GPU; {_SUPPORTED}')
    return M


def neighbors_with_self(x, n_neighbors, samples='rows'):
    """(idx int64 [M, k], dist float32 [M, k]), k = n_neighbors: column 0 the sample itself at distance 0, then its k - 1
    nearest other samples (tsne.nearest) as Euclidean distances, nearest first."""
    idx, d2 = nearest(x, n_neighbors - 1, samples)
    M = idx.size(0)
    idx = torch.cat((torch.arange(M, device=idx.device)[:, None], idx), 1)
    return idx.contiguous(), torch.cat((d2.new_zeros(M, 1), d2.sqrt()), 1).contiguous()


def umap(x, n_components=2, *, n_neighbors=15, min_dist=0.1, spread=1.0, n_epochs=None, init='pca', samples='rows', seed=0,
         a=None, b=None, neighbors=None):
    """umap-learn's UMAP(n_neighbors, n_components, min_dist, spread, metric='euclidean') at its other defaults, of X = x
    (samples='rows': embeddings [N, D], D <= 256) or of X = x^T, never formed (samples='columns': the reference's
    featuriser, at most 2048 columns), as include/ampconv.h ("UMAP") specifies it: synchronous epochs, negative samples
    from the counter-based stream under `seed`.  n_epochs: None is 500 up to 10000 samples, else 200.  init: 'pca' (there
    is no spectral start) or a float32 [M, n_components] tensor, mapped per column to [0, 10] either way.  a, b: the
    curve, fitted from spread and min_dist if None.  neighbors=(idx, dist) bypasses the neighbour search (its k replaces
    n_neighbors).  Returns a UMAPResult; nothing carries a gradient, two runs give the same bits, and invalid arguments
    raise ValueError before any launch."""
    M = _check(x, n_components, n_neighbors, min_dist, spread, n_epochs, init, samples, seed, a, b, neighbors)
    x = x.detach()
    idx, dist = neighbors if neighbors is not None else neighbors_with_self(x, n_neighbors, samples)
    if bool(((idx < 0) | (idx >= M)).any()):
        raise ValueError('umap: some samples have fewer neighbours than asked for (rows of x with NaN?) or ids out of range')
    memb, sigma, rho = memberships(idx, dist)
    indptr, indices, val = fuzzy_graph(idx, memb)
    if indices.numel() == 0:
        raise ValueError('umap: the fuzzy graph has no entry (distances with NaN?)')
    if a is None:
        a, b = find_ab_params(spread, min_dist)
    n_epochs = (500 if M <= 10000 else 200) if n_epochs is None else n_epochs
    y0 = scaled_start(init if isinstance(init, torch.Tensor) else pca(x, n_components, samples=samples).scores)
    state = Layout(y0, *schedule(indptr, indices, val, n_epochs), a, b, n_epochs, seed)
    for n in range(n_epochs):
        state.epoch(n)
    return UMAPResult(state.y[0], (indptr, indices, val), sigma, rho, float(a), float(b), n_epochs)
