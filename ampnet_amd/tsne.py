"""t-SNE of node embeddings and features (csrc/tsne.hip): the reference's visualization/plot_TSNE_2D_plot.py,
`TSNE(n_components=2, perplexity=10, learning_rate=10).fit_transform(x.T)`, and the standard picture of what
`AMPGCN.embed` and `pair_loss` produce.

`tsne(x, ...)` computes what scikit-learn 1.7.2's `TSNE(method='barnes_hut', init='pca')` computes with the repulsive
term summed exactly (its own code at angle = 0), for two output dimensions.  The neighbours come from `knn`
(samples='rows') or from `pca.gram` (samples='columns': the samples are the columns of x, the transpose is never
formed), the conditional affinities from ampconv_tsne_affinities, the joint probabilities from one library sort, and
every iteration is two calls: ampconv_tsne_repulsion (the N x N Student-t term, tiled on chip, never written) and
ampconv_tsne_step (attraction over the CSR of P, gains, momentum).  The host reads two numbers back every 50 iterations.
With exact PCA as the start nothing is random: two runs give the same bits.  The contract is include/ampconv.h,
"t-SNE".  There is no autograd and no CPU fallback: what the kernels do not take raises ValueError.
"""
import math

import torch

from . import _lib
from .graph import _stream
from .head import _rows
from .knn import MAX_D as KNN_MAX_D, MAX_K as KNN_MAX_K, knn
from .pca import MAX_W as PCA_MAX_W, gram, pca

SAMPLES = ('rows', 'columns')
MAX_K = _lib.TSNE_MAX_K
MAX_PERPLEXITY = (MAX_K - 1) / 3.0                       # int(3 perplexity + 1) neighbours have to fit MAX_K
EXPLORATION_ITER, N_ITER_CHECK, MIN_GAIN = 250, 50, 0.01   # scikit-learn's _EXPLORATION_MAX_ITER, _N_ITER_CHECK, min_gain
_SUPPORTED = (f"supported: x [N, D] float32 or bfloat16 on the GPU, D <= {KNN_MAX_D} (samples='rows') or at most "
              f"{PCA_MAX_W} columns (samples='columns'), n_components = 2, perplexity < samples and <= "
              f'{MAX_PERPLEXITY:.0f} (ampnet_amd has no CPU fallback)')


def affinities(dist2, perplexity):
    """(p float32 [N, K], beta float64 [N]): scikit-learn's _binary_search_perplexity on squared distances [N, K]
    (float32, K <= 256, a row-strided view is read in place), in fp64 on the device."""
    lib = _lib.load()
    dist2, ldd = _rows(dist2)
    N, K = dist2.shape
    p = torch.empty(N, K, dtype=torch.float32, device=dist2.device)
    beta = torch.empty(N, dtype=torch.float64, device=dist2.device)
    with torch.cuda.device(dist2.device):
        _lib.check(lib.ampconv_tsne_affinities(dist2.data_ptr(), N, K, ldd, float(perplexity), p.data_ptr(), beta.data_ptr(),
                                               _stream()), 'ampconv_tsne_affinities')
    return p, beta


def joint_probabilities(idx, cond):
    """(indptr int64 [N + 1], indices int64 [nnz], val float32 [nnz]): the CSR of (P + P^T) / max(sum, eps) for
    P[i, idx[i, j]] = cond[i, j] -- scikit-learn's _joint_probabilities_nn.  indices ascend within a row; a pair that
    is a neighbour both ways appears once with the summed value; a pair whose probabilities are exactly 0 both ways is
    no entry, as in scipy's P + P.T (cond is float32: `affinities` writes a p that is positive in fp64 as a positive
    float32, and the zero test here reads the bits).  The neighbours of a row have to be distinct node ids
    other than the row.  One stable library sort of the 2 N K (row, column) keys, sums in fp64 in that order: bitwise
    reproducible."""
    N, K = idx.shape
    dev = idx.device
    rows = torch.arange(N, device=dev).repeat_interleave(K)
    cols = idx.reshape(-1)
    v = cond.reshape(-1).double()
    some = cond.reshape(-1).contiguous().view(torch.int32) != 0      # by the bits: ampconv_tsne_affinities never writes a
    key, order = torch.sort(torch.cat((rows * N + cols, cols * N + rows)), stable=True)      # positive p as 0
    v, some = torch.cat((v, v))[order], torch.cat((some, some))[order]
    first = torch.ones_like(key, dtype=torch.bool)
    first[1:] = key[1:] != key[:-1]
    twice = torch.zeros_like(first)
    twice[:-1] = ~first[1:]                                   # the next key is the same pair from the other side
    v = v + torch.where(twice, torch.cat((v[1:], v.new_zeros(1))), v.new_zeros(()))
    some = some | (twice & torch.cat((some[1:], some.new_zeros(1))))
    first &= some                                             # scipy's P + P.T stores no entry whose sum is exactly 0
    key, v = key[first], v[first]
    total = v.sum().clamp(min=torch.finfo(torch.float64).eps)
    indptr = torch.searchsorted(key, torch.arange(N + 1, device=dev) * N)
    return indptr, key % N, (v / total).float()


def _merged_neighbors(x, k):
    """knn stops at 64 neighbours: more come from knn over disjoint chunks of the keys (key s in chunk s mod C), the
    rows' candidates merged by a stable sort on the distance after one on the key id, so the earlier key wins a tie.
    A chunk that gave all its 64 candidates to a row may hide a closer key: then the number of chunks doubles, up to
    chunks of at most 64 keys, which hide nothing.  Reads one flag back per attempt (a one-time stage)."""
    N, cap = x.size(0), KNN_MAX_K
    exact_at = (N + cap - 1) // cap
    C = min(2 * ((k + cap - 1) // cap), exact_at)
    ids = torch.arange(N, device=x.device)
    while True:
        ci, cd = [], []
        for c in range(C):
            keys = ids[c::C].contiguous()
            i, d = knn(x, min(cap, keys.numel()), keys=keys, metric='l2', exclude_self=True)
            ci.append(i)
            cd.append(d)
        ci, cd = torch.cat(ci, 1), torch.cat(cd, 1)
        by_id = ci.masked_fill(ci < 0, N).sort(dim=1, stable=True)
        cd = cd.gather(1, by_id.indices)
        by_d = cd.sort(dim=1, stable=True)
        idx, d2 = by_id.values.gather(1, by_d.indices)[:, :k].contiguous(), by_d.values[:, :k].contiguous()
        if C >= exact_at:
            return idx, d2
        used = torch.zeros(N, C, dtype=torch.int64, device=x.device).scatter_add_(1, idx % C, torch.ones_like(idx))
        if not bool((used >= cap).any()):
            return idx, d2
        C = min(2 * C, exact_at)


def nearest(x, k, samples='rows'):
    """(idx int64 [M, k], dist2 float32 [M, k]): every sample's k nearest other samples by squared Euclidean distance,
    nearest first.  'rows': knn(metric='l2', exclude_self=True), merged over key chunks above 64.  'columns': the
    distances from pca.gram(x) without a shift, G_ii + G_jj - 2 G_ij clamped at 0 in fp64, and torch.topk on that
    W x W matrix."""
    if samples == 'rows':
        if k <= KNN_MAX_K:
            return knn(x, k, metric='l2', exclude_self=True)
        return _merged_neighbors(x, k)
    G = gram(x)
    g = G.diagonal()
    d2 = (g[:, None] + g[None, :] - 2.0 * G).clamp_(min=0)
    d2.fill_diagonal_(float('inf'))
    d2, idx = torch.topk(d2, k, dim=1, largest=False, sorted=True)
    return idx, d2.float()


def neighbor_preservation(x, y, k):
    """The mean share of each point's k nearest in x [N, D] that are among its k nearest in y [N, d] (both from knn,
    squared Euclidean distance, the point itself excluded): a float in [0, 1]."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor) or x.dim() != 2 or y.dim() != 2 or x.size(0) != y.size(0):
        raise ValueError('neighbor_preservation: x [N, D] and y [N, d] have to be 2-d tensors with the same number of rows')
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(KNN_MAX_K, x.size(0) - 1):
        raise ValueError(f'neighbor_preservation: k = {k!r} with {x.size(0)} points; 1 <= k <= min({KNN_MAX_K}, N - 1)')
    a, _ = knn(x, k, metric='l2', exclude_self=True)
    b, _ = knn(y, k, metric='l2', exclude_self=True)
    hits = torch.zeros((), dtype=torch.float64, device=a.device)
    for r in range(0, a.size(0), 4096):
        hits += ((a[r:r + 4096, :, None] == b[r:r + 4096, None, :]) & (a[r:r + 4096, :, None] >= 0)).any(2).sum()
    return float(hits) / (a.size(0) * k)


class TSNEResult:
    """embedding float32 [M, 2]; kl_divergence (float, the error of the last iteration, as scikit-learn's
    kl_divergence_); n_iter (scikit-learn's n_iter_); affinities = (indptr, indices, val), the CSR of P; beta float64
    [M], the precisions of the perplexity search; learning_rate as used."""

    def __init__(self, embedding, kl_divergence, n_iter, affinities, beta, learning_rate):
        self.embedding, self.kl_divergence, self.n_iter = embedding, kl_divergence, n_iter
        self.affinities, self.beta, self.learning_rate = affinities, beta, learning_rate

    def standardized(self):
        """The reference script's second figure: StandardScaler().fit_transform(embedding), (y - mean) / std per
        column with the population std, 1 where it is 0."""
        y = self.embedding.double()
        std = y.std(dim=0, unbiased=False)
        return ((y - y.mean(dim=0)) / torch.where(std > 0, std, torch.ones_like(std))).float()


class Descent:
    """The device state of the iteration: y in two buffers, update, gains, the workspaces.  step() is one iteration
    (ampconv_tsne_repulsion, ampconv_tsne_step) and returns (error, gradient norm) if asked to, else None."""

    def __init__(self, y0, indptr, indices, val):
        self.lib = _lib.load()
        dev, N = y0.device, y0.size(0)
        self.N, self.nnz = N, indices.numel()
        self.y = [y0.clone().contiguous(), torch.empty_like(y0)]
        self.indptr, self.indices, self.val = indptr.contiguous(), indices.contiguous(), val.contiguous()
        self.neg = torch.empty(N, 2, dtype=torch.float32, device=dev)
        self.Z = torch.empty(1, dtype=torch.float64, device=dev)
        self.err = torch.empty(2, dtype=torch.float64, device=dev)
        self.ws_rep = torch.empty(max(int(self.lib.ampconv_tsne_repulsion_workspace_bytes(N)), 256), dtype=torch.uint8, device=dev)
        self.ws_step = torch.empty(max(int(self.lib.ampconv_tsne_step_workspace_bytes(N, self.nnz)), 256), dtype=torch.uint8,
                                   device=dev)
        self.reset()

    def reset(self):
        self.update, self.gains = torch.zeros_like(self.y[0]), torch.ones_like(self.y[0])

    def step(self, exaggeration, momentum, learning_rate, want_error):
        lib, (y_in, y_out) = self.lib, self.y
        with torch.cuda.device(y_in.device):
            s = _stream()
            _lib.check(lib.ampconv_tsne_repulsion(y_in.data_ptr(), self.N, self.neg.data_ptr(), self.Z.data_ptr(),
                                                  self.ws_rep.data_ptr(), self.ws_rep.numel(), s), 'ampconv_tsne_repulsion')
            _lib.check(lib.ampconv_tsne_step(y_in.data_ptr(), y_out.data_ptr(), self.update.data_ptr(), self.gains.data_ptr(),
                                             self.N, self.indptr.data_ptr(), self.indices.data_ptr(), self.val.data_ptr(),
                                             self.nnz, self.neg.data_ptr(), self.Z.data_ptr(), exaggeration, momentum,
                                             learning_rate, MIN_GAIN, self.err.data_ptr() if want_error else None,
                                             self.ws_step.data_ptr(), self.ws_step.numel(), s), 'ampconv_tsne_step')
        self.y = [y_out, y_in]
        if not want_error:
            return None
        e = self.err.cpu()                                       # the read-back: every 50 iterations and at the last
        return float(e[0]), math.sqrt(float(e[1]))


def descend(step, it, max_iter, n_iter_without_progress, min_grad_norm):
    """scikit-learn's _gradient_descent around step(want_error) -> (error, gradient norm) or None: (error, i).  The
    error is None if no iteration ran."""
    error, best_error, best_iter, i = None, math.inf, it, it
    for i in range(it, max_iter):
        check = (i + 1) % N_ITER_CHECK == 0
        out = step(check or i == max_iter - 1)
        if out is not None:
            error, grad_norm = out
        if check:
            if error < best_error:
                best_error, best_iter = error, i
            elif i - best_iter > n_iter_without_progress:
                break
            if grad_norm <= min_grad_norm:
                break
    return error, i


def _check(x, n_components, perplexity, early_exaggeration, learning_rate, max_iter, n_iter_without_progress,
           min_grad_norm, init, samples, neighbors_):
    if samples not in SAMPLES:
        raise ValueError(f'tsne: samples must be one of {SAMPLES}, got {samples!r}')
    if n_components != 2:
        raise ValueError(f'tsne: n_components = {n_components!r}: two output dimensions only (one degree of freedom, '
                         'q = 1 / (1 + d^2))')
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f'tsne: x has to be a 2-d tensor; {_SUPPORTED}')
    if x.dtype not in _lib.DTYPES:
        raise ValueError(f'tsne: x is {x.dtype}; {_SUPPORTED}')
    if x.requires_grad:
        raise ValueError('tsne: x requires grad, and t-SNE has no autograd: its inputs are data (pass x.detach())')
    R, W = x.shape
    M = R if samples == 'rows' else W
    if samples == 'rows' and W > KNN_MAX_D:
        raise ValueError(f'tsne: x has {W} columns, the neighbour search takes at most {KNN_MAX_D}: reduce them first, '
                         f"e.g. ampnet_amd.pca(x, 50).scores (samples='rows')")
    if samples == 'columns' and not 1 <= W <= PCA_MAX_W:
        raise ValueError(f'tsne: x has {W} columns; {_SUPPORTED}')
    if M < 2 or R < 1 or W < 1:
        raise ValueError(f'tsne: {M} samples; at least 2 are needed')
    for name, v in (('perplexity', perplexity), ('early_exaggeration', early_exaggeration), ('min_grad_norm', min_grad_norm)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f'tsne: {name} = {v!r} has to be a finite number')
    if not 0 < perplexity < M:
        raise ValueError(f'tsne: perplexity = {perplexity} has to be positive and less than the {M} samples')
    if int(3.0 * perplexity + 1) > MAX_K and M - 1 > MAX_K:
        raise ValueError(f'tsne: perplexity = {perplexity} needs {int(3.0 * perplexity + 1)} neighbours, at most {MAX_K} are taken')
    if early_exaggeration < 1:
        raise ValueError(f'tsne: early_exaggeration = {early_exaggeration} has to be at least 1')
    if learning_rate != 'auto' and (isinstance(learning_rate, (bool, str)) or not isinstance(learning_rate, (int, float))
                                    or not learning_rate > 0):
        raise ValueError(f"tsne: learning_rate = {learning_rate!r} has to be 'auto' or a positive number")
    for name, v, lo in (('max_iter', max_iter, EXPLORATION_ITER), ('n_iter_without_progress', n_iter_without_progress, 0)):
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise ValueError(f'tsne: {name} = {v!r} has to be an integer of at least {lo}')
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32 or tuple(init.shape) != (M, 2) or init.device != x.device:
            raise ValueError(f'tsne: init has to be a float32 [{M}, 2] tensor on the device of x, got {init.dtype} '
                             f'{tuple(init.shape)} on {init.device}')
    elif init != 'pca':
        raise ValueError(f"tsne: init = {init!r} has to be 'pca' or a float32 [{M}, 2] tensor (there is no random start)")
    elif min(R, W) < 2:
        raise ValueError(f"tsne: init='pca' needs at least 2 features, x is {tuple(x.shape)}")
    if neighbors_ is not None:
        ok = isinstance(neighbors_, (tuple, list)) and len(neighbors_) == 2 and all(isinstance(t, torch.Tensor) for t in neighbors_)
        if ok:
            idx, d2 = neighbors_
            ok = (idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.dim() == 2 and idx.shape == d2.shape
                  and idx.size(0) == M and 1 <= idx.size(1) <= MAX_K and idx.device == x.device == d2.device)
        if not ok:
            raise ValueError(f'tsne: neighbors has to be (idx int64 [{M}, k], dist2 float32 [{M}, k]) on the device of x, '
                             f'1 <= k <= {MAX_K}')
    if not x.is_cuda:
        raise ValueError(f'tsne: x has to be on the GPU; {_SUPPORTED}')
    return M


def pca_start(x, samples='rows'):
    """float32 [M, 2]: scikit-learn's init='pca' -- the first two PCA scores divided by the population standard
    deviation of the first and multiplied by 1e-4 (exact PCA here, scikit-learn's start uses the randomised solver)."""
    scores = pca(x, 2, samples=samples).scores
    std = scores[:, 0].double().std(unbiased=False).float()
    return (scores / std * 1e-4).contiguous()


def tsne(x, n_components=2, *, perplexity=30.0, early_exaggeration=12.0, learning_rate='auto', max_iter=1000,
         n_iter_without_progress=300, min_grad_norm=1e-7, init='pca', samples='rows', neighbors=None):
    """scikit-learn's TSNE(n_components=2, method='barnes_hut', angle=0, init='pca') of X = x (samples='rows': embeddings
    [N, D], D <= 256) or of X = x^T, never formed (samples='columns': the reference's fit_transform(x.T), at most 2048
    columns).  n_neighbors = min(M - 1, int(3 perplexity + 1)); learning_rate='auto' is max(M / early_exaggeration / 4,
    50); 250 iterations at momentum 0.5 on the exaggerated P, then momentum 0.8; error and gradient norm every 50
    iterations and at the last, with both of scikit-learn's stopping rules.  init: 'pca' or a float32 [M, 2] tensor;
    neighbors=(idx, dist2) bypasses the neighbour search.  Returns a TSNEResult; nothing carries a gradient, nothing is
    random, and invalid arguments raise ValueError before any launch."""
    M = _check(x, n_components, perplexity, early_exaggeration, learning_rate, max_iter, n_iter_without_progress,
               min_grad_norm, init, samples, neighbors)
    x = x.detach()
    idx, d2 = neighbors if neighbors is not None else nearest(x, min(M - 1, int(3.0 * perplexity + 1)), samples)
    if bool(((idx < 0) | (idx >= M)).any()):
        raise ValueError('tsne: some samples have fewer neighbours than asked for (rows of x with NaN?) or ids out of range')
    cond, beta = affinities(d2, perplexity)
    indptr, indices, val = joint_probabilities(idx, cond)
    y0 = init if isinstance(init, torch.Tensor) else pca_start(x, samples)
    lr = max(M / early_exaggeration / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)

    state = Descent(y0, indptr, indices, val)
    error, it = descend(lambda want: state.step(float(early_exaggeration), 0.5, lr, want), 0, EXPLORATION_ITER,
                        EXPLORATION_ITER, min_grad_norm)
    state.reset()
    last, it = descend(lambda want: state.step(1.0, 0.8, lr, want), it + 1, max_iter, n_iter_without_progress, min_grad_norm)
    return TSNEResult(state.y[0], error if last is None else last, it, (indptr, indices, val), beta, lr)
