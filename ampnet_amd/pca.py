"""PCA of node features and embeddings (csrc/pca.hip): the reference's sklearn.decomposition.PCA -- its PCA featuriser
(src/ampnet/module/amp_gcn.py:185-237, `pca.fit_transform(x.numpy().transpose())`), the cumulative explained-variance
curve and the 2-D component plot (visualization/plot_PCA_2D_plot.py).

`pca(x, k, samples=...)` computes what `PCA(n_components=k, svd_solver='full')` computes.  The reference leaves
svd_solver at 'auto', which picks the RANDOMISED solver at Cora's shape; the exact solver is the specification here.

Whatever `samples` is, the work on the rows of x is one W x W matrix Sm = A^T A in fp64 (ampconv_pca_gram: exact-fp32
MFMA products, fp32 sums over runs of 32 rows, fp64 above that, no centred copy and no transpose) and one projection
(ampconv_pca_project); the means come from ampconv_pca_shift.  The eigen-decomposition of Sm is the one library call,
torch.linalg.eigh on float64: on the device where this torch build has a solver for it, else on the host (W x W only).
The contract is include/ampconv.h, "principal components".  There is no autograd and no eager fallback.
"""
import torch

from . import _lib
from .graph import _stream
from .head import _rows

MAX_W, MAX_K = _lib.PCA_MAX_W, _lib.PCA_MAX_K
SAMPLES = ('rows', 'columns')
_SUPPORTED = (f'supported: x [R, W] float32 or bfloat16 on the GPU with W <= {MAX_W}, at least 2 samples, '
              f'1 <= n_components <= min(samples, features, {MAX_K}) (ampnet_amd has no CPU fallback)')

EIGH_DEVICE = None        # None: not tried yet; True / False: torch.linalg.eigh(float64) runs on the device / the host


def _check_matrix(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f'{what}: x has to be a 2-d tensor, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}; {_SUPPORTED}')
    if x.dtype not in _lib.DTYPES:
        raise ValueError(f'{what}: x is {x.dtype}; {_SUPPORTED}')
    if x.requires_grad:
        raise ValueError(f'{what}: x requires grad, and PCA has no autograd: its inputs are data (pass x.detach())')
    if not 1 <= x.size(1) <= MAX_W or x.size(0) < 1:
        raise ValueError(f'{what}: x has shape {tuple(x.shape)}; {_SUPPORTED}')


def column_or_row_mean(x, axis):
    """float32 mean of every column (axis 0, [W]) or row (axis 1, [R]) of x, summed in fp64 in a fixed order."""
    lib = _lib.load()
    x, ldx = _rows(x)
    R, W = x.shape
    out = torch.empty(W if axis == 0 else R, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(int(lib.ampconv_pca_shift_workspace_bytes(R, W, axis)), 256), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ampconv_pca_shift(x.data_ptr(), R, W, ldx, axis, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _lib.DTYPES[x.dtype], _stream()), 'ampconv_pca_shift')
    return out


def gram(x, row_shift=None, col_shift=None):
    """float64 [W, W]: A^T A with A = x - row_shift[:, None] - col_shift[None, :] (either may be None)."""
    lib = _lib.load()
    x, ldx = _rows(x)
    R, W = x.shape
    Sm = torch.empty(W, W, dtype=torch.float64, device=x.device)
    ws = torch.empty(max(int(lib.ampconv_pca_gram_workspace_bytes(R, W)), 256), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ampconv_pca_gram(x.data_ptr(), R, W, ldx, _lib.ptr(row_shift), _lib.ptr(col_shift), Sm.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.DTYPES[x.dtype], _stream()), 'ampconv_pca_gram')
    return Sm


def project(x, V, row_shift=None, col_shift=None, scale=None):
    """float32 [R, k]: scale * ((x - row_shift[:, None] - col_shift[None, :]) @ V), V [W, k] float32."""
    lib = _lib.load()
    x, ldx = _rows(x)
    R, W = x.shape
    V = V.contiguous()
    k = V.size(1)
    out = torch.empty(R, k, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ampconv_pca_project(x.data_ptr(), R, W, ldx, _lib.ptr(row_shift), _lib.ptr(col_shift), V.data_ptr(),
                                           k, _lib.ptr(scale), out.data_ptr(), k, _lib.DTYPES[x.dtype], _stream()),
                   'ampconv_pca_project')
    return out


def eigh_descending(Sm):
    """(eigenvalues clamped at 0, eigenvectors as columns) of the symmetric float64 Sm, largest first: torch.linalg.eigh
    on the device if this build has a float64 solver there, else on the host (remembered in EIGH_DEVICE)."""
    global EIGH_DEVICE
    lam = vec = None
    if EIGH_DEVICE is not False:
        try:
            lam, vec = torch.linalg.eigh(Sm)
            EIGH_DEVICE = True
        except RuntimeError:
            if EIGH_DEVICE:               # it has worked before: this is not a missing solver
                raise
            EIGH_DEVICE = False
    if lam is None:
        lam, vec = torch.linalg.eigh(Sm.cpu())
        lam, vec = lam.to(Sm.device), vec.to(Sm.device)
    return lam.flip(0).clamp_(min=0), vec.flip(1)


def _positive_largest(components):
    """+1 / -1 per row of `components`: what makes the row's largest-magnitude entry (the first on a tie) positive."""
    at = components.abs().argmax(dim=1, keepdim=True)
    return torch.where(components.gather(1, at) < 0, -1.0, 1.0).to(components.dtype)


class PCAResult:
    """scores [M, k], components [k, P], mean [P] (float32); singular_values, explained_variance,
    explained_variance_ratio [k] and all_explained_variance_ratio [min(M, P)] (float64, from the fp64 spectrum)."""

    def __init__(self, samples, scores, components, mean, singular_values, explained_variance, explained_variance_ratio,
                 all_explained_variance_ratio):
        self.samples = samples
        self.scores, self.components, self.mean = scores, components, mean
        self.singular_values = singular_values
        self.explained_variance, self.explained_variance_ratio = explained_variance, explained_variance_ratio
        self.all_explained_variance_ratio = all_explained_variance_ratio
        self._V = components.t().contiguous() if samples == 'rows' else None

    def transform(self, y):
        """float32 [R, k]: (y - mean) @ components^T for new rows y [R, P] (samples='rows' only), the fit's projection."""
        if self.samples != 'rows':
            raise ValueError("transform needs a fit with samples='rows': new samples of a samples='columns' fit are columns")
        _check_matrix(y, 'PCAResult.transform')
        if y.size(1) != self.mean.numel():
            raise ValueError(f'PCAResult.transform: y has {y.size(1)} columns, the fit has {self.mean.numel()}')
        if not y.is_cuda or y.device != self.mean.device:
            raise ValueError(f'PCAResult.transform: y has to be on {self.mean.device}; {_SUPPORTED}')
        return project(y, self._V, col_shift=self.mean)


def pca(x, n_components, samples='rows'):
    """sklearn.decomposition.PCA(n_components, svd_solver='full') of X = x (samples='rows': embeddings [N, D]) or of
    X = x^T, never formed (samples='columns': the reference's fit_transform(x.transpose()), the samples are the feature
    columns).  With X [M, P]: mean [P], Xc = X - mean = U S Vt, components = Vt[:k], scores = U[:, :k] S[:k],
    explained_variance = S^2 / (M - 1), explained_variance_ratio = S^2 / sum(S^2) (0 where that sum is 0).  Every
    component has its largest-magnitude entry positive (the first on a tie; scikit-learn >= 1.5).  The exact solver is
    the specification: the reference's default svd_solver='auto' takes the randomised one at Cora's shape.
    Where S_j <= S_1 max(M, P) 2^-23 a vector that needs a division by S_j (the components of samples='columns') is
    zeros; S_j itself is reported.  Returns a PCAResult; nothing carries a gradient."""
    _check_matrix(x, 'pca')
    if samples not in SAMPLES:
        raise ValueError(f'pca: samples must be one of {SAMPLES}, got {samples!r}')
    R, W = x.shape
    M, P = (R, W) if samples == 'rows' else (W, R)
    k = n_components
    if isinstance(k, bool) or not isinstance(k, int) or M < 2 or not 1 <= k <= min(M, P, MAX_K):
        raise ValueError(f'pca: n_components = {k!r} with {M} samples of {P} features; {_SUPPORTED}')
    if not x.is_cuda:
        raise ValueError(f'pca: x has to be on the GPU; {_SUPPORTED}')

    rows = samples == 'rows'
    mean = column_or_row_mean(x, 0 if rows else 1)
    Sm = gram(x, col_shift=mean) if rows else gram(x, row_shift=mean)
    lam, vec = eigh_descending(Sm)
    nv = min(M, P)
    total = lam[:nv].sum()
    ratio = torch.where(total > 0, lam[:nv] / total, torch.zeros_like(lam[:nv]))
    S = lam[:k].sqrt()
    if rows:
        comp = vec[:, :k].t().float()
        comp = (comp * _positive_largest(comp)).contiguous()
        scores = project(x, comp.t().contiguous(), col_shift=mean)
    else:
        keep = S > S[0] * (max(M, P) * 2.0 ** -23)
        scale = torch.where(keep, 1.0 / S.clamp(min=torch.finfo(torch.float64).tiny), torch.zeros_like(S)).float()
        U = vec[:, :k]
        comp = project(x, U.float().contiguous(), row_shift=mean, scale=scale).t().contiguous()
        sign = _positive_largest(comp)
        comp = comp * sign
        scores = ((U * S) * sign.t().double()).float()
    return PCAResult(samples, scores, comp, mean, S, lam[:k] / (M - 1), ratio[:k].clone(), ratio)
