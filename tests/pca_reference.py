"""fp64 numpy models of ampnet_amd.pca (include/ampconv.h, "principal components").

pca_model is the specification -- sklearn.decomposition.PCA(n_components=k, svd_solver='full') with scikit-learn >= 1.5's
sign rule -- written from the definition: centring in fp64, numpy.linalg.svd, nothing of the kernels' route through the
W x W matrix.  gram_model, shift_model and project_model mirror the roundings of one C call each."""
import numpy as np

U24 = 2.0 ** -24


def sign_flip(components, scores):
    """Every component (row) gets its largest-magnitude entry positive, the first such entry on a tie; the scores'
    columns flip with it.  numpy.argmax returns the first maximum."""
    at = np.abs(components).argmax(axis=1)
    sign = np.where(components[np.arange(components.shape[0]), at] < 0, -1.0, 1.0)
    return components * sign[:, None], scores * sign[None, :]


def pca_model(x, k, samples='rows'):
    """dict of scores [M, k], components [k, P], mean [P], singular_values, explained_variance, explained_variance_ratio
    [k], all_explained_variance_ratio [min(M, P)] and deficient [k] (bool: S_j <= S_1 max(M, P) 2^-23), all fp64, of
    X = x (samples='rows') or x^T ('columns').  The rank rule: the vectors that the kernels recover by a division by S_j
    -- the components of samples='columns' -- are zeros in a deficient direction."""
    X = np.asarray(x, dtype=np.float64)
    if samples == 'columns':
        X = X.T
    M, P = X.shape
    mean = X.mean(axis=0)
    U, S, Vt = np.linalg.svd(X - mean, full_matrices=False)
    components, scores = sign_flip(Vt[:k], U[:, :k] * S[:k])
    deficient = S[:k] <= S[0] * max(M, P) * 2.0 ** -23
    if samples == 'columns':
        components = np.where(deficient[:, None], 0.0, components)
    total = float((S * S).sum())
    ratio = S * S / total if total > 0 else np.zeros_like(S)
    return dict(scores=scores, components=components, mean=mean, singular_values=S[:k],
                explained_variance=S[:k] ** 2 / (M - 1), explained_variance_ratio=ratio[:k],
                all_explained_variance_ratio=ratio, deficient=deficient)


def shifted(x, row_shift=None, col_shift=None):
    """A as the kernels form it: fp32(x) - shift in fp32 (row shift first), returned as fp64."""
    A = np.asarray(x, dtype=np.float32)
    if row_shift is not None:
        A = (A - np.asarray(row_shift, dtype=np.float32)[:, None]).astype(np.float32)
    if col_shift is not None:
        A = (A - np.asarray(col_shift, dtype=np.float32)[None, :]).astype(np.float32)
    return A.astype(np.float64)


def gram_model(x, row_shift=None, col_shift=None):
    """(A^T A in fp64, |A|^T |A|): the second is the scale of ampconv_pca_gram's bound (kPcaRun + 2) 2^-24 |A|^T |A|."""
    A = shifted(x, row_shift, col_shift)
    return A.T @ A, np.abs(A).T @ np.abs(A)


def shift_model(x, axis):
    """ampconv_pca_shift: the fp64 mean, rounded to fp32 once."""
    return np.float32(np.asarray(x).astype(np.float64).mean(axis))


def project_model(x, V, row_shift=None, col_shift=None, scale=None):
    """(scale * (A @ V) in fp64, |scale| * (|A| |V|)): the second is the scale of ampconv_pca_project's bound."""
    A, V = shifted(x, row_shift, col_shift), np.asarray(V, dtype=np.float64)
    sc = np.ones(V.shape[1]) if scale is None else np.asarray(scale, dtype=np.float64)
    return (A @ V) * sc[None, :], (np.abs(A) @ np.abs(V)) * np.abs(sc)[None, :]


def prescribed(M, P, seed, decay=0.7, noise=1e-4):
    """float32 [M, P] with a prescribed spectrum: orthonormal factors from seeded QRs, singular values decay^j, noise at
    noise * s_1 -- the gaps keep the eigenvectors well conditioned."""
    rng = np.random.default_rng(seed)
    r = min(M, P)
    Q1, _ = np.linalg.qr(rng.standard_normal((M, r)))
    Q2, _ = np.linalg.qr(rng.standard_normal((P, r)))
    s = decay ** np.arange(r)
    X = (Q1 * s) @ Q2.T + noise * s[0] * rng.standard_normal((M, P)) + rng.standard_normal(P)[None, :]
    return X.astype(np.float32)


def fp32_composite_error(x, k, samples):
    """The yardstick of the end-to-end tolerance: the largest error against pca_model of a PLAIN fp32 composite -- fp32
    centring, torch.linalg.svd in fp32, the same sign rule -- over scores, components, singular values and both
    variance vectors.  Runs on the CPU; it is not the code under test."""
    import torch
    X = torch.as_tensor(np.asarray(x, dtype=np.float32))
    if samples == 'columns':
        X = X.t()
    M = X.shape[0]
    Xc = X - X.mean(dim=0, keepdim=True)
    U, S, Vt = torch.linalg.svd(Xc, full_matrices=False)
    comp, scores = sign_flip(Vt[:k].numpy().astype(np.float64), (U[:, :k] * S[:k]).numpy().astype(np.float64))
    S = S.numpy().astype(np.float64)
    total = float((S * S).sum())
    got = dict(scores=scores, components=comp, singular_values=S[:k], explained_variance=S[:k] ** 2 / (M - 1),
               explained_variance_ratio=S[:k] ** 2 / total)
    ref = pca_model(x, k, samples)
    return max(float(np.abs(got[n] - ref[n]).max()) for n in got)
