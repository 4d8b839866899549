#!/usr/bin/env python3
"""tests/golden/pca/pca_*.npz: inputs with a prescribed spectrum and what scikit-learn's
PCA(n_components=k, svd_solver='full') returns for them, for tests/test_pca_cpu.py and tests/test_gpu_pca.py.

TEST INFRASTRUCTURE; runs on the CPU where scikit-learn is installed (written with 1.7.2; the sign rule of the
specification is that of >= 1.5 and is asserted here).  The inputs come from tests/pca_reference.prescribed: orthonormal
factors from seeded QRs, singular values 0.7^j, noise at 1e-4 s_1 and a constant per column, stored as float32;
scikit-learn gets them widened to float64 so that it works in fp64 (float32 input would make it work in fp32).
samples='columns' fixtures hold x as the library takes it ([features, samples]) and scikit-learn's fit of x^T.

The fixtures live in tests/golden/pca/: conftest.golden_files() takes every tests/golden/*.npz for an AMPConv layer.

    python tools/make_pca_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
OUT_DIR = os.path.join(ROOT, 'tests', 'golden', 'pca')

#         name               x shape  samples   k  seed
CASES = (('pca_rows_40x12', (40, 12), 'rows', 5, 11),
         ('pca_columns_12x40', (12, 40), 'columns', 5, 12),
         ('pca_rows_64x64', (64, 64), 'rows', 8, 13))


def main():
    import sklearn
    from sklearn.decomposition import PCA
    import pca_reference as pr
    os.makedirs(OUT_DIR, exist_ok=True)
    for name, shape, samples, k, seed in CASES:
        x = pr.prescribed(shape[0], shape[1], seed) if samples == 'rows' else pr.prescribed(shape[1], shape[0], seed).T.copy()
        assert x.dtype == np.float32 and x.shape == shape
        X = x.astype(np.float64) if samples == 'rows' else x.astype(np.float64).T
        fit = PCA(n_components=k, svd_solver='full')
        scores = fit.fit_transform(X)
        full = PCA(n_components=None, svd_solver='full').fit(X)
        comp = fit.components_
        at = np.abs(comp).argmax(axis=1)
        assert (comp[np.arange(k), at] > 0).all(), 'this scikit-learn does not flip signs by the components (needs >= 1.5)'
        np.savez(os.path.join(OUT_DIR, name + '.npz'), x=x, k=np.int64(k), samples=np.array(samples),
                 scores=scores, components=comp, mean=fit.mean_, singular_values=fit.singular_values_,
                 explained_variance=fit.explained_variance_, explained_variance_ratio=fit.explained_variance_ratio_,
                 all_explained_variance_ratio=full.explained_variance_ratio_, sklearn_version=np.array(sklearn.__version__))
        print(f'{name}: x {x.shape} {samples}, k {k}, S {fit.singular_values_[:3]} ..., sklearn {sklearn.__version__}')


if __name__ == '__main__':
    main()
