"""The fp64 model of ampnet_amd.pca (tests/pca_reference.py) against scikit-learn's recorded outputs
(tests/golden/pca/, tools/make_pca_golden.py), its sign and rank rules on constructed inputs, and the argument checks of
pca(), which raise before anything touches a GPU."""
import glob
import os

import numpy as np
import pytest
import torch

import pca_reference as pr
from conftest import GOLDEN_DIR, load_golden

FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'pca', 'pca_*.npz')))
FIELDS = ('scores', 'components', 'mean', 'singular_values', 'explained_variance', 'explained_variance_ratio',
          'all_explained_variance_ratio')


def test_there_are_three_fixtures():
    assert [os.path.basename(f) for f in FIXTURES] == ['pca_columns_12x40.npz', 'pca_rows_40x12.npz', 'pca_rows_64x64.npz']


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_model_matches_scikit_learn(path):
    g = load_golden(path)
    m = pr.pca_model(g['x'], int(g['k']), str(g['samples']))
    assert not m['deficient'].any()
    for name in FIELDS:
        err = float(np.abs(m[name] - g[name]).max())
        print(f'[pca] {os.path.basename(path)} {name}: max err {err:.3e}')
        assert m[name].shape == g[name].shape and err <= 1e-9, (name, err)


@pytest.mark.parametrize('path', FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_model_matches_the_installed_scikit_learn(path):
    """The same against whatever scikit-learn is installed, where one is (the fixtures were written with 1.7.2)."""
    dec = pytest.importorskip('sklearn.decomposition')
    g = load_golden(path)
    X = g['x'].astype(np.float64)
    X = X if str(g['samples']) == 'rows' else X.T
    fit = dec.PCA(n_components=int(g['k']), svd_solver='full')
    scores = fit.fit_transform(X)
    m = pr.pca_model(g['x'], int(g['k']), str(g['samples']))
    for got, name in ((scores, 'scores'), (fit.components_, 'components'), (fit.explained_variance_ratio_, 'explained_variance_ratio')):
        assert float(np.abs(m[name] - got).max()) <= 1e-9, name


def test_sign_rule_on_a_constructed_tie():
    """The component (-a, +a, small): both large entries tie in magnitude, the FIRST decides, so the component is
    flipped to (+a, -a, ...); a component whose first maximum is already positive stays."""
    a = np.sqrt(0.5)
    comp = np.array([[-a, a, 0.0], [a, -a, 0.0], [0.1, -0.2, 0.2]])
    scores = np.arange(12.0).reshape(4, 3)
    c, s = pr.sign_flip(comp, scores)
    np.testing.assert_array_equal(c, [[a, -a, 0.0], [a, -a, 0.0], [-0.1, 0.2, -0.2]])
    np.testing.assert_array_equal(s, scores * np.array([-1.0, 1.0, -1.0]))
    # through the model: samples on the line (t, -t) have the component +-(1, -1) / sqrt 2, a tie by construction
    t = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])
    m = pr.pca_model(np.stack([t, -t], axis=1), 1)
    if abs(m['components'][0, 0]) == abs(m['components'][0, 1]):
        assert m['components'][0, 0] > 0 > m['components'][0, 1]
    else:                                               # the SVD's rounding broke the tie: the larger entry decides
        assert m['components'][0, np.abs(m['components'][0]).argmax()] > 0


@pytest.mark.parametrize('samples', ['rows', 'columns'])
def test_rank_rule_on_an_exactly_rank_two_input(samples):
    rng = np.random.default_rng(5)
    X = rng.integers(-3, 4, (9, 2)).astype(np.float64) @ rng.integers(-3, 4, (2, 7)).astype(np.float64)
    X = X - X.mean(axis=0)                              # small integers over 9: rank 2 survives the centring
    x = X if samples == 'rows' else X.T
    m = pr.pca_model(x, 4, samples)
    assert m['deficient'].tolist() == [False, False, True, True]
    assert (m['singular_values'] >= 0).all() and m['singular_values'][2] <= 1e-12 * m['singular_values'][0]
    if samples == 'columns':
        assert (m['components'][2:] == 0).all() and (m['components'][:2] != 0).any()
    assert np.abs(m['scores'][:, 2:]).max() <= 1e-12 * np.abs(m['scores']).max()
    assert abs(m['explained_variance_ratio'][:2].sum() - 1) <= 1e-12


def test_gram_and_project_models_round_like_the_kernels():
    x = np.array([[1.0 + 2.0 ** -23, 3.0], [5.0, 7.0]], dtype=np.float32)
    A = pr.shifted(x, col_shift=np.array([2.0 ** -24, 0.0], dtype=np.float32))
    assert A[0, 0] == float(np.float32(np.float32(1.0 + 2.0 ** -23) - np.float32(2.0 ** -24)))     # rounded once, in fp32
    S, scale = pr.gram_model(x)
    np.testing.assert_array_equal(S, x.astype(np.float64).T @ x.astype(np.float64))
    np.testing.assert_array_equal(S, scale)
    out, bound = pr.project_model(x, np.eye(2), scale=np.array([2.0, -1.0]))
    np.testing.assert_array_equal(out, x.astype(np.float64) * [2.0, -1.0])
    np.testing.assert_array_equal(bound, x.astype(np.float64) * [2.0, 1.0])


BAD_CALLS = [
    ('not a tensor', lambda: ([[1.0, 2.0], [3.0, 4.0]], 1, 'rows')),
    ('1-d', lambda: (torch.zeros(4), 1, 'rows')),
    ('float64', lambda: (torch.zeros(4, 3, dtype=torch.float64), 1, 'rows')),
    ('integer', lambda: (torch.zeros(4, 3, dtype=torch.int64), 1, 'rows')),
    ('too wide', lambda: (torch.zeros(4, 2049), 1, 'rows')),
    ('no column', lambda: (torch.zeros(4, 0), 1, 'rows')),
    ('one sample, rows', lambda: (torch.zeros(1, 3), 1, 'rows')),
    ('one sample, columns', lambda: (torch.zeros(3, 1), 1, 'columns')),
    ('k = 0', lambda: (torch.zeros(4, 3), 0, 'rows')),
    ('k > features', lambda: (torch.zeros(4, 3), 4, 'rows')),
    ('k > samples', lambda: (torch.zeros(3, 5), 4, 'rows')),
    ('k > samples, columns', lambda: (torch.zeros(5, 3), 4, 'columns')),
    ('k > 128', lambda: (torch.zeros(200, 200), 129, 'rows')),
    ('k a float', lambda: (torch.zeros(4, 3), 2.0, 'rows')),
    ('k a bool', lambda: (torch.zeros(4, 3), True, 'rows')),
    ('samples', lambda: (torch.zeros(4, 3), 1, 'nodes')),
    ('requires grad', lambda: (torch.zeros(4, 3, requires_grad=True), 1, 'rows')),
    ('on the CPU', lambda: (torch.zeros(4, 3), 1, 'rows')),
]


@pytest.mark.parametrize('what,args', BAD_CALLS, ids=[b[0] for b in BAD_CALLS])
def test_pca_refuses_before_any_gpu_call(what, args, monkeypatch):
    from ampnet_amd import _lib, pca

    def no_library():
        raise AssertionError('the library was loaded for a call that has to be refused first')
    monkeypatch.setattr(_lib, 'load', no_library)
    x, k, samples = args()
    with pytest.raises(ValueError):
        pca(x, k, samples=samples)


def test_requires_grad_is_refused_with_a_clear_message():
    from ampnet_amd import pca
    with pytest.raises(ValueError, match='no autograd'):
        pca(torch.zeros(4, 3, requires_grad=True), 1)


def test_transform_is_for_rows_fits_only():
    from ampnet_amd import PCAResult
    z = torch.zeros(2, 3)
    res = PCAResult('columns', z, z, torch.zeros(3), z[0], z[0], z[0], z[0])
    with pytest.raises(ValueError, match="samples='rows'"):
        res.transform(torch.zeros(4, 3))
