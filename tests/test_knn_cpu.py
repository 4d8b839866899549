"""The nearest-neighbour model of tests/knn_reference.py against a brute-force sort, the 64-bit key order against the rule of
include/ampconv.h ("nearest neighbours"), the reference's fixtures, and what ampnet_amd.knn refuses -- no GPU needed."""
import glob
import os

import numpy as np
import pytest
import torch

import knn_reference as ref
from conftest import ATOL, RTOL, load_golden


def _tol(want, scale):
    return ATOL * scale + RTOL * np.abs(want)


def _brute(x, k, qid, kid, metric, exclude_self):
    """Every query by a Python sort of (−g, position) tuples."""
    g = ref.goodness(x, qid, kid, metric)
    rows = []
    for q in range(len(qid)):
        c = [(-(g[q, s] + 0.0), s) for s in range(len(kid))
             if not np.isnan(g[q, s]) and not (exclude_self and kid[s] == qid[q])]
        rows.append([kid[s] for _, s in sorted(c)[:k]])
    return rows


@pytest.mark.parametrize('metric', sorted(ref.METRICS))
@pytest.mark.parametrize('exclude_self', (False, True))
def test_model_against_a_brute_force_sort(metric, exclude_self):
    rng = np.random.default_rng(0)
    x = rng.integers(-3, 4, (40, 5)).astype(np.float64)        # small integers: ties in every row
    x[7] = np.nan
    queries, keys = rng.integers(0, 40, 23), rng.integers(0, 40, 31)
    for k in (1, 4, 31, 40):
        idx, score, g, cand, pos = ref.knn(x, k, queries, keys, metric, exclude_self)
        want = _brute(x, k, queries, keys, metric, exclude_self)
        for q in range(23):
            n = len(want[q])
            assert list(idx[q, :n]) == want[q] and (idx[q, n:] == -1).all()
            assert (score[q, n:] == (np.inf if metric == 'l2' else -np.inf)).all()
            assert n == min(k, int(cand[q].sum()))
            if metric == 'l2':
                assert (np.diff(score[q, :n]) >= 0).all() and (score[q, :n] >= 0).all()
            else:
                assert (np.diff(score[q, :n]) <= 0).all()
    assert (ref.knn(x, 3, np.array([7]), keys, metric)[0] == -1).all()          # a NaN query: no candidate
    assert 7 not in ref.knn(x, 40, None, None, metric)[0]                       # a NaN key is never returned


def test_key_encoding_is_the_order_of_the_rule():
    tiny = np.float32(1e-45)                                    # the smallest denormal
    values = np.array([-np.inf, -3.4e38, -1.0, -1e-38, -tiny, 0.0, tiny, 1e-38, 1.0, 3.4e38, np.inf], dtype=np.float32)
    img = ref.float_image(values)
    assert (np.diff(img.astype(np.int64)) > 0).all()            # strictly increasing with the value
    assert img[0] == 0x007FFFFF and (img > 0).all()             # key 0 stays free for "no candidate"
    assert ref.float_image(np.float32(-0.0)) == ref.float_image(np.float32(0.0)) == 0x80000000       # -0 counts as +0
    # (g descending, s ascending) is one unsigned compare; equal g: the earlier position is the larger key
    g = np.array([1.0, 1.0, -0.0, 0.0, -2.0, np.inf, -np.inf], dtype=np.float32)
    s = np.array([5, 2, 9, 1, 0, 2 ** 31 - 2, 3], dtype=np.int64)
    keys = ref.encode_keys(g, s)
    by_key = list(np.argsort(keys)[::-1])
    by_rule = sorted(range(len(g)), key=lambda i: (-(float(g[i]) + 0.0), int(s[i])))
    assert by_key == by_rule == [5, 1, 0, 3, 2, 4, 6]
    assert len(set(keys.tolist())) == len(keys) and (keys > 0).all()
    # a NaN has no place in the order: the model never encodes one
    x = np.array([[1.0], [np.nan], [2.0]])
    for metric in ref.METRICS:
        idx, _, g64, cand, _ = ref.knn(x, 3, None, None, metric)
        assert not cand[1].any() and not cand[:, 1].any() and (idx[1] == -1).all() and 1 not in idx


def _fixtures():
    return sorted(glob.glob(os.path.join(ref.KNN_GOLDEN, 'knn_xor_*.npz')))


def test_fixtures_are_the_three_of_the_issue():
    assert [os.path.basename(f) for f in _fixtures()] == ['knn_xor_128.npz', 'knn_xor_400.npz', 'knn_xor_64.npz']


@pytest.mark.parametrize('path', _fixtures(), ids=os.path.basename)
def test_model_on_the_reference_fixtures(path):
    f = load_golden(path)
    x, k, n = f['x'], int(f['k']), f['x'].shape[0]
    assert x.dtype == np.float32 and f['edge_index'].shape == (2, n * (k + 1))
    ei = ref.knn_graph(x, k)
    assert ei.shape == f['edge_index'].shape and (ei[0] == f['edge_index'][0]).all()
    assert (np.diff(ei[1].reshape(n, k + 1), axis=1) > 0).all()                 # (row, neighbour) order
    if int(f['exact']):
        assert float(f['gap']) >= 4 * float(f['bound'])
        assert (ei == f['edge_index']).all()
    # the reference's own neighbour sets pass the all-rows optimality check (l2: no neighbour is ordered in the fixture,
    # so the check runs on the sets: every member within 2 tol of the model's (k + 1)-th, every non-member no better)
    g = ref.goodness(x, np.arange(n), np.arange(n), 'l2')
    sq = (x.astype(np.float64) ** 2).sum(1)
    scale = max(1.0, float((sq[:, None] + sq[None, :]).max()))
    nbr = f['edge_index'][1].reshape(n, k + 1)
    for q in range(n):
        member = np.zeros(n, dtype=bool)
        member[nbr[q]] = True
        kth = np.sort(g[q])[::-1][k]
        assert (g[q, member] >= kth - 2 * _tol(kth, scale)).all()
        assert (g[q, ~member] <= g[q, member].min() + 2 * _tol(g[q, ~member], scale)).all()


def test_wrappers_of_the_model():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((30, 4))
    ei = ref.knn_graph(x, 3, loop=False)
    assert ei.shape == (2, 90) and (ei[0] != ei[1]).all()
    y = np.array([2, 2, 5, 5, 0, 1] * 5)
    idx = np.array([[0, 2, -1], [2, 0, 1], [-1, -1, -1], [4, 5, 3]])
    assert list(ref.vote(idx, y, 7)) == [2, 2, -1, 0]          # tie 2 / 5 -> 2; majority; no neighbour; tie 0 / 1 / 5 -> 0


def test_value_errors():
    """Every pattern is text that only the intended check emits (none of it is in the `supported: ...` tail that several
    messages share)."""
    from ampnet_amd import knn, knn_classify, knn_graph
    x = torch.zeros(10, 4)
    with pytest.raises(ValueError, match='x has to be on the GPU'):
        knn(x, 3)                                               # a CPU tensor: no fallback
    for k in (0, 65, 2.0, True):
        with pytest.raises(ValueError, match='knn: k = '):
            knn(x, k)
    with pytest.raises(ValueError, match=r'x has shape \(10, 257\)'):
        knn(torch.zeros(10, 257), 3)
    with pytest.raises(ValueError, match=r'x has shape \(10,\)'):
        knn(torch.zeros(10), 3)
    with pytest.raises(ValueError, match='x is torch.float64'):
        knn(x.double(), 3)
    with pytest.raises(ValueError, match='metric must be one of'):
        knn(x, 3, metric='euclid')
    # a wrong id dtype or shape is refused before anything else about the device: the kernel would read int64 values
    # from the list's address
    for name in ('queries', 'keys'):
        for bad, what in ((torch.zeros(3, dtype=torch.int32), r'torch.int32 \(3,\)'),
                          (torch.zeros(3, dtype=torch.float32), r'torch.float32 \(3,\)'),
                          (torch.zeros(3, 1, dtype=torch.int64), r'torch.int64 \(3, 1\)'), ([1, 2], 'list')):
            with pytest.raises(ValueError, match=f'{name} has to be a 1-d int64 tensor or None, got {what}'):
                knn(x, 3, **{name: bad})
    with pytest.raises(ValueError, match='11 neighbours per node and 10 nodes'):
        knn_graph(x, 10)                                        # k + 1 > N
    with pytest.raises(ValueError, match='10 neighbours per node besides itself and 10 nodes'):
        knn_graph(x, 10, loop=False)                            # k > N - 1
    with pytest.raises(ValueError, match='x has to be on the GPU'):
        knn_graph(x, 9)                                         # k + 1 == N is a shape the kernel takes
    with pytest.raises(ValueError, match='y has to be a 1-d integer tensor'):
        knn_classify(x, torch.zeros(10), 1)
    with pytest.raises(ValueError, match='9 labels for 10 nodes'):
        knn_classify(x, torch.zeros(9, dtype=torch.int64), 1)


def test_workspace_bytes_are_monotone():
    from ampnet_amd import _lib
    f = _lib.load().ampconv_knn_workspace_bytes
    base = dict(Q=17, S=20000, N=20000, D=100, k=10)
    assert f(*base.values()) > 0
    ladders = dict(Q=(1, 15, 16, 17, 64, 511, 512, 513, 528, 529, 4096, 32767, 32768, 32769, 100000, 2 ** 31 - 1),
                   S=(0, 1, 31, 32, 33, 2047, 2048, 2049, 20000, 10 ** 6, 2 ** 31 - 1),
                   N=(1, 63, 64, 65, 20000, 10 ** 6, 2 ** 31 - 1), D=(1, 3, 4, 100, 128, 255, 256), k=(1, 2, 10, 63, 64))
    for name, values in ladders.items():
        got = [f(*{**base, name: v}.values()) for v in values]
        assert all(b >= a for a, b in zip(got, got[1:])), f'{name}: {got}'
        assert all(g > 0 and g % 256 == 0 for g in got), f'{name}: {got}'
    # every pair of the Q and S ladders, not only one line through them
    for k in (1, 64):
        grid = [[f(Q, S, 1000, 64, k) for S in ladders['S']] for Q in ladders['Q']]
        assert all(b >= a for row in grid for a, b in zip(row, row[1:]))
        assert all(b >= a for col in zip(*grid) for a, b in zip(col, col[1:]))
    assert f(0, 10, 10, 4, 1) == 0 and f(10, 10, 10, 0, 1) == 0 and f(10, 10, 10, 4, 65) == 0 and f(2 ** 31, 10, 10, 4, 1) == 0
