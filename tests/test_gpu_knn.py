"""The fused nearest-neighbour search on the GPU (csrc/knn.hip) against the fp64 model of tests/knn_reference.py: through
ctypes on a strided view inside NaN margins with every output pre-filled, and through the three wrappers.

Every row of every case passes knn_reference.check_rows: (1) distinct candidates with exactly the trailing slots empty,
(2) scores those of the pairs, (3) the kernel's own (score, position) sequence strictly ordered, bitwise, (4) optimality
within 2 tol.  tol = conftest.ATOL * scale + conftest.RTOL * |want| with scale = 1 (cosine), max(1, max |score|) (dot: a
score is a sum of D products) and max(1, max(|a|^2 + |b|^2)) (l2: the expansion cancels at that magnitude) -- the
`scaled=True` of conftest.assert_close_scaled, with its reason here.  bf16 storage is held to the same bars: the products
of stored values are exact in fp32.  The share of the bar a case used is printed ([tol] lines, pytest -rP)."""
import glob
import os

import numpy as np
import pytest
import torch

import knn_reference as ref
from conftest import ATOL, RTOL, load_golden

pytestmark = pytest.mark.gpu

METRICS = ('dot', 'cosine', 'l2')
IDX_FILL, SCORE_FILL, OOB_FILL = 7777, 7.0, 7
E_BADARG, E_WORKSPACE = -1, -3                          # AMPCONV_E_BADARG, AMPCONV_E_WORKSPACE


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _tol(want, scale):
    return ATOL * scale + RTOL * np.abs(want)


def _view(x, dtype, dev):
    """(x as a strided view inside NaN margins on the device, the stored values in fp64).  D % 4 == 0: the view keeps
    the alignment of the one-load-per-chunk path; otherwise it starts 3 elements in, on an odd row stride."""
    N, D = x.shape
    left = 4 if D % 4 == 0 else 3
    ld = (left + D + 7) // 4 * 4 if D % 4 == 0 else left + D + 2 + (left + D) % 2
    buf = torch.full((N + 2, ld), float('nan'), dtype=dtype)
    t = torch.from_numpy(np.asarray(x, dtype=np.float32)).to(dtype)
    buf[1:N + 1, left:left + D] = t
    return buf.to(dev)[1:N + 1, left:left + D], t.double().numpy()


def _call(xv, k, metric, queries=None, keys=None, exclude_self=False, *, N=None, D=None, ldx=None, Q=None, S=None,
          null=(), ws_bytes=None, metric_code=None, dtype_code=None):
    """ampconv_knn through ctypes, every output pre-filled: (return code, idx, score, oob)."""
    from ampnet_amd import _lib
    lib = _lib.load()
    dev = xv.device
    n, d = xv.shape
    N = n if N is None else N
    D = d if D is None else D
    q = None if queries is None else torch.as_tensor(queries, dtype=torch.int64).to(dev)
    s = None if keys is None else torch.as_tensor(keys, dtype=torch.int64).to(dev)
    Q = (n if q is None else q.numel()) if Q is None else Q
    S = (n if s is None else s.numel()) if S is None else S
    rows = max(min(Q, 1 << 16), 0)
    kk = min(max(k, 1), 64)
    idx = torch.full((rows, kk), IDX_FILL, dtype=torch.int64, device=dev)
    score = torch.full((rows, kk), SCORE_FILL, dtype=torch.float32, device=dev)
    oob = torch.full((1,), OOB_FILL, dtype=torch.int32, device=dev)
    need = int(lib.ampconv_knn_workspace_bytes(rows, min(S, 1 << 20), n, min(max(d, 1), 256), kk))
    ws = torch.full((max(need, 256),), 0x5A, dtype=torch.uint8, device=dev)
    p = dict(X=xv.data_ptr(), idx=idx.data_ptr(), score=score.data_ptr(), oob=oob.data_ptr(), ws=ws.data_ptr(),
             query=_lib.ptr(q), key=_lib.ptr(s))
    for name in null:
        p[name] = None
    rc = lib.ampconv_knn(p['X'], N, D, xv.stride(0) if ldx is None else ldx, p['query'], Q, p['key'], S, k,
                         ref.METRICS[metric] if metric_code is None else metric_code, int(exclude_self), p['idx'],
                         p['score'], p['oob'], p['ws'], ws.numel() if ws_bytes is None else ws_bytes,
                         _lib.DTYPES[xv.dtype] if dtype_code is None else dtype_code,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, idx.cpu().numpy(), score.cpu().numpy(), int(oob)


def _check(dev, x, k, metric, queries=None, keys=None, exclude_self=False, dtype=torch.float32, tag=''):
    xv, x64 = _view(x, dtype, dev)
    rc, idx, score, oob = _call(xv, k, metric, queries, keys, exclude_self)
    assert rc == 0 and oob == 0, f'{tag}: rc {rc}, oob {oob}'
    used = ref.check_rows(idx, score, x64, k, queries, keys, metric, exclude_self, _tol, tag)
    print(f'[tol] {tag} {metric} {str(dtype)[6:]}: scores use {100 * used:.2f} % of the tolerance')
    return idx, score


_RNG = np.random.default_rng(20240)
_X = {D: _RNG.standard_normal((300, D)).astype(np.float32) for D in (1, 3, 4, 31, 32, 33, 100, 128, 256)}
_PERM = _RNG.permutation(300)


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('Q', (1, 15, 16, 17, 63, 64, 65))
def test_query_ladder(dev, Q, metric):
    _check(dev, _X[100], 10, metric, queries=_PERM[:Q], tag=f'Q{Q}')


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('S', (1, 9, 10, 31, 32, 33, 300))
def test_key_ladder(dev, S, metric):
    # k = 10: S = k - 1 leaves one empty slot, S = 1 nine
    _check(dev, _X[100], 10, metric, queries=_PERM[:33], keys=_PERM[::-1][:S].copy(), tag=f'S{S}')


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('D', sorted(_X))
def test_channel_ladder(dev, D, metric):
    _check(dev, _X[D], 10, metric, queries=_PERM[:33], tag=f'D{D}')
    if D % 8 == 0:
        _check(dev, _X[D], 10, metric, queries=_PERM[:33], dtype=torch.bfloat16, tag=f'D{D}')


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('k', (1, 2, 10, 11, 63, 64))
def test_k_ladder(dev, k, metric):
    _check(dev, _X[100], k, metric, queries=_PERM[:33], exclude_self=k == 11, tag=f'k{k}')


@pytest.mark.parametrize('metric', METRICS)
def test_split_merge(dev, metric):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((20000, 100)).astype(np.float32)
    _check(dev, x, 10, metric, queries=rng.integers(0, 20000, 17), tag='Q17 S20000')


@pytest.mark.parametrize('metric', METRICS)
def test_all_rows(dev, metric):
    x = np.random.default_rng(2).standard_normal((2000, 128)).astype(np.float32)
    _check(dev, x, 16, metric, exclude_self=True, tag='N2000 all rows')


@pytest.mark.parametrize('metric', METRICS)
def test_no_query_and_no_key(dev, metric):
    xv, _ = _view(_X[32], torch.float32, dev)
    rc, idx, score, oob = _call(xv, 5, metric, queries=np.zeros(0, dtype=np.int64))
    assert rc == 0 and oob == 0 and idx.shape == (0, 5)
    rc, idx, score, oob = _call(xv, 5, metric, queries=_PERM[:20], keys=np.zeros(0, dtype=np.int64))
    assert rc == 0 and oob == 0 and (idx == -1).all()
    assert (score == (np.inf if metric == 'l2' else -np.inf)).all()
    # a NULL list with a count of 0 (what an empty tensor hands over) is a list of nothing, not "every node"
    rc, idx, score, oob = _call(xv, 5, metric, queries=_PERM[:20], null=('key',), S=0)
    assert rc == 0 and oob == 0 and (idx == -1).all()
    assert (score == (np.inf if metric == 'l2' else -np.inf)).all()
    rc, idx, score, oob = _call(xv, 5, metric, null=('query',), Q=0)
    assert rc == 0 and oob == 0 and idx.shape == (0, 5)
    rc, idx, score, oob = _call(xv, 5, metric, null=('query', 'oob'), Q=0)       # Q == 0: oob may be left out
    assert rc == 0 and oob == OOB_FILL


# ---- exact indices: idx equal to the model's, element for element
def _integer_rows(N, D, seed):
    """Values in -3..3: every product and sum is exact in fp32.  The last third of the rows repeats the first third."""
    x = np.random.default_rng(seed).integers(-3, 4, (N, D)).astype(np.float32)
    x[N - N // 3:] = x[:N // 3]
    return x


@pytest.mark.parametrize('metric', ('dot', 'l2'))
@pytest.mark.parametrize('dtype', (torch.float32, torch.bfloat16), ids=('f32', 'bf16'))
def test_exact_ties_by_position(dev, metric, dtype):
    x = _integer_rows(300, 24, 3)
    rng = np.random.default_rng(4)
    keys = rng.integers(0, 300, 500)                    # repeated ids: equal scores at different positions
    queries = rng.integers(0, 300, 70)
    xv, x64 = _view(x, dtype, dev)
    for k, ex in ((10, False), (64, True)):
        rc, idx, score, oob = _call(xv, k, metric, queries, keys, ex)
        want_idx, want_score, g, cand, _ = ref.knn(x64, k, queries, keys, metric, ex)
        assert rc == 0 and oob == 0
        assert (idx == want_idx).all()
        assert (score == want_score).all()              # exact arithmetic: the fp64 scores are the fp32 ones
        assert any(len(set(row)) < len(row) for row in want_score.tolist())       # ties did occur
    rc, idx, score, _ = _call(xv, 12, metric)           # all rows, no lists: ties between the duplicated rows
    assert rc == 0 and (idx == ref.knn(x64, 12, None, None, metric)[0]).all()


def test_exact_cosine_of_equal_norms(dev):
    base = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], dtype=np.float32)
    rng = np.random.default_rng(5)
    x = np.stack([rng.permutation(base) * rng.choice([-1.0, 1.0], 12) for _ in range(200)]).astype(np.float32)
    x[150:] = x[:50]                                    # equal rows: ties
    xv, x64 = _view(x, torch.float32, dev)
    keys = rng.integers(0, 200, 300)
    rc, idx, score, _ = _call(xv, 9, 'cosine', None, keys, True)
    # equal norms: the cosine ranking is the dot ranking, which is exact
    assert rc == 0 and (idx == ref.knn(x64, 9, None, keys, 'dot', True)[0]).all()
    ref.check_rows(idx, score, x64, 9, None, keys, 'cosine', True, _tol, 'cosine of equal norms')


@pytest.mark.parametrize('metric', METRICS)
def test_exclude_self_with_repeated_ids(dev, metric):
    x = _integer_rows(60, 8, 6) if metric != 'cosine' else _X[32][:60]
    queries = np.array([5, 5, 17, 59])
    keys = np.array([5, 17, 5, 3, 5, 59, 17, 5, 8, 9, 10, 11])
    xv, x64 = _view(x, torch.float32, dev)
    rc, idx, score, _ = _call(xv, 12, metric, queries, keys, True)
    assert rc == 0
    for q, node in enumerate(queries):
        assert node not in idx[q]
        assert (idx[q] == -1).sum() == (keys == node).sum()
    ref.check_rows(idx, score, x64, 12, queries, keys, metric, True, _tol, 'exclude_self')
    if metric != 'cosine':
        assert (idx == ref.knn(x64, 12, queries, keys, metric, True)[0]).all()


@pytest.mark.parametrize('metric', METRICS)
def test_nan_rows(dev, metric):
    x = _X[33].copy()
    x[40, 7] = np.nan
    x[41] = np.nan
    xv, x64 = _view(x, torch.float32, dev)
    rc, idx, score, _ = _call(xv, 64, metric, queries=np.array([40, 41, 3, 299]), keys=np.arange(30, 94))
    assert rc == 0
    assert (idx[:2] == -1).all()                        # a NaN row as a query: no candidate, an all-empty row
    assert not np.isin(idx, (40, 41)).any() and (idx[2:, :62] >= 0).all() and (idx[2:, 62:] == -1).all()
    assert not np.isnan(score).any()
    ref.check_rows(idx, score, x64, 64, np.array([40, 41, 3, 299]), np.arange(30, 94), metric, False, _tol, 'NaN rows')


@pytest.mark.parametrize('metric', METRICS)
def test_ids_out_of_range_are_clamped(dev, metric):
    xv, x64 = _view(_X[31], torch.float32, dev)
    queries = np.array([-5, 0, 299, 300, 2 ** 40, -2 ** 62, 7])
    keys = np.concatenate((np.arange(100, 160), [-1, 300, 2 ** 33, -2 ** 50, 5]))
    rc, idx, score, oob = _call(xv, 8, metric, queries, keys)
    assert rc == 0 and oob != 0 and oob != OOB_FILL
    rc2, idx2, score2, oob2 = _call(xv, 8, metric, np.clip(queries, 0, 299), np.clip(keys, 0, 299))
    assert rc2 == 0 and oob2 == 0
    assert (idx == idx2).all() and (score.view(np.uint32) == score2.view(np.uint32)).all()
    assert ((idx >= 0) & (idx < 300)).all()
    ref.check_rows(idx, score, x64, 8, queries, keys, metric, False, _tol, 'clamped ids')


@pytest.mark.parametrize('metric', METRICS)
def test_geometry_independence(dev, metric):
    x = np.random.default_rng(8).standard_normal((1500, 100)).astype(np.float32)
    xv, _ = _view(x, torch.float32, dev)
    rc, idx, score, _ = _call(xv, 10, metric, exclude_self=True)                   # all rows: 22 splits of the 47 key tiles
    rc1, idx1, score1, _ = _call(xv, 10, metric, exclude_self=True)
    assert rc == 0 and rc1 == 0
    assert (idx == idx1).all() and (score.view(np.uint32) == score1.view(np.uint32)).all()
    # one query: 47 splits; ...; 32 800 queries: one split, every list decoded by the tile kernel itself
    for sub in (np.array([1499]), np.array([77, 3, 1000, 3]), np.arange(0, 1500, 7), np.arange(32800) % 1500):
        rc2, idx2, score2, _ = _call(xv, 10, metric, queries=sub, exclude_self=True)
        assert rc2 == 0
        assert (idx2 == idx[sub]).all() and (score2.view(np.uint32) == score[sub].view(np.uint32)).all()


def test_refusals(dev):
    xv, _ = _view(_X[32], torch.float32, dev)
    q, s = np.arange(10), np.arange(50)
    cases = {
        'D = 0': dict(D=0), 'D = 257': dict(D=257), 'k = 0': dict(k=0), 'k = 65': dict(k=65),
        'ldx < D': dict(ldx=31), 'NULL X': dict(null=('X',)), 'NULL idx': dict(null=('idx',)),
        'NULL score': dict(null=('score',)), 'NULL oob': dict(null=('oob',)),
        'NULL queries, Q != N': dict(null=('query',)), 'NULL keys, S != N': dict(null=('key',)),
        'metric 3': dict(metric_code=3), 'metric -1': dict(metric_code=-1), 'dtype 2': dict(dtype_code=2),
        'Q = 2^31': dict(Q=2 ** 31), 'S = 2^31': dict(S=2 ** 31), 'N = 2^31': dict(N=2 ** 31), 'Q < 0': dict(Q=-1),
        'N = 0': dict(N=0), 'short workspace': dict(ws_bytes=255), 'NULL workspace': dict(null=('ws',)),
    }
    for name, opts in cases.items():
        k = opts.pop('k', 5)
        rc, idx, score, oob = _call(xv, k, 'l2', q, s, **opts)
        assert rc == (E_WORKSPACE if 'workspace' in name else E_BADARG), f'{name}: rc {rc}'
        assert (idx == IDX_FILL).all() and (score == SCORE_FILL).all() and oob == OOB_FILL, f'{name}: something was written'


# ---- the wrappers
def _fixtures():
    return sorted(glob.glob(os.path.join(ref.KNN_GOLDEN, 'knn_xor_*.npz')))


@pytest.mark.parametrize('path', _fixtures(), ids=os.path.basename)
def test_knn_graph_on_the_reference_fixtures(dev, path):
    from ampnet_amd import knn_graph
    f = load_golden(path)
    x, k, n = f['x'], int(f['k']), f['x'].shape[0]
    ei = knn_graph(torch.from_numpy(x).to(dev), k)
    assert ei.dtype == torch.int64 and ei.device.type == 'cuda'
    ei = ei.cpu().numpy()
    assert ei.shape == f['edge_index'].shape == (2, n * (k + 1))
    assert (ei[0] == f['edge_index'][0]).all()                                   # the reference's shape and order
    nbr = ei[1].reshape(n, k + 1)
    assert (np.diff(nbr, axis=1) > 0).all() and (nbr >= 0).all() and (nbr < n).all()
    if int(f['exact']):
        assert (ei == f['edge_index']).all()
    # every row's neighbour set is optimal within 2 tol (the one check knn_xor_400 is held to: its smallest gap is
    # below the error bound of the expansion)
    x64 = x.astype(np.float64)
    g = ref.goodness(x64, np.arange(n), np.arange(n), 'l2')
    sq = (x64 * x64).sum(1)
    scale = max(1.0, float((sq[:, None] + sq[None, :]).max()))
    for q in range(n):
        member = np.zeros(n, dtype=bool)
        member[nbr[q]] = True
        kth = np.sort(g[q])[::-1][k]
        assert (g[q, member] >= kth - 2 * _tol(kth, scale)).all(), f'row {q}'
        assert (g[q, ~member] <= g[q, member].min() + 2 * _tol(g[q, ~member], scale)).all(), f'row {q}'


def test_knn_graph_without_loops(dev):
    from ampnet_amd import knn_graph
    x = _integer_rows(90, 6, 9)                         # exact arithmetic: the model's graph, element for element
    for metric in ('l2', 'dot'):
        ei = knn_graph(torch.from_numpy(x).to(dev), 7, metric=metric, loop=False).cpu().numpy()
        assert ei.shape == (2, 630) and (ei[0] != ei[1]).all()
        assert (ei == ref.knn_graph(x, 7, metric=metric, loop=False)).all()
    ei = knn_graph(torch.from_numpy(x[:40]).to(dev), 39, loop=False).cpu().numpy()     # k == N - 1: everyone else
    assert (ei == ref.knn_graph(x[:40], 39, loop=False)).all()


def test_knn_public_function(dev):
    from ampnet_amd import knn
    x = torch.from_numpy(_X[100]).to(dev)
    wide = torch.zeros(300, 260, device=dev)
    wide[:, 5:105] = x
    queries = torch.from_numpy(_PERM[:40]).to(dev)
    idx, score = knn(x.requires_grad_(True), 6, queries=queries, metric='cosine', exclude_self=True)
    assert idx.dtype == torch.int64 and score.dtype == torch.float32 and idx.shape == score.shape == (40, 6)
    assert not idx.requires_grad and not score.requires_grad
    ref.check_rows(idx.cpu().numpy(), score.cpu().numpy(), _X[100].astype(np.float64), 6, _PERM[:40], None, 'cosine', True,
                   _tol, 'public')
    idx2, score2 = knn(wide[:, 5:105], 6, queries=queries, metric='cosine', exclude_self=True)      # a strided view, in place
    assert torch.equal(idx, idx2) and torch.equal(score, score2)
    bad = queries.clone()
    bad[3] = 300
    knn(x, 6, queries=bad)                              # clamped silently ...
    with pytest.raises(ValueError, match='outside'):
        knn(x, 6, queries=bad, check_indices=True)      # ... or reported
    idx, score = knn(x, 3, queries=queries[:0])
    assert idx.shape == (0, 3) and score.shape == (0, 3)
    idx, score = knn(x, 3, queries=queries[:4], keys=queries[:0])
    assert (idx == -1).all() and (score == -np.inf).all()


def test_knn_refuses_id_lists_it_cannot_read(dev):
    """The kernel reads count int64 values from a list's address: an int32 list would be read past its end, a list on
    another device is no device address of this one.  Neither reaches the library."""
    from ampnet_amd import knn
    x = torch.from_numpy(_X[32]).to(dev)
    for name in ('queries', 'keys'):
        for bad, what in ((torch.zeros(40, dtype=torch.int32, device=dev), r'torch.int32 \(40,\)'),
                          (torch.zeros(40, dtype=torch.float64, device=dev), r'torch.float64 \(40,\)'),
                          (torch.zeros(40, 1, dtype=torch.int64, device=dev), r'torch.int64 \(40, 1\)')):
            with pytest.raises(ValueError, match=f'{name} has to be a 1-d int64 tensor or None, got {what}'):
                knn(x, 3, **{name: bad})
        with pytest.raises(ValueError, match=f'{name} is on cpu, it has to be on the device of x'):
            knn(x, 3, **{name: torch.zeros(40, dtype=torch.int64)})
        if torch.cuda.device_count() > 1:
            with pytest.raises(ValueError, match=f'{name} is on cuda:1, it has to be on the device of x'):
                knn(x, 3, **{name: torch.zeros(40, dtype=torch.int64, device='cuda:1')})


def test_knn_graph_with_nan_rows(dev):
    from ampnet_amd import knn_graph
    x = torch.from_numpy(_X[4][:50].copy()).to(dev)
    assert int(knn_graph(x, 5, check_finite=True).min()) == 0
    x[7, 2] = float('nan')
    ei = knn_graph(x, 5).cpu().numpy()                  # documented: the missing neighbours are -1, in front of their row
    nbr = ei[1].reshape(50, 6)
    assert (nbr[7] == -1).all() and 7 not in nbr and (np.delete(nbr, 7, axis=0) >= 0).all()
    with pytest.raises(ValueError, match='fewer neighbours than asked for'):
        knn_graph(x, 5, check_finite=True)


def test_knn_classify(dev):
    from ampnet_amd import knn_classify
    rng = np.random.default_rng(10)
    z = rng.standard_normal((200, 16)).astype(np.float32)
    y = rng.integers(0, 7, 200)
    zt, yt = torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)
    for k in (1, 2, 5, 8):                              # even k: vote ties, decided for the smaller class
        got = knn_classify(zt, yt, k).cpu().numpy()
        assert got.dtype == np.int64 and (got == ref.knn_classify(z, y, k)).all()
    ties = sum(1 for row in ref.knn(z, 2, None, None, 'cosine', True)[0] if y[row[0]] != y[row[1]])
    assert ties > 0
    # k larger than the key count: empty slots do not vote; a query whose only key is itself gets -1
    keys = np.array([3, 50, 120])
    queries = np.array([3, 0, 199, 50])
    got = knn_classify(zt, yt, 6, queries=torch.from_numpy(queries).to(dev), keys=torch.from_numpy(keys).to(dev),
                       num_classes=7).cpu().numpy()
    assert (got == ref.knn_classify(z, y, 6, queries, keys, num_classes=7)).all()
    got = knn_classify(zt, yt, 4, queries=torch.tensor([3], device=dev), keys=torch.tensor([3, 3], device=dev)).cpu().numpy()
    assert list(got) == [-1]
    got = knn_classify(zt, yt, 5, metric='l2', exclude_self=False).cpu().numpy()
    assert (got == ref.knn_classify(z, y, 5, metric='l2', exclude_self=False)).all()
