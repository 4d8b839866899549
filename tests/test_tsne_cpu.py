"""ampnet_amd.tsne without a GPU: the fp64 models of tests/tsne_reference.py against scikit-learn's recordings
(tests/golden/tsne/, written by tools/make_golden_tsne.py), the conditions on the inputs that tests/test_gpu_tsne.py
relies on, the host-side pieces (the joint probabilities, the schedule) and the argument checks.

What the fixture generator measured where scikit-learn is installed is recorded in the fixtures and held here:
the search model agrees with _binary_search_perplexity to 1.2e-16 and the gradient model with
_kl_divergence_bh(angle=0) (fp32 code) to 6e-9."""
import importlib
import os

import numpy as np
import pytest
import torch

import tsne_reference as tr

ts = importlib.import_module('ampnet_amd.tsne')
NAMES = [c[0] for c in tr.CASES]


@pytest.fixture(scope='module', params=NAMES)
def fx(request):
    f = tr.load(request.param)
    f['name'] = request.param
    x = f['x'].astype(np.float64)
    f['X'] = x if str(f['samples']) == 'rows' else x.T
    return f


def test_fixtures_are_small_and_whole():
    for name, shape, perplexity, samples, _, head in tr.CASES:
        path = os.path.join(tr.GOLDEN_DIR, name + '.npz')
        assert os.path.getsize(path) < 100_000
        f = tr.load(name)
        M = shape[0] if samples == 'rows' else shape[1]
        k = min(M - 1, int(3.0 * perplexity + 1))
        assert f['x'].shape == shape and f['x'].dtype == np.float32 and str(f['samples']) == samples
        assert f['nbr_idx'].shape == (M, k) and f['nbr_dist2'].shape == (head, k) == f['cond_p'].shape
        assert f['indptr'].shape == (M + 1,) and f['indices'].size == f['indptr'][-1] and f['val'].size == f['indptr'][head]
        assert f['kl_auto'].shape == (4,) == f['kl_lr10'].shape and f['emb_auto'].shape == (M, 2)
        for tag in ('wide', 'start'):
            assert np.unique(f['y_' + tag], axis=0).shape[0] == M        # no coincident embedding points


def test_neighbours_of_the_fixtures(fx):
    """The exact fp64 neighbours of the stored input are scikit-learn's (as sets: the inputs lie on a grid, and the
    two order exactly equal distances differently), the squared distances its float32 ones (scikit-learn squares a
    rounded square root: one float32 ulp), and the last neighbour is further from the first one left out than any fp32
    evaluation of the distance can bridge."""
    k, head = int(fx['k']), int(fx['head'])
    idx, d2 = tr.exact_neighbors(fx['X'], k)
    assert np.array_equal(np.sort(idx, 1), np.sort(fx['nbr_idx'].astype(np.int64), 1))
    assert float(fx['gap']) > 2 * float(fx['bound'])
    assert np.abs(d2[:head] / fx['nbr_dist2'].astype(np.float64) - 1).max() <= 2.0 ** -23


def test_search_model_against_the_recording(fx):
    assert float(fx['search_agreement']) <= 1.2e-16
    P, beta, margin = tr.search_model(fx['nbr_dist2'], float(fx['perplexity']))
    assert np.abs(P - fx['cond_p'].astype(np.float64)).max() <= 2.0 ** -24        # the recording is rounded to float32
    assert np.allclose(P.sum(1), 1.0, atol=1e-12) and (beta > 0).all()
    H = -(P * np.log(np.maximum(P, 1e-300))).sum(1)
    assert np.abs(H - np.log(float(fx['perplexity']))).max() <= 1e-5 + 1e-9
    assert margin >= float(fx['search_margin']) * (1 - 1e-6) >= 1e-10          # recorded over all rows, these are the first


def test_joint_model_against_the_recording(fx):
    """scikit-learn's recorded neighbour ids and conditional probabilities through the joint model and through the
    library's own symmetrisation (torch on the host here): indptr and indices equal the recording exactly, the values
    lie within 2^-22 relative of it (tsne_reference.joint_bound derives the figure).  Two fixtures record every row and
    are held whole.  The other two record the probabilities of their first rows only (a file stays under 100 kB): there
    the rows that are not recorded come from the search model, and the entries held to the recording are those whose
    row and column are both recorded rows -- the others depend on inputs scikit-learn's recording does not hold, and
    are held to the model alone.  The model's own agreement with scikit-learn in fp64 over ALL entries was measured by
    the generator and is held to the error of two sums of nnz positive terms."""
    cond, pinned = tr.recorded_cond(fx, fx['X'])
    M, head = fx['X'].shape[0], int(fx['head'])
    assert pinned.all() == (head == M) and pinned.sum() >= 500
    assert float(fx['joint_agreement']) <= (2 * fx['indices'].size + 4) * 2.0 ** -53
    indptr, indices, val = tr.joint_model(fx['nbr_idx'], cond)
    assert np.array_equal(indptr, fx['indptr']) and np.array_equal(indices, fx['indices'])
    n = fx['val'].size
    rec = fx['val'].astype(np.float64)
    v32 = val.astype(np.float32).astype(np.float64)
    assert (np.abs(v32[:n] - rec) <= tr.joint_bound(rec))[pinned[:n]].all()
    assert abs(val.sum() - 1) <= 1e-12
    ti, tj, tv = ts.joint_probabilities(torch.as_tensor(fx['nbr_idx'].astype(np.int64)), torch.as_tensor(cond))
    assert np.array_equal(ti.numpy(), fx['indptr']) and np.array_equal(tj.numpy(), fx['indices'])
    assert (np.abs(tv.numpy()[:n] - rec) <= tr.joint_bound(rec))[pinned[:n]].all()
    assert (np.abs(tv.numpy() - val) <= 2.0 ** -22 * val + 2.0 ** -149).all()
    sym = {(i, j): v for i in range(len(indptr) - 1) for j, v in zip(indices[indptr[i]:indptr[i + 1]], val[indptr[i]:indptr[i + 1]])}
    assert all(sym[(j, i)] == v for (i, j), v in sym.items())


def full_val(fx):
    """The float32 values of P for all rows: scikit-learn's where the fixture records every row, else the joint model
    on scikit-learn's probabilities for the recorded rows and the search model's for the rest."""
    if int(fx['head']) == fx['X'].shape[0]:
        return fx['val']
    return tr.joint_model(fx['nbr_idx'], tr.recorded_cond(fx, fx['X'])[0])[2].astype(np.float32)


def test_gradient_model_against_the_recording(fx):
    """On scikit-learn's own P (the two whole fixtures) the fp64 gradient model agrees with _kl_divergence_bh(angle=0),
    which is fp32 code, to 6e-9.  Where P is not recorded whole, the unrecorded rows' probabilities are the search
    model's on distances that differ from scikit-learn's by a float32 ulp: tsne_reference.search_sensitivity bounds
    what that does to P, and the gradient is linear in P up to the same relative change."""
    assert float(fx['gradient_agreement']) <= 6e-9
    indptr, indices = fx['indptr'].astype(np.int64), fx['indices'].astype(np.int64)
    val = full_val(fx)
    slack = 0.0
    if int(fx['head']) != fx['X'].shape[0]:
        _, d2 = tr.exact_neighbors(fx['X'], int(fx['k']))
        # (the largest bound of the entries that carry a row: those within two sd of its mean distance)
        E = tr.search_sensitivity(d2.astype(np.float32), float(fx['perplexity']), 2.0 ** -23 * d2.max())
        P = tr.search_model(d2.astype(np.float32), float(fx['perplexity']))[0]
        slack = float((E * P).sum(1).max())
    for tag in ('wide', 'start'):
        err, grad = tr.gradient_model(fx['y_' + tag], indptr, indices, val)
        rec = fx['grad_' + tag].astype(np.float64)
        pos = tr.attraction_model(fx['y_' + tag], indptr, indices, val, 1.0, 1.0)[1]
        assert (np.abs(grad - rec) <= 6e-9 + 4.0 * slack * pos).all()
        assert err == pytest.approx(float(fx['err_' + tag]), rel=1e-5 + slack)


def test_joint_probabilities_is_the_model():
    """ampnet_amd.tsne.joint_probabilities (a library sort, no kernel): on the fixtures and on a star whose hub row has
    N - 1 entries."""
    cases = [(tr.load(n)['nbr_idx'].astype(np.int64), None) for n in NAMES]
    N = 40
    star = np.zeros((N, 1), np.int64)
    star[0, 0] = 1
    cases.append((star, None))
    for idx, _ in cases:
        rng = np.random.default_rng(idx.size)
        cond = rng.uniform(0.1, 1.0, idx.shape)
        cond /= cond.sum(1, keepdims=True)
        indptr, indices, val = ts.joint_probabilities(torch.as_tensor(idx), torch.as_tensor(tr.cond_f32(cond)))
        mp, mi, mv = tr.joint_model(idx, tr.cond_f32(cond))
        assert indptr.dtype == torch.int64 == indices.dtype and val.dtype == torch.float32
        assert np.array_equal(indptr.numpy(), mp) and np.array_equal(indices.numpy(), mi)
        assert np.abs(val.numpy() / mv - 1).max() <= 2.0 ** -22
    assert indptr[1] - indptr[0] == N - 1                                # the hub


def test_conditions_the_gpu_affinity_sweep_relies_on():
    """At every step of every row the model's |H - log perplexity| stays at least 1e-10 away from the tolerance 1e-5:
    fp64 noise of the order of 1e-15 cannot flip a stop decision."""
    ns, ks = set(), set()
    for N, K in tr.AFFINITY_SWEEP:
        d, perplexity = tr.affinity_case(N, K)
        P, beta, margin = tr.search_model(d, perplexity)
        assert margin >= 1e-10, (N, K, margin)
        assert np.isfinite(P).all() and (d[0] == 0).all() and np.exp(-d[N - 1].astype(np.float64)).max() == 0.0
        ns.add(N)
        ks.add(K)
    assert ns == {2, 3, 63, 64, 65, 257} and ks == {1, 2, 31, 63, 64, 65, 91, 256}


def test_conditions_the_gpu_step_test_relies_on():
    """No element of the step inputs has its gain decision inside the bound's own band, for either exaggeration: the 1 %
    cap of the GPU test can never hide a wrong kernel.  The CSR has the row lengths the issue names."""
    c = tr.step_case(5)
    lens = np.diff(c['indptr'])
    assert {0, 1, 63, 64, 65, c['N'] - 1} <= set(lens.tolist()) and (lens > tr.PART).sum() == 2
    for exag, mom, lr in ((1.0, 0.8, 200.0), (12.0, 0.5, 200.0)):
        e = tr.step_expectation(c, exag, mom, lr)
        assert not e['band'].any()
        assert np.array_equal(e['gains'].astype(np.float32), tr.gains_fp32(c['update'], e['grad'].astype(np.float32), c['gains']))


def test_schedule_is_the_models():
    """ampnet_amd.tsne.descend against tests/tsne_reference.descend on scripted errors and norms: both stopping rules,
    the check every 50 iterations and at the last."""
    def script(errors, norms):
        def model(i, want):
            return errors(i), norms(i)

        calls = []

        def ours(want):
            calls.append(want)
            i = start + len(calls) - 1
            return (errors(i), norms(i)) if want else None
        return model, ours, calls

    for errors, norms, start, max_iter, patience, min_norm, last in (
            (lambda i: 1.0 / (i + 1), lambda i: 1.0, 0, 250, 250, 1e-7, 249),         # runs out
            (lambda i: 1.0 + i, lambda i: 1.0, 250, 1000, 100, 1e-7, 449),           # no progress since 299
            (lambda i: 1.0 / (i + 1), lambda i: 1e-9, 0, 250, 250, 1e-7, 49),        # small gradient at the first check
            (lambda i: 1.0, lambda i: 1.0, 250, 1000, 300, 1e-7, 649),
            (lambda i: 1.0, lambda i: 1.0, 1000, 1000, 300, 1e-7, 1000)):            # nothing left to run
        model, ours, calls = script(errors, norms)
        want_e, want_i = tr.descend(model, start, max_iter, patience, min_norm)
        got_e, got_i = ts.descend(ours, start, max_iter, patience, min_norm)
        assert got_i == want_i == last and (got_e == want_e or (got_e is None and want_e == np.inf))
        assert sum(calls) <= (max_iter - start) // 50 + 1                        # read-backs


def test_argument_checks():
    from ampnet_amd import TSNEResult, neighbor_preservation, tsne
    x = torch.randn(40, 8)
    for kwargs, match in ((dict(n_components=3), 'two output dimensions'), (dict(perplexity=40.0), 'less than'),
                          (dict(perplexity=0.0), 'positive'), (dict(samples='both'), 'samples'),
                          (dict(init='random'), 'init'), (dict(init=torch.zeros(40, 3)), 'init'),
                          (dict(init=torch.zeros(40, 2, dtype=torch.float64)), 'init'),
                          (dict(learning_rate=-1.0), 'learning_rate'), (dict(learning_rate='fast'), 'learning_rate'),
                          (dict(max_iter=100), 'max_iter'), (dict(n_iter_without_progress=-1), 'n_iter_without_progress'),
                          (dict(early_exaggeration=0.5), 'early_exaggeration'),
                          (dict(neighbors=(torch.zeros(40, 5), torch.zeros(40, 5))), 'neighbors'),
                          (dict(neighbors=(torch.zeros(39, 5, dtype=torch.int64), torch.zeros(39, 5))), 'neighbors'),
                          (dict(), 'on the GPU')):
        kw = dict(perplexity=5.0)
        kw.update(kwargs)
        nc = kw.pop('n_components', 2)
        with pytest.raises(ValueError, match=match):
            tsne(x, nc, **kw)
    for bad, match in ((torch.randn(40, 300), 'pca'), (torch.randn(40), '2-d'), (torch.randn(1, 8), 'at least 2'),
                       (torch.randn(40, 8).double(), 'float64'), (torch.randn(40, 8, requires_grad=True), 'requires grad'),
                       (torch.randn(40, 8).long(), 'int64')):
        with pytest.raises(ValueError, match=match):
            tsne(bad, perplexity=5.0 if bad.dim() == 2 and bad.size(0) > 6 else 0.5)
    with pytest.raises(ValueError, match='samples'):
        tsne(torch.randn(40, 1), perplexity=0.5, samples='columns')
    with pytest.raises(ValueError, match='neighbours'):
        tsne(torch.randn(400, 8), perplexity=100.0)
    with pytest.raises(ValueError, match='same number of rows'):
        neighbor_preservation(torch.randn(5, 2), torch.randn(6, 2), 2)
    with pytest.raises(ValueError, match='k ='):
        neighbor_preservation(torch.randn(5, 2), torch.randn(5, 2), 5)
    r = TSNEResult(torch.tensor([[0.0, 1.0], [2.0, 1.0], [4.0, 1.0]]), 0.1, 999, None, None, 50.0)
    z = r.standardized()
    assert torch.allclose(z[:, 0], torch.tensor([-1.0, 0.0, 1.0]) * (1.5 ** 0.5)) and (z[:, 1] == 0).all()


def test_binding_mirrors_the_header_constants():
    import re
    from ampnet_amd import _lib
    hdr = open(os.path.join(os.path.dirname(tr.GOLDEN_DIR), '..', '..', 'include', 'ampconv.h')).read()
    for name, v in (('MAX_K', _lib.TSNE_MAX_K), ('RUN', _lib.TSNE_RUN), ('TILE', _lib.TSNE_TILE), ('CHUNK', _lib.TSNE_CHUNK),
                    ('PART', _lib.TSNE_PART)):
        assert int(re.search(r'#define AMPCONV_TSNE_%s (\d+)' % name, hdr).group(1)) == v
    assert (tr.RUN, tr.TILE, tr.CHUNK, tr.PART) == (_lib.TSNE_RUN, _lib.TSNE_TILE, _lib.TSNE_CHUNK, _lib.TSNE_PART)
    assert _lib.TSNE_MAX_N == 1 << 24 and '#define AMPCONV_TSNE_MAX_N (1 << 24)' in hdr


def test_loop_model_reaches_scikit_learns_divergence():
    """The whole-loop model (fp64 state, exact PCA start by numpy's SVD) on the smallest fixture, scikit-learn's schedule:
    it runs all 1000 iterations and ends at most 1.10 x above scikit-learn's recorded kl_divergence_ -- the condition the
    GPU tests hold ampnet_amd.tsne to is one the reference model satisfies."""
    f = tr.load('tsne_rows_70x12')
    X = f['x'].astype(np.float64)
    Xc = X - X.mean(0)
    U, S, _ = np.linalg.svd(Xc, full_matrices=False)
    y0 = U[:, :2] * S[:2]
    y0 = y0 / y0[:, 0].std() * 1e-4
    fx = dict(f, X=X)
    indptr, indices, val = f['indptr'].astype(np.int64), f['indices'].astype(np.int64), full_val(fx)
    y, err, n_iter = tr.loop_model(y0, indptr, indices, val, learning_rate=max(70 / 12.0 / 4.0, 50.0))
    kl = tr.kl_model(y, indptr, indices, val)
    assert n_iter == 999 and np.isfinite(y).all()
    assert kl <= 1.10 * float(f['kl_auto'].max()) and err == pytest.approx(kl, rel=0.05)


def test_one_iteration_expands_differences():
    """Why tests/test_gpu_tsne.py holds ten iterations step by step instead of compounding a bound: at the PCA start of
    the smallest fixture, under the exaggerated P and learning_rate 50, a perturbation of y of relative size 1e-6 comes
    out of ONE model iteration 25 to 30 times larger (10 is asserted), so a bound compounded over ten iterations would admit anything."""
    f = tr.load('tsne_rows_70x12')
    X = f['x'].astype(np.float64)
    U, S, _ = np.linalg.svd(X - X.mean(0), full_matrices=False)
    y0 = U[:, :2] * S[:2]
    y0 = y0 / y0[:, 0].std() * 1e-4
    indptr, indices, val = f['indptr'].astype(np.int64), f['indices'].astype(np.int64), f['val']

    def iterate(y):
        _, grad = tr.gradient_model(y, indptr, indices, val, 12.0)
        return tr.step_model(y, np.zeros_like(y), np.ones_like(y), grad, 0.5, 50.0)[0]
    dy = np.random.default_rng(0).normal(0.0, 1e-10, y0.shape)
    factor = np.linalg.norm(iterate(y0 + dy) - iterate(y0)) / np.linalg.norm(dy)
    assert factor > 10.0, factor
