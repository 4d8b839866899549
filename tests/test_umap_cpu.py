"""The fp64 models of tests/umap_reference.py held to their invariants on the CPU, and the host side of ampnet_amd.umap
(the curve fit, the argument checks).  No umap source exists to record from: the header's statements are the
specification, and what can be checked without one is checked here -- the fit against scipy where it is installed, the
calibration's own stopping rule, the identity that lets the kernels gather instead of scatter, the integer-exact
schedule, and that the layout does what a UMAP is for (it keeps neighbours that a 2-d PCA loses)."""
import importlib

import numpy as np
import pytest
import torch

import umap_reference as ur

AB_CASES = ((1.0, 0.1), (1.0, 0.5), (2.0, 0.01))


# -------------------------------------------------------------------------------------------------------- the curve
def test_model_fit_matches_scipy():
    optimize = pytest.importorskip('scipy.optimize')
    for spread, min_dist in AB_CASES:
        x = np.linspace(0.0, 3.0 * spread, 300)
        y = np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))
        want, _ = optimize.curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2.0 * b)), x, y)
        got = ur.find_ab_params(spread, min_dist)
        assert np.allclose(got, want, rtol=1e-4, atol=0), (spread, min_dist, got, want)


def test_package_fit_matches_the_model_and_the_recorded_defaults():
    um = importlib.import_module('ampnet_amd.umap')
    for spread, min_dist in AB_CASES:
        assert np.allclose(um.find_ab_params(spread, min_dist), ur.find_ab_params(spread, min_dist), rtol=1e-6, atol=0)
    a, b = um.find_ab_params()
    assert a == pytest.approx(1.5769, abs=2e-4) and b == pytest.approx(0.8951, abs=2e-4)
    a, b = um.find_ab_params(1.0, 1.0)                            # min_dist = spread: still a fit
    assert np.isfinite([a, b]).all() and a > 0 and b > 0


# ------------------------------------------------------------------------------------------------------ calibration
def test_calibration_reaches_its_target_wherever_the_floor_does_not_bind():
    rng = np.random.default_rng(0)
    hit = 0
    for M, D, k in ((2, 3, 2), (65, 4, 15), (300, 8, 64), (300, 8, 256), (40, 2, 3)):
        X = rng.normal(0.0, 1.0, (M, D)) * rng.choice([0.01, 1.0, 50.0], (M, 1))      # rows at very different scales
        _, dist = ur.neighbors_with_self(X, k)
        sigma, rho, psum, floored = ur.smooth_knn(dist)
        free = ~floored
        hit += int(free.sum())
        assert (np.abs(psum - np.log2(k))[free] < 1e-5).all()
        assert (rho == dist[:, 1]).all() and (sigma > 0).all()
        # where the floor binds the search's sigma was SMALLER: the sum at the floored sigma is no smaller than at the search's
        x = dist[:, 1:].astype(np.float64) - rho[:, None]
        at = np.where(x > 0, np.exp(-x / sigma[:, None]), 1.0).sum(1)
        assert (at[floored] >= psum[floored] - 1e-12).all()
    assert hit > 300


def test_duplicate_points_have_rho_zero_and_the_global_floor():
    """A block of exact duplicates wider than k: all k distances of its rows are 0, so rho = 0 and every round sums k - 1
    ones, 7 against the target log2(8) = 3: the search halves mid 64 times and never stops, and the floor -- 1e-3 x the
    mean of ALL distances, since the row's own mean is 0 -- is what sigma becomes."""
    rng = np.random.default_rng(1)
    X = rng.normal(0.0, 1.0, (60, 3))
    X[:20] = X[0]
    k = 8
    idx, dist = ur.neighbors_with_self(X, k)
    assert (dist[:20] == 0).all()
    sigma, rho, psum, floored = ur.smooth_knn(dist)
    assert (rho[:20] == 0).all() and floored[:20].all()
    assert np.allclose(sigma[:20], 1e-3 * dist.astype(np.float64).mean(), rtol=1e-12)
    assert (rho[20:] > 0).all()
    memb, _, _ = ur.memberships_model(idx, dist)
    assert (memb[:20, 1:] == 1).all() and (memb[:, 0] == 0).all()


def test_memberships_and_fuzzy_union():
    rng = np.random.default_rng(2)
    X = rng.normal(0.0, 1.0, (50, 3))
    idx, dist = ur.neighbors_with_self(X, 6)
    memb, sigma, rho = ur.memberships_model(idx, dist)
    assert (memb[:, 0] == 0).all() and (memb[:, 1] == 1).all() and ((memb >= 0) & (memb <= 1)).all()
    assert (np.diff(memb[:, 1:], axis=1) <= 0).all()
    indptr, indices, val = ur.fuzzy_model(idx, memb.astype(np.float32))
    M = 50
    W = np.zeros((M, M), np.float32)
    rows = np.repeat(np.arange(M), np.diff(indptr))
    W[rows, indices] = val
    assert np.array_equal(W.view(np.int32), W.T.copy().view(np.int32)) and (np.diag(W) == 0).all() and (val != 0).all()
    assert all((np.diff(indices[indptr[i]:indptr[i + 1]]) > 0).all() for i in range(M))
    P = np.zeros((M, M))
    P[np.arange(M)[:, None], idx] = memb.astype(np.float32)
    assert np.allclose(W, P + P.T - P * P.T, rtol=3e-7, atol=0)
    one_sided = ((P > 0) != (P.T > 0)).sum()
    assert one_sided > 0 and ((P > 0) & (P.T > 0)).sum() > 0          # both kinds of pair are in this case


# ------------------------------------------------------------------------------------------------------------ epochs
def small_graph(M=40, k=6, dim=2, n_epochs=30, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 1.0, (M, 4))
    idx, dist = ur.neighbors_with_self(X, k)
    memb, _, _ = ur.memberships_model(idx, dist)
    g = ur.fuzzy_model(idx, memb.astype(np.float32))
    y0 = ur.scaled_start_model(rng.normal(0.0, 1.0, (M, dim)))
    return g, y0, ur.State(*ur.schedule_model(*g, n_epochs))


def test_scatter_with_frozen_positions_equals_the_gather():
    """The identity the kernels rest on: the mirrored entry has the same weight bits, so the same schedule, and with the
    positions frozen its move of its tail is the move the row computes itself.  Both forms, epoch after epoch, each
    from the gather's positions, on a graph with mutual and one-sided neighbours, two coincident points included."""
    a, b = ur.find_ab_params()
    for dim in (2, 3):
        g, y0, st = small_graph(dim=dim)
        Y = y0.astype(np.float64)
        Y[7] = Y[int(st.indices[st.indptr[7]])]                       # an edge of length 0
        rows = st.rows
        mirror = {(int(r), int(c)): e for e, (r, c) in enumerate(zip(rows, st.indices))}
        assert all((c, r) in mirror and st.eps[mirror[(c, r)]] == st.eps[e] for (r, c), e in mirror.items())
        moved = 0
        for n in range(30):
            s1, s2 = st.copy(), st.copy()
            Yg, info = ur.epoch_gather(Y, s1, n, 30, a, b, seed=5)
            Ys = ur.epoch_scatter(Y, s2, n, 30, a, b, seed=5)
            scale = np.abs(Y).max() + 8.0 * info['count'].max()
            assert np.abs(Yg - Ys).max() <= 64 * np.finfo(np.float64).eps * scale, n
            assert np.array_equal(s1.next, s2.next) and np.array_equal(s1.nextneg, s2.nextneg) and np.array_equal(s1.drawn, s2.drawn)
            moved += info['fired'].size
            Y, st = Yg, s1
        assert moved > 0 and np.isfinite(Y).all()


def test_schedule_counts_what_it_draws():
    """eps = max / w >= 1; the strongest entries fire in every epoch from 1 on, an entry with eps = 4 about every fourth,
    with about 5 negatives per firing; drawn counts what was drawn; the ids are draw(seed, e, counter) % M with
    consecutive counters per entry."""
    g, y0, st = small_graph(n_epochs=30)
    a, b = ur.find_ab_params()
    assert (st.eps >= 1).all() and (st.eps <= 30).all() and (st.eps == 1).any()
    Y = y0.astype(np.float64)
    total = np.zeros(st.eps.size, np.int64)
    fires = np.zeros(st.eps.size, np.int64)
    for n in range(30):
        before = st.drawn.copy()
        Y, info = ur.epoch_gather(Y, st, n, 30, a, b, seed=9)
        total[info['fired']] += info['m']
        fires[info['fired']] += 1
        for ee, p, s in info['ids']:
            want = ur.draw(9, ee, before[ee].astype(np.int64) + p) % np.uint64(40)
            assert np.array_equal(s, want.astype(np.int64))
    assert np.array_equal(total, st.drawn)
    top = st.eps == 1
    assert (fires[top] == 29).all()                                   # next = 1: epochs 1 .. 29
    assert np.allclose(fires, np.floor(29.0 / st.eps.astype(np.float64)), atol=1)
    assert np.allclose(total, 5.0 * 29.0 / st.eps.astype(np.float64), atol=6)


def test_model_layout_keeps_neighbours_that_pca_loses():
    """The end-to-end case of tests/test_gpu_umap.py, checked on the model first: six clusters in 16 dimensions of which
    the 2-d PCA start overlaps two pairs; the start's 15-neighbour preservation is clearly below the final one."""
    X, lab = ur.clusters_case()
    fit = ur.fit_model(X, 2, 15, seed=0)
    y0 = fit['y0']
    sep = [np.linalg.norm(y0[lab == p].mean(0) - y0[lab == q].mean(0)) / y0[lab == p].std(0).max() for p, q in ((0, 1), (2, 3), (0, 2))]
    assert sep[0] < 3 and sep[1] < 3 and sep[2] > 10                  # two pairs of clusters overlap in the start
    start = ur.neighbor_preservation_model(X, y0, 15)
    final = ur.neighbor_preservation_model(X, fit['embedding'], 15)
    print(f'neighbor preservation: start {start:.3f}, final {final:.3f}')
    assert np.isfinite(fit['embedding']).all() and final > start + 0.1
    assert y0.min() == 0 and y0.max() == 10


# -------------------------------------------------------------------------------------------------------- validation
def test_arguments_are_checked_before_anything_runs():
    from ampnet_amd import umap
    x = torch.randn(20, 5)
    with pytest.raises(ValueError, match='GPU'):
        umap(x)
    for kw in (dict(n_neighbors=1), dict(n_neighbors=21), dict(n_neighbors=257), dict(n_components=1), dict(n_components=33),
               dict(min_dist=1.5), dict(min_dist=-0.1), dict(spread=0.0), dict(n_epochs=0), dict(init='spectral'),
               dict(init=torch.zeros(20, 3)), dict(init=torch.zeros(19, 2)), dict(samples='both'), dict(seed=1.5), dict(a=1.0),
               dict(a=-1.0, b=1.0), dict(neighbors=(torch.zeros(20, 1, dtype=torch.int64), torch.zeros(20, 1))),
               dict(neighbors=(torch.zeros(20, 3, dtype=torch.int32), torch.zeros(20, 3))), dict(n_components=6)):
        with pytest.raises(ValueError):
            umap(x, **kw)
    with pytest.raises(ValueError, match='grad'):
        umap(torch.randn(20, 5, requires_grad=True))
    with pytest.raises(ValueError):
        umap(torch.randn(20, 5).double())
    with pytest.raises(ValueError):
        umap(torch.randn(1, 5))
    with pytest.raises(ValueError):
        umap(torch.randn(20, 300))
