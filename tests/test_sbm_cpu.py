"""The numpy model of the stochastic block model generator (tests/sbm_reference.py) held to what include/ampconv.h,
"THE BLOCK MODEL", promises -- its invariants on the whole ladder, the margin condition of every (case, seed) pair, the
5-sigma count bar per block pair, the first moments against networkx -- and shown to differ from each of its mutants on
the ladder; then the argument checks of ampnet_amd.random_graphs, which run before the library is loaded.  No GPU.

Figures of the ladder as committed (702 runs, 1923 block pairs with 0 < p < 1): smallest margin 8.3e-8
([100]*4, asymmetric, directed, seed 3), the larger case's 1.6e-9; largest count deviation 3.56 standard deviations
([64, 65, 63, 1], p = 0.3, undirected, seed 0)."""
import numpy as np
import pytest

import sbm_reference as sr

LADDER = sr.ladder()


def runs(cases=LADDER):
    for c in cases:
        for seed in sr.SEEDS:
            yield c, seed, sr.reference(*c, seed)


# -------------------------------------------------------------------------------------------------------------- invariants
@pytest.mark.parametrize('sizes', [tuple(s) for s in sr.SIZES], ids=lambda s: 'x'.join(map(str, s)))
def test_model_invariants(sizes):
    """No duplicate pair, no self loop unless asked, columns in range and in their unit's block order, row-major order,
    mirrors present and in the order of their originals, p = 1 every candidate, p = 0 none; counts and offsets consistent."""
    K, N = len(sizes), sum(sizes)
    for c, seed, r in runs([c for c in LADDER if c[0] == sizes]):
        _, name, directed, selfloops = c
        e, P = r.edge_index, sr.MATRICES[name](K)
        assert e.dtype == np.int64 and e.shape[0] == 2 and r.block.shape == (N,)
        assert np.array_equal(r.block, np.repeat(np.arange(K), sizes))
        assert ((e >= 0) & (e < N)).all(), c
        key = e[0] * N + e[1]
        assert np.unique(key).size == key.size, (c, seed, 'duplicate pair')
        if not selfloops:
            assert (e[0] != e[1]).all(), (c, seed, 'self loop')
        up = e[:, :r.e_upper]
        assert (np.diff(up[0] * N + up[1]) > 0).all(), (c, seed, 'not row-major ascending')
        if directed:
            assert r.e_upper == e.shape[1]
        else:
            assert (up[0] <= up[1]).all()
            keep = up[0] != up[1]
            assert np.array_equal(e[:, r.e_upper:], up[::-1][:, keep]), (c, seed, 'mirrors')
        n_pairs, got = sr.candidate_pairs(sizes, directed, selfloops), sr.pair_counts(r, K, not directed)
        assert np.array_equal(got[P >= 1], n_pairs[P >= 1]) and (got[P <= 0] == 0).all(), (c, seed)
        assert r.count.sum() == r.e_upper and (directed or r.mcount.sum() == e.shape[1] - r.e_upper), (c, seed)
        assert np.array_equal(r.off, np.cumsum(r.count) - r.count) and np.array_equal(r.moff, np.cumsum(r.mcount) - r.mcount)
        unit = r.block[up[1]] + K * up[0]
        assert np.array_equal(np.bincount(unit, minlength=N * K), r.count), (c, seed)


def test_every_pair_of_the_ladder_meets_the_margin_condition():
    worst = min((r.margin, sr.case_id(c), seed) for c, seed, r in runs())
    big = min((sr.big_reference(d, seed).margin, d, seed) for d in (True, False) for seed in sr.SEEDS)
    print(f'[margin] ladder: {worst}; larger case: {big}')
    assert worst[0] >= sr.MARGIN_MIN and big[0] >= sr.MARGIN_MIN, (worst, big)


def test_counts_lie_within_five_standard_deviations():
    """Per block pair: |count - n_pairs p| <= 5 sqrt(n_pairs p (1 - p)); exact where p is 0 or 1."""
    worst, pairs = (0.0, None, None), 0
    cases = [(c, seed, r, len(c[0]), sr.MATRICES[c[1]](len(c[0]))) for c, seed, r in runs()]
    cases += [(((5000,) * 4, 'larger', d, False), seed, sr.big_reference(d, seed), 4, sr.in_out(4, sr.BIG['p_in'], sr.BIG['p_out']))
              for d in (True, False) for seed in sr.SEEDS]
    for c, seed, r, K, P in cases:
        n = sr.candidate_pairs(c[0], c[2], c[3])
        got = sr.pair_counts(r, K, not c[2])
        mean, sd = n * P, np.sqrt(n * P * (1 - P))
        rnd = sd > 0
        assert np.array_equal(got[~rnd], mean[~rnd]), (c, seed)
        if rnd.any():
            z = np.abs(got - mean)[rnd] / sd[rnd]
            pairs += int(rnd.sum())
            if z.max() > worst[0]:
                worst = (float(z.max()), sr.case_id(c), seed)
    print(f'[counts] {pairs} block pairs, worst {worst}')
    assert worst[0] <= 5.0, worst


NX_SIZES = (6, 5, 0, 7)
NX_P = np.array([[0.5, 0.2, 0.3, 0.1], [0.2, 0.6, 0.3, 0.05], [0.3, 0.3, 0.3, 0.3], [0.1, 0.05, 0.3, 0.4]])


@pytest.mark.parametrize('directed,selfloops', [(False, False), (True, False), (False, True), (True, True)])
def test_first_moments_agree_with_networkx(directed, selfloops):
    """300 seeds at sizes [6, 5, 0, 7]: the per-block-pair mean count of the model and that of
    networkx.stochastic_block_model each within 5 standard errors of n_pairs p."""
    nx = pytest.importorskip('networkx')
    K, R = 4, 300
    n = sr.candidate_pairs(NX_SIZES, directed, selfloops)
    block = sr.blocks_of(NX_SIZES)
    ours, theirs = np.zeros((K, K)), np.zeros((K, K))
    for seed in range(R):
        ours += sr.pair_counts(sr.block_model(NX_SIZES, NX_P, directed, selfloops, seed), K, not directed)
        g = nx.stochastic_block_model(list(NX_SIZES), NX_P.tolist(), seed=seed, directed=directed, selfloops=selfloops)
        e = np.array(list(g.edges()), dtype=np.int64).reshape(-1, 2)
        if not directed:
            e = np.sort(e, axis=1)
        theirs += np.bincount(block[e[:, 0]] * K + block[e[:, 1]], minlength=K * K).reshape(K, K)
    mean, se = n * NX_P, np.sqrt(n * NX_P * (1 - NX_P) / R)
    live = se > 0
    for name, got in (('model', ours / R), ('networkx', theirs / R)):
        assert np.array_equal(got[~live], mean[~live]), name
        z = np.abs(got - mean)[live] / se[live]
        print(f'[networkx] {name}: worst {z.max():.2f} standard errors')
        assert z.max() <= 5.0, (name, z)


# ----------------------------------------------------------------------------------------------------------------- mutants
def differing_runs(mutant):
    out = []
    for c, seed, r in runs():
        m = sr.block_model(c[0], sr.MATRICES[c[1]](len(c[0])), c[2], c[3], seed, mutant=mutant)
        if m.edge_index.shape != r.edge_index.shape or not np.array_equal(m.edge_index, r.edge_index):
            out.append((sr.case_id(c), seed))
    return out


@pytest.mark.parametrize('mutant', ['u_stays_a_candidate', 'counter_b_major', 'stop_after_the_cast'])
def test_the_ladder_tells_the_model_from_its_mutant(mutant):
    """The candidate list not excluding u, the counter b N + u in place of u K + b, the stop test after the cast to
    int64: each gives another edge_index than the model on runs of the ladder (the cast only where q overflows it: the
    1e-300 entry of the mixed matrix, from K = 4 on)."""
    diff = differing_runs(mutant)
    print(f'[mutant] {mutant}: {len(diff)} of {len(LADDER) * len(sr.SEEDS)} runs differ')
    assert diff, mutant
    if mutant == 'stop_after_the_cast':
        assert all('mixed' in name for name, _ in diff)


def test_the_ladder_tells_u_without_the_plus_one_where_a_draw_is_small():
    """U = (r >> 11) 2^-53 in place of ((r >> 11) + 1) 2^-53 moves log(U) by 2^-53 / U: the graphs differ only where
    r < 2^11 (U = 0, q infinite, the chain stops), a 2^-53 event per draw that no seed list reaches -- on the ladder as it
    stands the two give the same edges, which is asserted here so that it is known.  With such a draw PLANTED as the first
    of every chain (r = 0: U = 2^-53, q = 36.7 / |lq|) the ladder's cases tell them apart: the model skips
    floor(q) candidates and emits the next, the mutant emits nothing."""
    assert differing_runs('u_without_plus_one') == []

    def planted(seed, a, t):
        return sr.draw(seed, a, t) if t else np.zeros(np.shape(a), np.uint64)
    told = 0
    for c in LADDER:
        P = sr.MATRICES[c[1]](len(c[0]))
        good = sr.block_model(c[0], P, c[2], c[3], 0, stream=planted)
        bad = sr.block_model(c[0], P, c[2], c[3], 0, mutant='u_without_plus_one', stream=planted)
        rnd = (P > 0) & (P < 1)
        assert np.array_equal(sr.pair_counts(bad, len(c[0]), not c[2])[rnd], np.zeros(int(rnd.sum()), np.int64)), c
        told += good.edge_index.shape[1] != bad.edge_index.shape[1]
    assert told >= 20, told                 # the cases with a block of more than floor(q) + 1 candidates: 103 at p = 0.3


# ------------------------------------------------------------------------------------------------- the wrappers' validation
def test_wrapper_validation_needs_no_gpu(monkeypatch):
    """Every argument error is a ValueError raised before the library is loaded (load() is made to fail loudly)."""
    from ampnet_amd import _lib, random_graphs as rg

    def no_load():
        raise AssertionError('the library was loaded before the arguments were checked')
    monkeypatch.setattr(_lib, 'load', no_load)
    sbm = rg.stochastic_block_model
    ok = [[0.5, 0.1], [0.1, 0.5]]
    bad = [
        dict(sizes=[[3, 4]], p=ok),                                  # sizes not a list of numbers
        dict(sizes=[], p=[]),                                        # no block
        dict(sizes=[3, -1], p=ok),                                   # negative size
        dict(sizes=[3.5, 2], p=ok),                                  # not an integer
        dict(sizes=[3, 4], p=[0.5, 0.1]),                            # p not [K, K]
        dict(sizes=[3, 4], p=[[0.5, 0.1, 0.1], [0.1, 0.5, 0.1]]),
        dict(sizes=[3, 4, 5], p=ok),
        dict(sizes=[3, 4], p=[[0.5, float('nan')], [float('nan'), 0.5]]),
        dict(sizes=[3, 4], p=[[0.5, float('inf')], [float('inf'), 0.5]]),
        dict(sizes=[3, 4], p=[[0.5, -0.1], [-0.1, 0.5]]),
        dict(sizes=[3, 4], p=[[1.5, 0.1], [0.1, 0.5]]),
        dict(sizes=[3, 4], p=[[0.5, 0.1], [0.2, 0.5]]),              # asymmetric, undirected
        dict(sizes=[1] * 257, p=np.full((257, 257), 0.5)),           # K > 256
        dict(sizes=[2 ** 30, 2 ** 30], p=ok),                        # N > 2^31 - 1
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            sbm(**kw)
    with pytest.raises(ValueError):
        sbm([3, 4], ok, device='cpu')                                # no CPU fallback
    for args in (([3, 4], 1.5, 0.1), ([3, 4], 0.5, -0.1), ([3, -4], 0.5, 0.1)):
        with pytest.raises(ValueError):
            rg.random_partition_graph(*args)
    for args in ((10, 1.5), (-3, 0.5)):
        with pytest.raises(ValueError):
            rg.gnp_random_graph(*args)
    for kw in (dict(num_samples=10), dict(num_samples=8, same_class_link_prob=1.0), dict(num_samples=8, diff_class_link_prob=-0.1),
               dict(num_samples=8, diff_class_link_prob=1.0), dict(num_samples=8, noise_std=float('nan'))):
        with pytest.raises(ValueError):
            rg.xor_link_dataset(**kw)
    P = rg.xor_link_matrix(0.7, 0.1)
    assert np.array_equal(P, np.array([[.7, .1, .1, .7], [.1, .7, .7, .1], [.1, .7, .7, .1], [.7, .1, .1, .7]]))
