"""CPU checks of tests/pipeline_reference.py, the numpy models the featuriser and sampler kernels are held to by exact
equality (tests/test_gpu_featurizer_kernels.py, tests/test_gpu_sampler_kernels.py): the generator's published vector, the
uniformity of the two model streams (the GPU tests carry no statistical tolerance: they inherit this one), agreement
with the two restatements under oracle/, and one test per model that runs every listed MUTANT of it over the inputs
the GPU tests use -- a mutant that those inputs cannot tell from the model would mean a kernel with that defect passes."""
import numpy as np
import pytest
from scipy.stats import chi2 as chi2_dist

import pipeline_reference as pr
from oracle import featurizer_numpy, graphsaint_numpy

_U = np.uint64


def test_generator_vector_and_draw():
    assert int(pr.splitmix64(_U(0))) == 0xE220A8397B1DCDAF          # the generator's published first output from state 0
    s, a, b = 2 ** 63 + 5, 12345, 678
    inner = int(pr.splitmix64(_U((a * pr.MULT + b) % 2 ** 64)))
    assert int(pr.draw(s, a, b)) == int(pr.splitmix64(_U(s ^ inner)))
    assert int(pr.draw(s, 2 ** 40, 3)) == int(pr.splitmix64(_U(s ^ int(pr.splitmix64(_U((2 ** 40 * pr.MULT + 3) % 2 ** 64))))))
    assert pr.draw(s, np.arange(4)[:, None], np.arange(3)).shape == (4, 3)


def chi2_stat(counts, expected):
    return float(((counts - expected) ** 2 / expected).sum())


def test_model_streams_are_uniform():
    """The chi-square statistic of each model stream below the 99.9 % quantile of its distribution; deterministic.
    Featuriser: 19 present of 1433 columns, L = 4000 (dof 18 -> 42.3).  Walk: 4000 one-step walks from the node with 40
    out-edges, counted per out-edge SLOT (40 cells, dof 39 -> 72.1, below the 73.4 of dof 40) and per distinct
    neighbour with the duplicates' multiplicity in the expectation."""
    assert abs(chi2_dist.ppf(0.999, 18) - 42.3) < 0.05 and abs(chi2_dist.ppf(0.999, 40) - 73.4) < 0.05
    rng = np.random.default_rng(1)
    x = np.zeros((1, 1433), dtype=np.float32)
    present = np.sort(rng.choice(1433, 19, replace=False))
    x[0, present] = 1.0
    for seed in (9, 0, 2 ** 63 + 5):
        idx, empty = pr.sample_present(x, 4000, seed)
        assert not empty and set(idx[0].tolist()) <= set(present.tolist())
        stat = chi2_stat(np.array([(idx[0] == f).sum() for f in present]), 4000 / 19)
        print(f'[chi2] sample_present seed {seed}: {stat:.1f} (dof 18)')
        assert stat < chi2_dist.ppf(0.999, 18)
    e = pr.walk_graph()
    cscptr, crow, _ = pr.csc_of(e, pr.WALK_N)
    slots = crow[cscptr[49]:cscptr[50]]
    assert len(slots) == 40
    for seed in (12345, 2 ** 64 - 1):
        nxt = pr.random_walk(cscptr, crow, np.full(4000, 49), 1, seed)[:, 1]
        slot = (pr.draw(seed, np.arange(4000), 0) % _U(40)).astype(np.int64)
        assert np.array_equal(nxt, slots[slot])
        stat = chi2_stat(np.bincount(slot, minlength=40), 100.0)
        neigh, mult = np.unique(slots, return_counts=True)
        stat_n = chi2_stat(np.array([(nxt == v).sum() for v in neigh]), 4000 * mult / 40)
        print(f'[chi2] random_walk seed {seed}: {stat:.1f} (dof 39), by neighbour {stat_n:.1f} (dof {len(neigh) - 1})')
        assert stat < min(chi2_dist.ppf(0.999, 39), 73.4) and stat_n < chi2_dist.ppf(0.999, len(neigh) - 1)


# ------------------------------------------------------------------------------------- agreement with the oracles
@pytest.mark.parametrize('N,kind', pr.saint_cases(), ids=lambda v: str(v).replace(' ', '_'))
def test_subgraph_model_matches_the_oracle(N, kind):
    e = pr.saint_graph(N)
    cscptr, crow, cperm = pr.csc_of(e, N)
    nodes = pr.saint_node_input(N, kind)
    mark, relabel, node_idx, n_sub = pr.saint_nodes(nodes, N)
    cnt, off, e_sub = pr.count_edges(node_idx, n_sub, cscptr, crow, mark)
    ei, eid = pr.fill_edges(node_idx, n_sub, cscptr, crow, cperm, mark, relabel)
    n_ref, e_ref, keep = graphsaint_numpy.induced_subgraph(e, N, nodes)
    assert np.array_equal(node_idx, n_ref) and e_sub == len(keep) == ei.shape[1]
    order = np.argsort(eid)                                  # the oracle lists the kept edges by edge id: compare as sets
    assert np.array_equal(eid[order], keep) and np.array_equal(ei[:, order], e_ref)
    assert np.array_equal(np.repeat(np.arange(n_sub), cnt[:n_sub]), ei[0])          # grouped by source, ascending
    for nb in pr.n_bounds(n_sub, N):
        c2, o2, e2 = pr.count_edges(node_idx, n_sub, cscptr, crow, mark, nb)
        assert len(c2) == nb + 1 and e2 == e_sub and np.array_equal(c2[:n_sub], cnt[:n_sub]) and not c2[n_sub:].any()
        assert np.array_equal(o2[:n_sub + 1], off)
    if kind == 'leaving':
        assert e_sub == 0 and cscptr[N] - cscptr[N - 1] > 0


@pytest.mark.parametrize('shape', ['N > E', 'E > N', 'E = 0'])
def test_norms_model_is_the_oracle_in_float32(shape):
    nc, ec, src, ns = pr.norm_inputs(shape)
    nn, en = pr.norms(nc, ec, src, len(nc), ns)
    nn_ref, en_ref = graphsaint_numpy.norms(nc, ec, src, len(nc), ns)
    assert nn.dtype == en.dtype == np.float32
    assert np.array_equal(nn.view(np.int32), nn_ref.view(np.int32)) and np.array_equal(en.view(np.int32), en_ref.view(np.int32))
    if len(ec):          # every branch is there: 0 / 0, x / 0, above and below the clamp
        q = nc[src].astype(np.float64) / np.where(ec == 0, np.nan, ec)
        assert ((ec == 0) & (nc[src] == 0)).any() and ((ec == 0) & (nc[src] > 0)).any()
        assert ((q > 1e4) & (q < 1e4 + 1.1)).sum() >= 3 and ((q < 1e4) & (q > 1e4 - 1.1)).sum() >= 3
        assert en[(ec == 0) & (nc[src] == 0)].view(np.int32).tolist() == [np.float32(0.1).view(np.int32)] * 2
        assert (en[q > 1e4] == np.float32(1e4)).all() and (en[(ec == 0) & (nc[src] > 0)] == np.float32(1e4)).all()
    assert (nc == 0).sum() == 3 and (nn[nc == 0] == np.float32(ns) / np.float32(0.1) / np.float32(len(nc))).all()


@pytest.mark.parametrize('N,F,shift', pr.zscore_cases())
def test_zscore_model_matches_sklearn(N, F, shift):
    """The model's fp64 z against sklearn's StandardScaler (oracle/featurizer_numpy.zscore) within the z bar, the verdicts
    away from the rule's border, and a float32 emulation of the kernel and of the module within the bars the GPU is
    held to."""
    x = pr.zscore_columns(N, F, shift)
    mean, inv_std, constant = pr.zscore_stats(x)
    margin, zero = pr.zscore_margin(x)
    assert margin > 1e6 and zero, (margin, zero)
    z64 = (x.astype(np.float64) - mean) * inv_std
    bar = pr.z_bar(mean, inv_std, z64)
    assert (np.abs(featurizer_numpy.zscore(x).astype(np.float64) - z64) <= bar).all()
    m32, s32, c32 = kernel_stats(x)
    assert np.array_equal(c32, constant)
    assert pr.ulp_distance(m32, mean.astype(np.float32)).max() <= 1 and pr.ulp_distance(s32, inv_std.astype(np.float32)).max() <= 1
    z32 = ((x - m32).astype(np.float32) * s32).astype(np.float32)
    assert (np.abs(z32.astype(np.float64) - z64) <= bar).all()
    assert (z32[:, constant] == 0).all()


def kernel_stats(x, ddof=0, rule=True, mean_dtype=np.float64):
    """zscore_stats_kernel's arithmetic: sequential sums in double (mutants: fp32 accumulation of the mean, the sample
    variance, no constant rule) -> (mean fp32, inv_std fp32, constant)."""
    N = x.shape[0]
    s = np.zeros(x.shape[1], dtype=mean_dtype)
    for n in range(N):
        s = s + x[n].astype(mean_dtype)
    m = (s / mean_dtype(N)).astype(np.float64)
    v = np.zeros(x.shape[1])
    for n in range(N):
        v += (x[n].astype(np.float64) - m) ** 2
    with np.errstate(divide='ignore', invalid='ignore'):
        v = v / (N - ddof)
        constant = (v <= pr.zscore_bound(m, v, N)) if rule else np.zeros(len(v), bool)
        inv_std = np.where(constant, 1.0, 1.0 / np.sqrt(v))
    return m.astype(np.float32), inv_std.astype(np.float32), constant


# ---------------------------------------------------------------------------------------------------------- mutants
def sample_mutant(x, L, seed, kind):
    """sample_present as the kernel walks it -- 64-column masks, prefix counts, the rank's chunk, its k-th set bit --
    with one defect."""
    N, F = x.shape
    idx = np.full((N, L), -1, dtype=np.int32)
    if kind == 'seed32':
        seed &= 0xFFFFFFFF
    for n in range(N):
        present = (x[n] > 0) if kind == 'positive' else (x[n] != 0)
        count = int(present.sum())
        if count == 0:
            continue
        chunks = [np.nonzero(present[c:c + 64])[0] for c in range(0, F, 64)]
        prefix = np.concatenate([[0], np.cumsum([len(c) for c in chunks])])
        for l in range(L):
            r = int(pr.draw(seed, l, n) if kind == 'swapped' else pr.draw(seed, n, l))
            k = r % (max(count - 1, 1) if kind == 'count - 1' else count)
            if kind == 'all columns':
                idx[n, l] = r % F
                continue
            c = 0
            while c + 1 < len(chunks) and (prefix[c + 1] < k if kind == 'strict' else prefix[c + 1] <= k):
                c += 1
            k -= prefix[c]
            idx[n, l] = c * 64 + (chunks[c][k] if k < len(chunks[c]) else -1)      # no bit left: ffs(0) - 1
    return idx


def test_sampling_inputs_tell_the_mutants_apart():
    kinds = ('none', 'all columns', 'strict', 'swapped', 'count - 1', 'positive', 'seed32')
    differs = dict.fromkeys(kinds, 0)
    for F, L, seed in pr.sample_cases():
        x = pr.sample_rows(F)
        want, empty = pr.sample_present(x, L, seed)
        assert empty == 1 and (want[pr.EMPTY_ROW] == -1).all() and (np.delete(want, pr.EMPTY_ROW, 0) >= 0).all()
        assert featurizer_numpy.indices_are_present(np.delete(x, pr.EMPTY_ROW, 0), np.delete(want, pr.EMPTY_ROW, 0))
        if L > 40 and F > 200:
            x, want = x[:24], want[:24]                      # the walk above is a Python loop: the constructed rows and a few more
        for kind in kinds:
            differs[kind] += int(not np.array_equal(sample_mutant(x, L, seed, kind), want))
    assert differs.pop('none') == 0                          # the emulated walk IS the model
    assert all(differs.values()), differs
    print('[mutants] sample_present, cases that differ of', len(pr.SAMPLE_CASES), differs)


def walk_mutant(e, start, wl, seed, kind):
    N = pr.WALK_N
    ptr, nbr, _ = pr.csc_of(e[::-1] if kind == 'in-neighbours' else e, N)
    if kind == 'seed32':
        seed &= 0xFFFFFFFF
    walks = np.empty((len(start), wl + 1), dtype=np.int64)
    for b, cur in enumerate(start):
        walks[b, 0] = cur
        for t in range(wl):
            deg = int(ptr[cur + 1] - ptr[cur])
            r = int(pr.draw(seed, t, b) if kind == 'swapped' else pr.draw(seed, b, t))
            cur = nbr[ptr[cur] + r % deg] if deg else (0 if kind == 'sink to 0' else cur)
            walks[b, t + 1] = cur
    return walks


def test_walk_inputs_tell_the_mutants_apart():
    e = pr.walk_graph()
    cscptr, crow, _ = pr.csc_of(e, pr.WALK_N)
    kinds = ('none', 'in-neighbours', 'swapped', 'sink to 0', 'seed32')
    differs = dict.fromkeys(kinds, 0)
    for B, wl, seed in pr.walk_cases():
        start = pr.walk_starts(B)
        want = pr.random_walk(cscptr, crow, start, wl, seed)
        assert want.shape == (B, wl + 1) and graphsaint_numpy.walk_is_valid(e, pr.WALK_N, want)
        for kind in kinds:
            differs[kind] += int(not np.array_equal(walk_mutant(e, start, wl, seed, kind), want))
    assert differs.pop('none') == 0 and all(differs.values()), differs
    print('[mutants] random_walk, cases that differ of', len(pr.WALK_CASES), differs)


def fill_mutant(node_idx, n_sub, cscptr, crow, cperm, mark, relabel, kind):
    s, d, e = [], [], []
    for k in (range(n_sub - 1, -1, -1) if kind == 'descending' else range(n_sub)):
        u = node_idx[k]
        for p in range(cscptr[u], cscptr[u + 1]):
            if mark[crow[p]] or kind == 'keeps unsampled':
                s.append(k), d.append(crow[p] if kind == 'no relabel' else relabel[crow[p]])
                e.append(p if kind == 'csc position' else cperm[p])
    return np.array([s, d], dtype=np.int64).reshape(2, -1), np.array(e, dtype=np.int64)


def test_subgraph_inputs_tell_the_mutants_apart():
    kinds = ('none', 'keeps unsampled', 'csc position', 'no relabel', 'descending')
    differs = dict.fromkeys(kinds, 0)
    for N, kind in pr.saint_cases():
        cscptr, crow, cperm = pr.csc_of(pr.saint_graph(N), N)
        mark, relabel, node_idx, n_sub = pr.saint_nodes(pr.saint_node_input(N, kind), N)
        want = pr.fill_edges(node_idx, n_sub, cscptr, crow, cperm, mark, relabel)
        for m in kinds:
            got = fill_mutant(node_idx, n_sub, cscptr, crow, cperm, mark, relabel, m)
            differs[m] += int(not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])))
    assert differs.pop('none') == 0 and all(differs.values()), differs
    print('[mutants] fill_edges, cases that differ of', len(pr.saint_cases()), differs)


def norms_mutant(nc, ec, src, N, ns, kind):
    nn, en = pr.norms(nc, ec, src, N, ns)
    t = np.asarray(nc, np.float32)[src]
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == '0/0 -> 1e4':
            en[(ec == 0) & (t == 0)] = np.float32(1e4)
        if kind == 'no clamp':
            en = np.where(ec == 0, en, t / ec).astype(np.float32)
        if kind == 'count 0 kept':
            nn = (np.float32(ns) / np.asarray(nc, np.float32) / np.float32(N)).astype(np.float32)
    return nn, en


def test_norms_inputs_tell_the_mutants_apart():
    """At the bars the GPU test applies: 1 ulp on edge_norm, 2 ulp on node_norm."""
    for shape in ('N > E', 'E > N', 'E = 0'):
        nc, ec, src, ns = pr.norm_inputs(shape)
        nn, en = pr.norms(nc, ec, src, len(nc), ns)
        for kind in ('0/0 -> 1e4', 'no clamp', 'count 0 kept'):
            mn, me = norms_mutant(nc, ec, src, len(nc), ns, kind)
            caught = pr.ulp_distance(mn, nn).max(initial=0) > 2 or pr.ulp_distance(me, en).max(initial=0) > 1
            assert caught == (kind == 'count 0 kept' or shape != 'E = 0'), (shape, kind)


def test_zscore_inputs_tell_the_mutants_apart():
    """Sample variance, no constant rule, fp32 accumulation of the mean: each misses a bar of the GPU test (1 ulp on mean
    and inv_std, the verdict) somewhere in the cases, and the plain emulation misses none (test_zscore_model_matches_sklearn)."""
    caught = dict.fromkeys(('ddof', 'no rule', 'fp32 mean'), 0)
    for N, F, shift in pr.zscore_cases():
        x = pr.zscore_columns(N, F, shift)
        mean, inv_std, constant = pr.zscore_stats(x)
        for kind, kw in (('ddof', dict(ddof=1)), ('no rule', dict(rule=False)), ('fp32 mean', dict(mean_dtype=np.float32))):
            m, s, c = kernel_stats(x, **kw)
            ok = (np.array_equal(c, constant) and pr.ulp_distance(m, mean.astype(np.float32)).max() <= 1
                  and pr.ulp_distance(s, inv_std.astype(np.float32)).max() <= 1)
            caught[kind] += int(not ok)
    assert all(caught.values()), caught
    print('[mutants] zscore_stats, cases caught of', len(pr.zscore_cases()), caught)


def table_grad_f32(dout, idx, F, kind='none'):
    """table_grad_kernel in float32, tokens in launch order (mutants: row stride De, idx -1 into row F - 1)."""
    De = dout.shape[-1] - 1
    flat, out = dout.reshape(-1), np.zeros((F, De), dtype=np.float32)
    stride = De if kind == 'stride' else De + 1
    for t, f in enumerate(idx.reshape(-1)):
        if f < 0 and kind != 'minus one':
            continue
        out[f] += flat[t * stride:t * stride + De]           # (numpy: row -1 IS row F - 1)
    return out


@pytest.mark.parametrize('De', [d for d in pr.DE if d > 0])
def test_table_grad_inputs_tell_the_mutants_apart(De):
    for pattern in pr.PATTERNS:
        for kind in ('exact', 'random'):
            dout, idx = pr.grad_inputs(De, pattern, kind)
            ref, S, n = pr.table_grad(dout, idx, pr.GRAD_F)
            assert not ref[pr.GRAD_F - 4:].any() and n.sum() == (idx >= 0).sum()

            def passes(got):
                if kind == 'exact':
                    return np.array_equal(got.view(np.int32), (ref + 0.0).astype(np.float32).view(np.int32))
                return pr.random_share(got, ref, S, n) <= 1
            assert passes(table_grad_f32(dout, idx, pr.GRAD_F))
            assert not passes(table_grad_f32(dout, idx, pr.GRAD_F, 'stride')), (pattern, kind)
            if pattern == 'with -1':
                assert not passes(table_grad_f32(dout, idx, pr.GRAD_F, 'minus one')), kind
            if kind == 'exact':                              # ... and every exact value is a bf16 number
                assert np.array_equal(pr.to_bf16(dout), dout)
    if De == 1:
        assert pr.grad_inputs(De, 'hot', 'exact')[1].size == 4096


def test_token_model_and_inputs():
    """build_tokens_f32 against the oracle's concatenation where the two agree by construction (mean, inv_std of sklearn
    rounded to fp32: the z bar), zero rows for idx -1, and the last channel not a copy of x."""
    for De in pr.DE:
        x, mean, inv_std, idx, table = pr.token_inputs(De)
        out = pr.build_tokens_f32(x, mean, inv_std, idx, table)
        assert out.shape == (pr.TOKEN_N, pr.TOKEN_L, De + 1) and out.dtype == np.float32
        assert (idx == -1).sum() > pr.TOKEN_L and not out[idx == -1].any() and out[idx >= 0][:, De].all()
        assert idx.max() == pr.TOKEN_F - 1 and idx[idx >= 0].min() == 0
    x = pr.sample_rows(65)[pr.N_CONSTRUCTED:]
    idx = np.delete(pr.sample_present(x, 8, 3)[0], [], 0)
    m64, s64, _ = pr.zscore_stats(x)
    table = np.random.default_rng(0).standard_normal((65, 3)).astype(np.float32)
    got = pr.build_tokens_f32(x, m64.astype(np.float32), s64.astype(np.float32), idx, table)
    want = featurizer_numpy.build_tokens(x, idx, table).reshape(got.shape)
    assert np.array_equal(got[..., :3], want[..., :3])
    rows = np.arange(len(x))[:, None]
    z64 = ((x.astype(np.float64) - m64) * s64)[rows, idx]
    assert (np.abs(got[..., 3] - z64) <= pr.z_bar(m64[idx], s64[idx], z64)).all()
    assert (np.abs(want[..., 3] - z64) <= pr.z_bar(m64[idx], s64[idx], z64)).all()
