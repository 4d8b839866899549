"""ampnet_amd.umap on the GPU against the fp64 models of tests/umap_reference.py: the memberships kernel, the fuzzy
union, ONE epoch of the layout from the model's own state, then umap() end to end and the model hook.

The bounds (u = 2^-24):

  memberships  sigma and rho to 1e-12 relative -- fp64 against fp64 with the same branch sequence: what is left is the
               order of the fp64 sums and the last bits of exp.  The memberships to 2 ulp of float32: one rounding of an
               fp64 value that agrees with the model's to ~1e-12.
  fuzzy union  indptr / indices element for element, values bit for bit (a float32 expression of float32 inputs).
  epoch        next, nextneg, drawn bit for bit (float32 / int32 statements of the header); Y_out within
               umap_reference.epoch_bound, which derives the bound from the summation structure and the measured error
               of the coefficients (R_COEFF, profiles/umap.md) under the margin of 4.
"""
import importlib
import types

import numpy as np
import pytest
import torch

import umap_reference as ur
from edge_runner import stream

from ampnet_amd import _lib

um = importlib.import_module('ampnet_amd.umap')
pytestmark = pytest.mark.gpu

BADARG, EWORKSPACE = -1, -3
# The spread (largest - smallest) of the MODEL's 15-neighbour preservation on umap_reference.clusters_case over the
# seeds 0 .. 4, 500 epochs from the PCA start (profiles/umap.md, "end to end"): measured on the model, not on the kernels.
NP_SPREAD = 0.0185


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def dev():
    return torch.device('cuda:0')


def to_dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return t.to(dev(), dtype) if dtype is not None else t.to(dev())


def strided(a, pad=3):
    """a [rows, cols] as a row-strided view (row stride cols + pad) inside a NaN-filled buffer with NaN margins."""
    rows, cols = a.shape
    backing = torch.full((16 + rows * (cols + pad),), float('nan'), dtype=torch.float32, device=dev())
    view = torch.as_strided(backing, (rows, cols), (cols + pad, 1), 8)
    view.copy_(to_dev(a, torch.float32))
    return view, backing


def ulps32(got, want):
    """|got - want| in units of the float32 spacing at want (float32 arrays; denormal spacing at 0)."""
    want = np.asarray(want, np.float32)
    spacing = np.maximum(np.spacing(np.abs(want)), np.float32(2.0 ** -149)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / spacing


# ----------------------------------------------------------------------------------------------------- memberships
MEMBERSHIP_CASES = ((2, 2), (65, 2), (65, 15), (65, 64), (300, 15), (300, 64), (300, 256))


def membership_case(M, k, seed=0):
    """Points at very different scales with a block of 20 exact duplicates (all of a duplicate's distances are 0 up to
    k = 20: rho = 0 and the global floor; beyond, rho is the first positive distance)."""
    rng = np.random.default_rng(seed + 1000 * M + k)
    X = rng.normal(0.0, 1.0, (M, 6)) * rng.choice([0.05, 1.0, 30.0], (M, 1))
    if M >= 40:
        X[10:30] = X[10]
    return ur.neighbors_with_self(X, k)


def test_memberships_sweep():
    bad = []
    for M, k in MEMBERSHIP_CASES:
        name = f'memberships M{M} k{k}'
        idx, dist = membership_case(M, k)
        view, backing = strided(dist)
        before = backing.clone()
        memb, sigma, rho = um.memberships(to_dev(idx), view)
        again = um.memberships(to_dev(idx), view)
        torch.cuda.synchronize()
        if not torch.equal(backing.view(torch.int32), before.view(torch.int32)):
            bad.append(f'{name}: the input buffer was written')
        want, ws, wr = ur.memberships_model(idx, dist)
        gs, gr, gm = sigma.cpu().numpy(), rho.cpu().numpy(), memb.cpu().numpy()
        if not (np.abs(gs - ws) <= 1e-12 * ws).all():
            bad.append(f'{name}: sigma off by {(np.abs(gs - ws) / ws).max():.3e} relative')
        if not (np.abs(gr - wr) <= 1e-12 * wr).all():
            bad.append(f'{name}: rho off by {np.abs(gr - wr).max():.3e}')
        off = ulps32(gm, want.astype(np.float32))
        if not (off <= 2).all():
            bad.append(f'{name}: memberships off by {off.max():.1f} ulp')
        if not ((gm[:, 0] == 0).all() and np.isfinite(gm).all()):
            bad.append(f'{name}: column 0 or a non-finite membership')
        if M >= 40 and k <= 20 and not ((gr[10:30] == 0).all() and (gm[10:30, 1:] == 1).all()):
            bad.append(f'{name}: the duplicates')
        if not all(torch.equal(a, b) for a, b in zip((memb, sigma, rho), again)):
            bad.append(f'{name}: two calls differ')
    assert not bad, '\n'.join(bad)


def test_memberships_bad_arguments(lib):
    idx, dist = membership_case(65, 15)
    di, dd = to_dev(idx), to_dev(dist)
    memb = torch.full((65, 15), float('nan'), device=dev())
    sigma, rho = torch.full((65,), float('nan'), dtype=torch.float64, device=dev()), torch.full((65,), float('nan'), dtype=torch.float64, device=dev())
    ws = torch.empty(max(int(lib.ampconv_umap_memberships_workspace_bytes(65)), 256), dtype=torch.uint8, device=dev())
    base = dict(idx=di.data_ptr(), ldi=15, dist=dd.data_ptr(), ldd=15, M=65, k=15, memb=memb.data_ptr(), sigma=sigma.data_ptr(),
                rho=rho.data_ptr(), ws=ws.data_ptr(), wsn=ws.numel())
    for name, change, want in (('M = 1', dict(M=1), BADARG), ('k = 1', dict(k=1), BADARG), ('k = 257', dict(k=257, ldi=257, ldd=257), BADARG),
                               ('k > M', dict(M=10), BADARG), ('ldd < k', dict(ldd=14), BADARG), ('ldi < k', dict(ldi=14), BADARG),
                               ('NULL idx', dict(idx=None), BADARG), ('NULL dist', dict(dist=None), BADARG), ('NULL memb', dict(memb=None), BADARG),
                               ('NULL sigma', dict(sigma=None), BADARG), ('misaligned rho', dict(rho=rho.data_ptr() + 4), BADARG),
                               ('NULL workspace', dict(ws=None), EWORKSPACE), ('short workspace', dict(wsn=64), EWORKSPACE)):
        a = dict(base)
        a.update(change)
        got = lib.ampconv_umap_memberships(a['idx'], a['ldi'], a['dist'], a['ldd'], a['M'], a['k'], a['memb'], a['sigma'], a['rho'],
                                           a['ws'], a['wsn'], stream())
        assert got == want, name
    torch.cuda.synchronize()
    assert torch.isnan(memb).all() and torch.isnan(sigma).all() and torch.isnan(rho).all()
    assert lib.ampconv_umap_memberships_workspace_bytes(1) == 0


# ----------------------------------------------------------------------------------------------------- fuzzy union
def test_fuzzy_graph_equals_the_model_bit_for_bit():
    bad = []
    for M, k in ((2, 2), (65, 15), (300, 64)):
        idx, dist = membership_case(M, k)
        memb, _, _ = um.memberships(to_dev(idx), to_dev(dist))
        indptr, indices, val = um.fuzzy_graph(to_dev(idx), memb)
        wp, wi, wv = ur.fuzzy_model(idx, memb.cpu().numpy())
        gp, gi, gv = indptr.cpu().numpy(), indices.cpu().numpy(), val.cpu().numpy()
        if not (np.array_equal(gp, wp) and np.array_equal(gi, wi)):
            bad.append(f'M{M} k{k}: indptr / indices differ from the model')
            continue
        if not np.array_equal(gv.view(np.int32), wv.view(np.int32)):
            bad.append(f'M{M} k{k}: values differ from the model in {(gv.view(np.int32) != wv.view(np.int32)).sum()} entries')
        W = np.zeros((M, M), np.float32)
        W[np.repeat(np.arange(M), np.diff(gp)), gi] = gv
        if not np.array_equal(W.view(np.int32), W.T.copy().view(np.int32)):
            bad.append(f'M{M} k{k}: W differs from its transpose')
        if not all(torch.equal(a, b) for a, b in zip((indptr, indices, val), um.fuzzy_graph(to_dev(idx), memb))):
            bad.append(f'M{M} k{k}: two calls differ')
    assert not bad, '\n'.join(bad)


# ------------------------------------------------------------------------------------------------------- one epoch
N_EPOCHS, EPOCHS, SEED = 60, (0, 1, 7, 59), 11
PARTS = (None, 64, 128, 1 << 20)          # the library's part length, two small ones (the hub row is cut), one large


@pytest.fixture(scope='module', params=(70, 300))
def hub(request):
    """The model's graph and schedule of a case whose row 0 is a hub (every other sample's nearest neighbour), built
    through neighbors=(idx, dist): computed once per M and shared by the dimensions."""
    M = request.param
    _, idx, dist = ur.hub_neighbors(M, 15, seed=M)
    memb, _, _ = ur.memberships_model(idx, dist)
    graph = ur.fuzzy_model(idx, memb.astype(np.float32))
    assert graph[0][1] - graph[0][0] == M - 1
    return dict(M=M, idx=idx, dist=dist, graph=graph, sched=ur.schedule_model(*graph, N_EPOCHS), ab=ur.find_ab_params())


def run_epoch(c, y32, st, n, dim, part):
    a, b = c['ab']
    indptr, indices, eps = c['sched']
    lay = um.Layout(to_dev(y32), to_dev(indptr), to_dev(indices), to_dev(eps), a, b, N_EPOCHS, SEED, part=part)
    fresh = ur.State(indptr, indices, eps)
    start_ok = (np.array_equal(lay.next.cpu().numpy().view(np.int32), fresh.next.view(np.int32))
                and np.array_equal(lay.nextneg.cpu().numpy().view(np.int32), fresh.nextneg.view(np.int32)) and not bool(lay.drawn.any()))
    lay.next, lay.nextneg, lay.drawn = to_dev(st.next), to_dev(st.nextneg), to_dev(st.drawn)
    lay.epoch(n)
    torch.cuda.synchronize()
    return lay, start_ok


@pytest.mark.parametrize('dim', (2, 3, 30))
def test_one_epoch_from_the_models_state(hub, dim):
    c, M = hub, hub['M']
    a, b = c['ab']
    rng = np.random.default_rng(dim)
    Y = ur.scaled_start_model(rng.normal(0.0, 1.0, (M, dim))).astype(np.float64)
    st = ur.State(*c['sched'])
    bad, zero_edges, zero_negatives, cut = [], 0, 0, 0
    for n in range(N_EPOCHS):
        if n in EPOCHS:
            name = f'M{M} dim{dim} epoch {n}'
            y32 = Y.astype(np.float32)
            y32[1] = y32[0]                                           # two coincident points joined by an entry of weight 1
            want_st = st.copy()
            want, info = ur.epoch_gather(y32.astype(np.float64), want_st, n, N_EPOCHS, a, b, SEED)
            zero_edges += info['zero_edges']
            zero_negatives += info['zero_negatives']
            runs = [run_epoch(c, y32, st, n, dim, part) for part in PARTS + (None,)]
            lay = runs[0][0]
            if not all(ok for _, ok in runs):
                bad.append(f'{name}: the start state of Layout differs from the model')
            got = lay.y[0].cpu().numpy()
            if not np.array_equal(lay.y[1].cpu().numpy(), y32):
                bad.append(f'{name}: Y_in was changed')
            for what, g, w in (('next', lay.next, want_st.next), ('nextneg', lay.nextneg, want_st.nextneg), ('drawn', lay.drawn, want_st.drawn)):
                if not np.array_equal(g.cpu().numpy().view(np.int32), w.view(np.int32)):
                    bad.append(f'{name}: {what} differs from the model in {(g.cpu().numpy() != w).sum()} entries')
            bound = ur.epoch_bound(info, want, dim, b)
            err = np.abs(got.astype(np.float64) - want)
            used = (err / np.maximum(bound, 2.0 ** -149)).max()
            print(f'{name}: {info["fired"].size} entries fired, {int(info["m"].sum())} negatives, largest error {used:.3f} of the bound')
            if not (np.isfinite(got).all() and (err <= bound).all()):
                bad.append(f'{name}: Y_out off by {used:.3g} x the bound')
            if n == 0 and not np.array_equal(got, y32):
                bad.append(f'{name}: nothing fires in epoch 0, yet Y moved')
            for (other, _), part in zip(runs[1:], PARTS[1:] + ('a second run',)):
                same = (torch.equal(other.y[0], lay.y[0]) and torch.equal(other.next, lay.next) and torch.equal(other.nextneg, lay.nextneg)
                        and torch.equal(other.drawn, lay.drawn))
                if not same:
                    bad.append(f'{name}: part {part}: the bits differ from the default part length')
            cut += int(M - 1 > 64)
        Y, _ = ur.epoch_gather(Y, st, n, N_EPOCHS, a, b, SEED)
    assert zero_edges > 0 and zero_negatives > 0 and cut > 0          # the cases the test is there for did occur
    assert not bad, '\n'.join(bad)


def test_epoch_bad_arguments(lib):
    M, dim = 10, 2
    y = torch.zeros(M, dim, device=dev())
    out = torch.full((M, dim), float('nan'), device=dev())
    indptr = torch.arange(M + 1, device=dev())
    indices = torch.arange(M, device=dev()).roll(1)
    eps = torch.ones(M, device=dev())
    nx, nn, dr = eps.clone(), eps / 5, torch.zeros(M, dtype=torch.int32, device=dev())
    ws = torch.empty(max(int(lib.ampconv_umap_epoch_workspace_bytes(M, M, dim)), 256), dtype=torch.uint8, device=dev())
    base = dict(y=y.data_ptr(), out=out.data_ptr(), M=M, dim=dim, indptr=indptr.data_ptr(), indices=indices.data_ptr(), nnz=M,
                eps=eps.data_ptr(), nx=nx.data_ptr(), nn=nn.data_ptr(), dr=dr.data_ptr(), epoch=1, part=64, ws=ws.data_ptr(), wsn=ws.numel())
    for name, change, want in (('y_in == y_out', dict(out=y.data_ptr()), BADARG), ('M = 0', dict(M=0), BADARG), ('dim = 1', dict(dim=1), BADARG),
                               ('dim = 33', dict(dim=33), BADARG), ('nnz < 0', dict(nnz=-1), BADARG), ('epoch < 0', dict(epoch=-1), BADARG),
                               ('part 32', dict(part=32), BADARG), ('part 100', dict(part=100), BADARG), ('NULL indptr', dict(indptr=None), BADARG),
                               ('NULL indices', dict(indices=None), BADARG), ('NULL eps', dict(eps=None), BADARG), ('NULL drawn', dict(dr=None), BADARG),
                               ('misaligned y', dict(y=y.data_ptr() + 4), BADARG), ('NULL workspace', dict(ws=None), EWORKSPACE),
                               ('short workspace', dict(wsn=8), EWORKSPACE)):
        a = dict(base)
        a.update(change)
        got = lib.ampconv_umap_epoch_split(a['y'], a['out'], a['M'], a['dim'], a['indptr'], a['indices'], a['nnz'], a['eps'], a['nx'],
                                           a['nn'], a['dr'], 1.5, 0.9, 1.0, 1.0, a['epoch'], 0, a['part'], a['ws'], a['wsn'], stream())
        assert got == want, name
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.equal(nx, eps) and not bool(dr.any())
    assert lib.ampconv_umap_epoch_workspace_bytes(0, 5, 2) == 0 == lib.ampconv_umap_epoch_workspace_bytes(5, 5, 33)


# ------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def clusters():
    from ampnet_amd import umap
    X, lab = ur.clusters_case()
    xd = to_dev(X)
    return dict(X=X, lab=lab, xd=xd, run=umap(xd, seed=0))


def test_end_to_end_against_the_model_run(clusters):
    """Two runs give the same bits, another seed other bits; the result keeps the 15 nearest neighbours no worse than the
    fp64 model's run on the same graph from the same start, less the spread of the model's own score over five seeds."""
    from ampnet_amd import pca, umap
    c, run = clusters, clusters['run']
    y = run.embedding.cpu().numpy()
    assert run.embedding.dtype == torch.float32 and y.shape == (300, 2) and np.isfinite(y).all() and run.n_epochs == 500
    assert run.a == pytest.approx(1.5769, abs=2e-4) and run.b == pytest.approx(0.8951, abs=2e-4)
    again, other = umap(c['xd'], seed=0), umap(c['xd'], seed=1)
    assert torch.equal(again.embedding, run.embedding) and all(torch.equal(p, q) for p, q in zip(again.graph, run.graph))
    assert not torch.equal(other.embedding, run.embedding) and torch.isfinite(other.embedding).all()
    scores = pca(c['xd'], 2).scores
    y0 = um.scaled_start(scores)
    assert torch.equal(umap(c['xd'], seed=0, init=scores).embedding, run.embedding)      # init='pca' is this tensor
    assert float(y0.min()) == 0 and float(y0.max()) == 10
    assert np.array_equal(y0.cpu().numpy(), ur.scaled_start_model(scores.cpu().numpy()))
    graph = [t.cpu().numpy() for t in run.graph]
    model, _ = ur.layout_model(y0.cpu().numpy(), *graph, run.a, run.b, 500, seed=0)
    start = ur.neighbor_preservation_model(c['X'], y0.cpu().numpy(), 15)
    ours, theirs = ur.neighbor_preservation_model(c['X'], y, 15), ur.neighbor_preservation_model(c['X'], model, 15)
    print(f'neighbor preservation: start {start:.3f}, kernels {ours:.3f}, model {theirs:.3f} (margin {NP_SPREAD})')
    assert ours >= theirs - NP_SPREAD and ours > start
    # the graph is the model's on exact neighbours (no neighbour decision of this case is within the fp32 distance bound)
    idx, dist = ur.neighbors_with_self(c['X'], 15)
    gi, gd = um.neighbors_with_self(c['xd'], 15)
    if np.array_equal(gi.cpu().numpy(), idx):
        _, ws, wr = ur.memberships_model(idx, gd.cpu().numpy())
        assert np.allclose(run.sigma.cpu().numpy(), ws, rtol=1e-12, atol=0) and np.allclose(run.rho.cpu().numpy(), wr, rtol=1e-12, atol=0)


def test_neighbors_argument_and_a_whole_layout_across_part_lengths():
    """umap(neighbors=(idx, dist)) on the hub case: the graph has the model's structure (row 0 holds M - 1 entries), the
    run is finite and repeatable, and a WHOLE layout of 30 epochs -- schedule state handed from epoch to epoch on the
    device -- gives the same bits at part lengths 64 (the hub is cut into five parts) and the library's."""
    from ampnet_amd import umap
    M = 300
    X, idx, dist = ur.hub_neighbors(M, 15, seed=M)
    xd, di, dd = to_dev(X), to_dev(idx), to_dev(dist)
    run = umap(xd, n_epochs=30, seed=4, neighbors=(di, dd))
    again = umap(xd, n_epochs=30, seed=4, neighbors=(di, dd), n_neighbors=7)      # the k of neighbors replaces n_neighbors
    indptr, indices, val = run.graph
    memb, _, _ = ur.memberships_model(idx, dist)
    wp, wi, wv = ur.fuzzy_model(idx, memb.astype(np.float32))
    assert np.array_equal(indptr.cpu().numpy(), wp) and np.array_equal(indices.cpu().numpy(), wi) and int(indptr[1]) == M - 1
    assert (ulps32(val.cpu().numpy(), wv) <= 8).all()                 # two memberships at 2 ulp each through (p + q) - p q
    assert torch.isfinite(run.embedding).all() and torch.equal(run.embedding, again.embedding)
    y0 = um.scaled_start(run.embedding)
    a, b = run.a, run.b
    outs = []
    for part in (None, 64):
        lay = um.Layout(y0, *um.schedule(indptr, indices, val, 30), a, b, 30, 4, part=part)
        for n in range(30):
            lay.epoch(n)
        outs.append((lay.y[0], lay.next, lay.nextneg, lay.drawn))
    assert all(torch.equal(p, q) for p, q in zip(*outs)) and int(outs[0][3].sum()) > 0


def test_columns_equal_rows_of_the_transpose():
    """samples='columns' on a [40, 64] matrix against samples='rows' on its materialised transpose: the same graph
    structure, and values within what the two distance evaluations allow.  Both are float32 evaluations of squared
    distances within B = (P + 4) 2^-24 2 max |x_s|^2 of the exact ones (P = 40 features: the bound of the t-SNE column
    fixture, tools/make_golden_tsne.py), so a distance moves by at most dd = 2 B / (2 d_min).  A membership
    w = exp(-x), x = (d - rho) / sigma, moves by at most w |dx| <= 2 dd / sigma + x exp(-x) |d ln sigma|, where the two
    searches stop within 1e-5 of the same target on sums whose terms moved by at most 2 dd / sigma each:
    |d ln sigma| <= (2e-5 + 2 k dd / sigma) / sum_j x_j exp(-x_j), and x exp(-x) <= 1 / e.  An entry of W moves by at
    most the sum of its two memberships' moves."""
    from ampnet_amd import umap
    rng = np.random.default_rng(4)
    x = rng.normal(0.0, 1.0, (40, 64)).astype(np.float32)
    xd = to_dev(x)
    kw = dict(n_neighbors=10, n_epochs=20, seed=2)
    cols = umap(xd, samples='columns', **kw)
    rows = umap(xd.t().contiguous(), samples='rows', **kw)
    assert cols.embedding.shape == (64, 2) and torch.isfinite(cols.embedding).all()
    assert torch.equal(cols.graph[0], rows.graph[0]) and torch.equal(cols.graph[1], rows.graph[1])
    X = x.T.astype(np.float64)
    B = (40 + 4) * 2.0 ** -24 * 2.0 * (X * X).sum(1).max()
    idx, dist = ur.neighbors_with_self(X, 10)
    sigma, rho, _, floored = ur.smooth_knn(dist)
    assert not floored.any()
    dd = 2.0 * B / (2.0 * dist[:, 1].astype(np.float64).min())
    xs = (dist[:, 1:].astype(np.float64) - rho[:, None]) / sigma[:, None]
    dln = (2e-5 + 2.0 * 10 * dd / sigma.min()) / (xs * np.exp(-xs)).sum(1).min()
    tol = 2.0 * (2.0 * dd / sigma.min() + dln / np.e)
    diff = (cols.graph[2].double() - rows.graph[2].double()).abs().max().item()
    print(f'columns against rows: largest difference of an entry {diff:.3e}, allowed {tol:.3e}')
    assert diff <= tol
    assert np.allclose(cols.sigma.cpu().numpy(), sigma, rtol=0.0, atol=sigma.max() * dln * 2) and np.allclose(rows.rho.cpu().numpy(), rho, atol=dd)


# ------------------------------------------------------------------------------------------------------ model hook
def test_model_hook_fills_and_freezes_the_table():
    from ampnet_amd import AMPGCN, umap
    torch.manual_seed(0)
    N, F = 48, 36
    x = torch.randn(N, F, device=dev())
    want = umap(x, 30, samples='columns').embedding
    assert want.shape == (F, 30) and torch.isfinite(want).all()
    for freeze in (True, False):
        model = AMPGCN(device=dev(), embedding_dim=31, num_heads=1, num_node_features=F, num_sampled_vectors=4, output_dim=3,
                       feat_emb_dim=30, dropout_rate=0.0, dropout_adj_rate=0.0).to(dev())
        res = model.init_feature_table_from_umap(x, freeze=freeze)
        assert torch.equal(res.embedding, want) and torch.equal(model.feature_embedding_table.weight, want)
        assert model.feature_embedding_table.weight.requires_grad == (not freeze)
    short = model.init_feature_table_from_umap(x, freeze=True, n_epochs=5, n_neighbors=5, seed=3)
    assert short.n_epochs == 5 and torch.equal(model.feature_embedding_table.weight, short.embedding)
    assert torch.equal(short.embedding, umap(x, 30, samples='columns', n_epochs=5, n_neighbors=5, seed=3).embedding)
    with pytest.raises(ValueError):
        model.init_feature_table_from_umap(x[:, :5])
    with pytest.raises(ValueError):
        model.init_feature_table_from_umap(x, samples='rows')


# ------------------------------------------------------------------------------------------------------ validation
def test_rejected_arguments_raise_before_any_launch(monkeypatch):
    from ampnet_amd import umap
    x = torch.randn(30, 6, device=dev())

    def launched(*a, **k):
        raise AssertionError('a stage ran before the arguments were checked')

    for name in ('neighbors_with_self', 'memberships', 'fuzzy_graph', 'pca', 'scaled_start'):
        monkeypatch.setattr(um, name, launched)
    good_idx, good_dist = torch.zeros(30, 5, dtype=torch.int64, device=dev()), torch.zeros(30, 5, device=dev())
    for kw in (dict(n_neighbors=1), dict(n_neighbors=31), dict(n_neighbors=257), dict(n_components=1), dict(n_components=33),
               dict(n_components=7), dict(min_dist=1.5), dict(min_dist=2.5, spread=2.0), dict(spread=-1.0), dict(n_epochs=0),
               dict(n_epochs=2.5), dict(init='spectral'), dict(init=torch.zeros(30, 3, device=dev())), dict(init=torch.zeros(30, 2)),
               dict(init=torch.zeros(30, 2, dtype=torch.float64, device=dev())), dict(samples='both'), dict(seed='x'), dict(a=1.0),
               dict(b=0.5), dict(a=0.0, b=1.0), dict(neighbors=(good_idx, good_dist.cpu())), dict(neighbors=(good_idx[:, :1], good_dist[:, :1])),
               dict(neighbors=(good_idx.int(), good_dist)), dict(neighbors=(good_idx[:20], good_dist[:20])), dict(neighbors=good_idx)):
        with pytest.raises(ValueError):
            umap(x, **kw)
    for bad_x in (x.cpu(), x.double(), x[:1], x.clone().requires_grad_(True), torch.randn(30, 300, device=dev()), x[0]):
        with pytest.raises(ValueError):
            umap(bad_x)
    x256 = torch.randn(300, 4, device=dev())
    with pytest.raises(ValueError):
        umap(x256, n_neighbors=257)
