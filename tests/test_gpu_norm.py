"""The per-token LayerNorm sites (csrc/norm.hip behind ampnet_amd/norm.py) on the GPU against the numpy model of
tests/norm_reference.py, against torch autograd, and inside AMPGCN(layer_norm=True) against a twin built from
nn.LayerNorm's functional form.

Shapes (N, L, D): (5, 3, 4) fewer tokens than one wave's groups, a one-piece row; (257, 40, 100) 25 pieces in a 32-lane
group (masked lanes), a ragged last workgroup; (64, 20, 128) whole pieces, no masked lanes; (33, 1, 768) several pieces
per lane, one token per node; (3, 2, 1024) the widest row; (64, 2, 3) the element-wise path.  fp32 everywhere, bf16
where D % 8 == 0.  Every other (G, K, U) of norm.hip, the grid stride and the slot counts are on the ladders of
tests/test_gpu_norm_kernels.py.
Tolerances: y, pooled, dx at the project's flat atol 1e-5, rtol 1e-4; the weight and bias gradients (sums over all
tokens) under labels that name a parameter gradient, i.e. atol scaled by their magnitude; bf16 storage atol 2e-2,
rtol 2e-2."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_reference as glue
import norm_reference as ref
from conftest import assert_close_scaled, load_golden, model_files

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 4), (257, 40, 100), (64, 20, 128), (33, 1, 768), (3, 2, 1024), (64, 2, 3)]
CASES = [(s, 'f32') for s in SHAPES] + [(s, 'bf16') for s in SHAPES if s[2] % 8 == 0]
CASE_IDS = [f'N{s[0]}_L{s[1]}_D{s[2]}_{d}' for s, d in CASES]
ACTS = ['identity', 'relu', 'elu']
POOLINGS = ['mean', 'token0']
PS = [0.0, 0.1, 0.6]
SEED = 0x1234567890ABCDEF
EPS = 1e-5
TOL = {'f32': {}, 'bf16': dict(atol=2e-2, rtol=2e-2)}
TORCH_ACT = {'identity': lambda t: t, 'relu': F.relu, 'elu': F.elu}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """x [N, L * D], dy of that shape, dpooled [N, D] in the storage dtype (free of exact zeros), weight and bias [D]
    float32, both away from 1 and 0 and bias away from zero.  Drawn once per case; never modified."""
    N, L, D = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * L + D)
    tdt = torch.bfloat16 if dtype == 'bf16' else torch.float32

    def draw(*size):
        t = torch.randn(*size, generator=g)
        t = torch.where(t.abs() < 1e-3, torch.full_like(t, 0.5), t).to(tdt)
        assert (t != 0).all()
        return t
    x, dy, dpooled = draw(N, L * D), draw(N, L * D), draw(N, D)
    weight = 1 + 0.5 * torch.randn(D, generator=g)
    bias = 0.5 * torch.randn(D, generator=g)
    bias = torch.where(bias.abs() < 0.05, torch.full_like(bias, 0.25), bias)
    return x, dy, dpooled, weight, bias


def _np(t):
    return t.detach().float().cpu().numpy()


def _leaves(dev, *tensors):
    return [t.to(dev).requires_grad_(True) for t in tensors]


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_norm_act_dropout_matches_the_reference_model(case, dev):
    from ampnet_amd import norm_act_dropout
    shape, dtype = case
    N, L, D = shape
    x, dy, _, w, b = _inputs(shape, dtype)
    for p in PS:
        thr, _ = glue.mask_params(p)
        keep = glue.keep_mask(SEED, thr, x.shape)
        for a in ACTS:
            xg, wg, bg = _leaves(dev, x, w, b)
            y = norm_act_dropout(xg, D, wg, bg, EPS, p, a, seed=SEED)
            assert y.dtype == x.dtype and y.shape == x.shape
            y.backward(dy.to(dev))
            want_y, _ = ref.norm_fwd(_np(x), D, _np(w), _np(b), EPS, a, SEED, p)
            want_dx, want_dw, want_db = ref.norm_bwd(_np(x), _np(dy), D, _np(w), _np(b), EPS, a, SEED, p)
            label = f'{a} p={p}'
            assert_close_scaled(_np(y), want_y, 'y ' + label, **TOL[dtype])
            assert_close_scaled(_np(xg.grad), want_dx, 'dx ' + label, **TOL[dtype])
            assert_close_scaled(_np(wg.grad), want_dw, 'weight.grad ' + label, **TOL[dtype])
            assert_close_scaled(_np(bg.grad), want_db, 'bias.grad ' + label, **TOL[dtype])
            if a == 'identity' and p > 0:                        # z = xhat w + b is never exactly 0: the zeros ARE the mask
                assert np.array_equal(_np(y) != 0, keep), label
    x3 = x.view(N, L, D).to(dev)                                  # [N, L, D] in, [N, L, D] out, the same bits
    assert torch.equal(norm_act_dropout(x3, D, w.to(dev), b.to(dev), EPS, 0.1, 'elu', seed=SEED).view(N, L * D),
                       norm_act_dropout(x.to(dev), D, w.to(dev), b.to(dev), EPS, 0.1, 'elu', seed=SEED))


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_norm_pool_matches_the_reference_model(case, dev):
    from ampnet_amd import norm_act_dropout_pool
    shape, dtype = case
    N, L, D = shape
    x, _, dpooled, w, b = _inputs(shape, dtype)
    for p in PS:
        for a in ACTS:
            for pooling in POOLINGS:
                xg, wg, bg = _leaves(dev, x, w, b)
                out = norm_act_dropout_pool(xg, D, wg, bg, EPS, p, a, pooling, seed=SEED)
                assert out.dtype == x.dtype and out.shape == (N, D)
                out.backward(dpooled.to(dev))
                args = (L, D, _np(w), _np(b), EPS, a, pooling, SEED, p)
                want, _ = ref.norm_pool_fwd(_np(x), *args)
                want_dx, want_dw, want_db = ref.norm_pool_bwd(_np(x), _np(dpooled), *args)
                label = f'{a} {pooling} p={p}'
                assert_close_scaled(_np(out), want, 'pooled ' + label, **TOL[dtype])
                assert_close_scaled(_np(xg.grad), want_dx, 'dx ' + label, **TOL[dtype])
                assert_close_scaled(_np(wg.grad), want_dw, 'weight.grad ' + label, **TOL[dtype])
                assert_close_scaled(_np(bg.grad), want_db, 'bias.grad ' + label, **TOL[dtype])


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_against_torch_autograd_without_dropout(case, dev):
    from ampnet_amd import norm_act_dropout, norm_act_dropout_pool
    shape, dtype = case
    N, L, D = shape
    x, dy, dpooled, w, b = _inputs(shape, dtype)
    for affine in (True, False):
        for a in ACTS:
            def torch_site(xt, wt, bt):                          # torch's composite in fp32 on the same stored values
                return TORCH_ACT[a](F.layer_norm(xt.view(N, L, D), (D,), wt, bt, EPS))

            def leaves():
                return _leaves(dev, x, w, b) if affine else _leaves(dev, x) + [None, None]

            xt, wt, bt = leaves()
            xt32 = xt.float()
            xt32.retain_grad()
            want = torch_site(xt32, wt, bt).view(N, L * D)
            want.backward(dy.to(dev).float())
            xg, wg, bg = leaves()
            y = norm_act_dropout(xg, D, wg, bg, EPS, 0.0, a)
            y.backward(dy.to(dev))
            label = f'{a} affine={affine}'
            assert_close_scaled(_np(y), _np(want), 'y ' + label, **TOL[dtype])
            assert_close_scaled(_np(xg.grad), _np(xt32.grad), 'dx ' + label, **TOL[dtype])
            if affine:
                assert_close_scaled(_np(wg.grad), _np(wt.grad), 'weight.grad ' + label, **TOL[dtype])
                assert_close_scaled(_np(bg.grad), _np(bt.grad), 'bias.grad ' + label, **TOL[dtype])
            for pooling in POOLINGS:
                xt, wt, bt = leaves()
                xt32 = xt.float()
                xt32.retain_grad()
                h = torch_site(xt32, wt, bt)
                want = h.mean(dim=1) if pooling == 'mean' else h[:, 0]
                want.backward(dpooled.to(dev).float())
                xg, wg, bg = leaves()
                out = norm_act_dropout_pool(xg, D, wg, bg, EPS, 0.0, a, pooling)
                out.backward(dpooled.to(dev))
                label = f'{a} {pooling} affine={affine}'
                assert_close_scaled(_np(out), _np(want), 'pooled ' + label, **TOL[dtype])
                assert_close_scaled(_np(xg.grad), _np(xt32.grad), 'dx pooled ' + label, **TOL[dtype])
                if affine:
                    assert_close_scaled(_np(wg.grad), _np(wt.grad), 'weight.grad pooled ' + label, **TOL[dtype])
                    assert_close_scaled(_np(bg.grad), _np(bt.grad), 'bias.grad pooled ' + label, **TOL[dtype])


def _library_call(lib, fn, *args):
    rc = getattr(lib, fn)(*args)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_statistics_match_the_fp64_model(case, dev):
    """stats = (mean, 1 / sqrt(var + eps)) straight from the library, for the plain and both pooled calls."""
    from ampnet_amd import _lib
    lib = _lib.load()
    shape, dtype = case
    N, L, D = shape
    x = _inputs(shape, dtype)[0].to(dev)
    code = _lib.AMPCONV_BF16 if dtype == 'bf16' else _lib.AMPCONV_F32
    mu, rstd, _ = ref.token_stats(_np(x), D, EPS)
    want = np.stack([mu, rstd], axis=1)
    # rtol 1e-5; the mean of a token can be arbitrarily close to zero, so it also gets the absolute rounding error of an
    # fp32 sum: every addition rounds at 2^-24 of a partial sum <= sum |x|, and no value passes through more than
    # 16 (in the lane) + 6 (butterfly) of them
    mu_atol = 22 * 2.0 ** -24 * np.abs(_np(x).reshape(-1, D)).mean(axis=1)

    def check(got, rows):
        got = _np(got).astype(np.float64)
        err = np.abs(got - want[rows])
        assert (err[:, 0] <= 1e-5 * np.abs(want[rows, 0]) + mu_atol[rows]).all(), float(err[:, 0].max())
        np.testing.assert_allclose(got[:, 1], want[rows, 1], rtol=1e-5, atol=0)

    every, first = np.arange(N * L), np.arange(N) * L
    y, pooled = torch.empty_like(x), torch.empty(N, D, dtype=x.dtype, device=dev)
    stats = torch.full((N * L, 2), float('nan'), device=dev)
    assert _library_call(lib, 'ampconv_norm_fwd', x.data_ptr(), N * L, D, None, None, EPS, 0, 0, 0, 1.0, y.data_ptr(),
                         stats.data_ptr(), code, None) == 0
    check(stats, every)
    stats.fill_(float('nan'))
    assert _library_call(lib, 'ampconv_norm_pool_fwd', x.data_ptr(), N, L, D, None, None, EPS, 0, 0, 0, 0, 1.0,
                         pooled.data_ptr(), stats.data_ptr(), code, None) == 0
    check(stats, every)
    stats.fill_(float('nan'))
    assert _library_call(lib, 'ampconv_norm_pool_fwd', x.data_ptr(), N, L, D, None, None, EPS, 0, 1, 0, 0, 1.0,
                         pooled.data_ptr(), stats.data_ptr(), code, None) == 0
    check(stats[:N], first)
    assert L == 1 or bool(torch.isnan(stats[N:]).all())          # token 0: [N, 2] and not a byte more


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_constant_rows(dtype, dev):
    """Every token constant 0.5: all sums are exact, var = 0, xhat = 0, so y = act(bias); dx stays finite."""
    from ampnet_amd import norm_act_dropout, norm_act_dropout_pool
    N, L, D = 4, 2, 128
    _, dy, dpooled, w, b = _inputs((64, 20, 128), dtype)
    x = torch.full((N, L * D), 0.5, dtype=dy.dtype)
    for a in ACTS:
        want = glue.act(np.broadcast_to(_np(b), (N * L, D)), a).reshape(N, L * D)
        xg, wg, bg = _leaves(dev, x, w, b)
        y = norm_act_dropout(xg, D, wg, bg, EPS, 0.0, a)
        y.backward(dy[:N, :L * D].to(dev))
        assert_close_scaled(_np(y), want, f'y {a}', **TOL[dtype])
        assert torch.isfinite(xg.grad).all() and torch.isfinite(wg.grad).all() and torch.isfinite(bg.grad).all()
        for pooling in POOLINGS:
            xg, wg, bg = _leaves(dev, x, w, b)
            out = norm_act_dropout_pool(xg, D, wg, bg, EPS, 0.0, a, pooling)
            out.backward(dpooled[:N].to(dev))
            assert_close_scaled(_np(out), want[:, :D], f'pooled {a} {pooling}', **TOL[dtype])
            assert torch.isfinite(xg.grad).all()


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_token0_pooling_touches_token_0_only(case, dev):
    from ampnet_amd import norm_act_dropout_pool
    shape, dtype = case
    N, L, D = shape
    x, _, dpooled, w, b = _inputs(shape, dtype)
    xg, wg, bg = _leaves(dev, x, w, b)
    norm_act_dropout_pool(xg, D, wg, bg, EPS, 0.1, 'elu', 'token0', seed=SEED).backward(dpooled.to(dev))
    tail = xg.grad.view(N, L, D)[:, 1:]
    assert tail.numel() == 0 or bool((tail.contiguous().view(torch.int16 if dtype == 'bf16' else torch.int32) == 0).all())
    # the same call on the first tokens alone -- without dropout, whose mask follows the flat index in the full tensor
    xg, wg, bg = _leaves(dev, x, w, b)
    norm_act_dropout_pool(xg, D, wg, bg, EPS, 0.0, 'elu', 'token0').backward(dpooled.to(dev))
    x0, w0, b0 = _leaves(dev, x.view(N, L, D)[:, :1].contiguous(), w, b)
    norm_act_dropout_pool(x0, D, w0, b0, EPS, 0.0, 'elu', 'token0').backward(dpooled.to(dev))
    assert torch.equal(xg.grad.view(N, L, D)[:, :1], x0.grad)
    assert_close_scaled(_np(wg.grad), _np(w0.grad), 'weight.grad token0', **TOL[dtype])
    assert_close_scaled(_np(bg.grad), _np(b0.grad), 'bias.grad token0', **TOL[dtype])


@pytest.mark.parametrize('shape', [(1750, 40, 100), (257, 40, 100)], ids=['N1750', 'N257'])
def test_same_bits_on_every_launch(shape, dev):
    """(1750, 40, 100): more token steps than the grid has groups, so a workgroup sums several of them."""
    from ampnet_amd import norm_act_dropout, norm_act_dropout_pool
    N, L, D = shape
    g = torch.Generator().manual_seed(N)
    x, dy, dpooled = torch.randn(N, L * D, generator=g), torch.randn(N, L * D, generator=g), torch.randn(N, D, generator=g)
    w, b = _inputs((257, 40, 100), 'f32')[3:]

    def run(fn, grad):
        xg, wg, bg = _leaves(dev, x, w, b)
        out = fn(xg, wg, bg)
        out.backward(grad.to(dev))
        return out.detach(), xg.grad, wg.grad, bg.grad

    for fn, grad in ((lambda xg, wg, bg: norm_act_dropout(xg, D, wg, bg, EPS, 0.1, 'elu', seed=SEED), dy),
                     (lambda xg, wg, bg: norm_act_dropout_pool(xg, D, wg, bg, EPS, 0.1, 'elu', 'mean', seed=SEED), dpooled)):
        first, second = run(fn, grad), run(fn, grad)
        for a, c, name in zip(first, second, ('output', 'dx', 'weight.grad', 'bias.grad')):
            assert torch.equal(a, c), name
    assert not torch.equal(norm_act_dropout(x.to(dev), D, p=0.1, seed=SEED), norm_act_dropout(x.to(dev), D, p=0.1, seed=SEED + 1))


def test_library_rejects_bad_arguments(dev):
    from ampnet_amd import _lib
    lib = _lib.load()
    T, D = 8, 16
    x = torch.ones(T * D, device=dev)
    y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    stats, dw, db = torch.full((T, 2), 7.0, device=dev), torch.full((D,), 7.0, device=dev), torch.full((D,), 7.0, device=dev)
    w, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    need = lib.ampconv_norm_workspace_bytes(T, D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    X, Y, S, DX, W, B, DW, DB, WS = (t.data_ptr() for t in (x, y, stats, dx, w, b, dw, db, ws))

    def fwd(T=T, D=D, eps=EPS, act=1, thr=0, dtype=0):
        return lib.ampconv_norm_fwd(X, T, D, W, B, eps, act, 0, thr, 1.0, Y, S, dtype, None)

    def bwd(T=T, D=D, act=1, thr=0, dtype=0, ws_bytes=need, dw=DW, db=DB, w=W, b=B):
        return lib.ampconv_norm_bwd(X, Y, S, T, D, w, b, act, 0, thr, 1.0, DX, dw, db, WS, ws_bytes, dtype, None)

    def pool_fwd(N=4, L=2, D=D, eps=EPS, pooling=0, thr=0, dtype=0):
        return lib.ampconv_norm_pool_fwd(X, N, L, D, W, B, eps, 1, pooling, 0, thr, 1.0, Y, S, dtype, None)

    def pool_bwd(N=4, L=2, D=D, pooling=0, thr=0, dtype=0, ws_bytes=need):
        return lib.ampconv_norm_pool_bwd(X, Y, S, N, L, D, W, B, 1, pooling, 0, thr, 1.0, DX, DW, DB, WS, ws_bytes, dtype, None)

    for call in (fwd, bwd, pool_fwd, pool_bwd):
        assert call(D=0) == -1 and call(D=1025) == -1
        assert call(thr=65536) == -1
        assert call(dtype=7) == -2
    assert fwd(eps=0.0) == -1 and pool_fwd(eps=0.0) == -1 and fwd(eps=-1.0) == -1
    assert pool_fwd(L=0) == -1 and pool_bwd(L=0) == -1
    assert fwd(T=-1) == -1 and pool_fwd(N=-1) == -1
    assert fwd(act=3) == -1 and bwd(act=-1) == -1
    assert pool_fwd(pooling=2) == -1 and pool_bwd(pooling=2) == -1
    assert bwd(ws_bytes=need - 1) == -3 and pool_bwd(ws_bytes=need - 1) == -3
    assert bwd(w=None, b=None) == -1                             # gradients for a weight that is not there
    assert bwd(b=None) == -1                                     # weight without bias
    torch.cuda.synchronize()
    for t in (y, dx, stats, dw, db):                             # nothing was launched
        assert bool((t == 7.0).all())
    assert lib.ampconv_norm_workspace_bytes(0, D) == 0
    assert bwd(T=0, ws_bytes=0) == 0                             # no tokens: dgamma = dbeta = 0, nothing else written
    torch.cuda.synchronize()
    assert bool((dw == 0).all()) and bool((db == 0).all()) and bool((dx == 7.0).all())
    assert fwd() == 0 and bwd() == 0 and bwd(ws_bytes=0, dw=None, db=None) == 0
    torch.cuda.synchronize()


def test_modules_draw_their_own_seed_stream(dev):
    from ampnet_amd import NormTokenReadout, TokenLayerNorm, norm_act_dropout, norm_act_dropout_pool
    N, L, D = 64, 20, 128
    x = _inputs((N, L, D), 'f32')[0].to(dev)
    site, readout = TokenLayerNorm(D, p=0.6, activation='relu', seed=5).to(dev), NormTokenReadout(D, p=0.6, seed=5).to(dev)
    site.eval(), readout.eval()
    assert torch.equal(site(x), norm_act_dropout(x, D, site.weight, site.bias, activation='relu')) and site.last_seed is None
    assert torch.equal(readout(x), norm_act_dropout_pool(x, D, readout.weight, readout.bias))
    site.train()
    y1, s1 = site(x), site.last_seed
    y2, s2 = site(x), site.last_seed
    assert s1 != s2 and not torch.equal(y1, y2)
    assert torch.equal(y1, norm_act_dropout(x, D, site.weight, site.bias, p=0.6, activation='relu', seed=s1))
    plain = TokenLayerNorm(D, elementwise_affine=False).to(dev)
    assert_close_scaled(_np(plain(x)), _np(F.layer_norm(x.view(N, L, D), (D,)).view(N, -1)), 'y without weight and bias')


# ---- the whole model ---------------------------------------------------------------------------------------------------
MODEL = dict(embedding_dim=128, num_heads=4, num_sampled_vectors=20, feat_emb_dim=127, num_node_features=50, output_dim=7)


@functools.lru_cache(maxsize=None)
def _graph():
    g = torch.Generator().manual_seed(7)
    N, E, Fdim = 200, 800, MODEL['num_node_features']
    return (torch.randn(N, Fdim, generator=g), torch.randint(0, N, (2, E), generator=g),
            torch.randint(0, Fdim, (N, MODEL['num_sampled_vectors']), generator=g, dtype=torch.int32),
            torch.randn(N, MODEL['output_dim'], generator=g), torch.randint(0, MODEL['output_dim'], (N,), generator=g))


def _model(dev, **flags):
    from ampnet_amd import AMPGCN
    torch.manual_seed(11)
    model = AMPGCN(device=dev, layer_norm=True, dropout_adj_rate=0.0, **MODEL, **flags).to(dev)
    g = torch.Generator().manual_seed(13)
    with torch.no_grad():
        for norm in (model.norm1, model.norm2):                  # away from nn.LayerNorm's 1 and 0
            norm.weight.add_(0.3 * torch.randn(norm.weight.shape, generator=g).to(dev))
            norm.bias.add_(0.3 * torch.randn(norm.bias.shape, generator=g).to(dev))
    model.train()
    x, ei, idx, dlogits, labels = (t.to(dev) for t in _graph())
    return model, types.SimpleNamespace(x=x, edge_index=ei), idx, dlogits, labels


def _twin_logits(model, data, idx, masks=(None, None, None)):
    """The same AMPConv layers and parameters around nn.LayerNorm's functional form, ReLU, the token mean, the Linear and
    log_softmax; masks: the three dropout sites' keep * scale tensors (None: no dropout)."""
    D = model.emb_dim

    def drop(t, m):
        return t if m is None else t * m

    x, _ = model._tokens[0](data.x, idx)
    N = x.size(0)
    h1 = model.conv1(drop(x, masks[0]), data.edge_index)
    z = F.relu(F.layer_norm(h1.view(N, -1, D), (D,), model.norm1.weight, model.norm1.bias, model.norm1.eps)).view(N, -1)
    h2 = model.conv2(drop(z, masks[1]), data.edge_index)
    z = F.relu(F.layer_norm(h2.view(N, -1, D), (D,), model.norm2.weight, model.norm2.bias, model.norm2.eps)).view(N, -1)
    pooled = drop(z, masks[2]).view(N, -1, D).mean(dim=1)
    return F.log_softmax(model.final_linear_out(pooled), dim=1), h1, h2


def _grads(model):
    grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    return grads


def _compare_with_twin(model, data, idx, dlogits, logits, masks=(None, None, None)):
    emb1, emb2 = model.conv1_embedding.detach(), model.conv2_embedding.detach()
    (logits * dlogits).sum().backward()
    got = _grads(model)
    want_logits, h1, h2 = _twin_logits(model, data, idx, masks)
    (want_logits * dlogits).sum().backward()
    want = _grads(model)
    assert_close_scaled(_np(logits), _np(want_logits), 'logits')
    assert_close_scaled(_np(emb1), _np(h1), 'conv1_embedding')
    assert_close_scaled(_np(emb2), _np(h2), 'conv2_embedding')
    assert set(got) == set(want) and {'norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias'} <= set(got)
    for name in want:
        assert_close_scaled(_np(got[name]), _np(want[name]), name + '.grad')


@pytest.mark.parametrize('fused_head', [False, True], ids=['head_torch', 'head_fused'])
@pytest.mark.parametrize('fused_glue', [False, True], ids=['glue_torch', 'glue_fused'])
def test_model_without_dropout_matches_the_layer_norm_twin(fused_glue, fused_head, dev):
    model, data, idx, dlogits, _ = _model(dev, dropout_rate=0.0, fused_glue=fused_glue, fused_head=fused_head)
    _compare_with_twin(model, data, idx, dlogits, model(data, feature_indices=idx))


def test_model_nll_loss_matches_the_layer_norm_twin(dev):
    model, data, idx, _, labels = _model(dev, dropout_rate=0.0, fused_glue=True, fused_head=True)
    loss = model.nll_loss(data, y=labels, feature_indices=idx)
    loss.backward()
    got = _grads(model)
    want_loss = F.nll_loss(_twin_logits(model, data, idx)[0], labels, reduction='sum')
    want_loss.backward()
    want = _grads(model)
    assert_close_scaled(_np(loss), _np(want_loss), 'loss', scaled=True)       # a sum over the 200 nodes
    assert set(got) == set(want)
    for name in want:
        assert_close_scaled(_np(got[name]), _np(want[name]), name + '.grad')


def test_model_with_dropout_matches_the_twin_under_its_masks(dev):
    model, data, idx, dlogits, _ = _model(dev, dropout_rate=0.1, fused_glue=True)
    logits = model(data, feature_indices=idx)
    sites = [model._glue[0], model.norm1, model.norm2]
    seeds = [s.last_seed for s in sites]
    assert all(s is not None for s in seeds) and len(set(seeds)) == 3
    thr, scale = glue.mask_params(0.1)
    shape = tuple(model.conv1_embedding.shape)
    masks = [torch.from_numpy(glue.keep_mask(s, thr, shape)).to(dev).float() * float(scale) for s in seeds]
    assert all(0.85 < float((m != 0).float().mean()) < 0.95 for m in masks)
    _compare_with_twin(model, data, idx, dlogits, logits, masks)


def test_default_model_is_unchanged(dev):
    """AMPGCN() and AMPGCN(layer_norm=False) on a reference fixture: the same module tree and the same logits bitwise
    (torch's random stream re-seeded: the default glue draws its dropout masks from it)."""
    from ampnet_amd import AMPGCN
    import test_gpu_glue as glue_tests
    g = load_golden([p for p in model_files() if p.endswith('model_cora.npz')][0])
    outs = []
    for override in ({}, {'layer_norm': False}):
        model, data, idx = glue_tests._load_model(g, dev, **override)
        assert [n for n, _ in model.named_modules() if n.startswith('norm')] == []
        torch.manual_seed(3)
        outs.append(model(data, feature_indices=idx).detach())
    assert torch.equal(outs[0], outs[1])
    assert AMPGCN(device=dev).layer_norm is False
