"""The fused glue kernels (csrc/glue.hip behind ampnet_amd/glue.py) on the GPU against the numpy model of
tests/glue_reference.py, against torch autograd, and inside the whole model against the reference's fixtures.

Shapes (N, L, D): (5, 3, 4) fewer rows than waves and a row shorter than one wave's span; (257, 40, 100) a ragged last
workgroup, 1000 16-byte pieces per row; (64, 20, 128); (33, 1, 128) a single token; (64, 2, 3) the XOR toy's rows, which
no 16-byte piece divides (element-wise kernels).  fp32 everywhere, bf16 where D % 8 == 0.  The launch paths these shapes do
not reach (grid stride, tile and unroll remainders, unaligned bases) are on the ladders of tests/test_gpu_glue_kernels.py.
Tolerances: fp32 the project's flat atol 1e-5, rtol 1e-4; bf16 storage atol 2e-2, rtol 2e-2 (tests/test_gpu_parity.py,
test_bf16_storage)."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_reference as ref
from conftest import assert_close_scaled, load_golden, model_files

pytestmark = pytest.mark.gpu

SHAPES = [(5, 3, 4), (257, 40, 100), (64, 20, 128), (33, 1, 128), (64, 2, 3)]
CASES = [(s, 'f32') for s in SHAPES] + [(s, 'bf16') for s in SHAPES if s[2] % 8 == 0]
CASE_IDS = [f'N{s[0]}_L{s[1]}_D{s[2]}_{d}' for s, d in CASES]
ACTS = ['identity', 'relu', 'elu']
PS = [0.0, 0.1, 0.6]
SEED = 0x1234567890ABCDEF
TOL = {'f32': {}, 'bf16': dict(atol=2e-2, rtol=2e-2)}
TORCH_ACT = {'identity': lambda t: t, 'relu': F.relu, 'elu': F.elu}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """x [N, L * D], dy of the same shape, dpooled [N, D]: seeded, free of exact zeros, already rounded to the storage
    dtype (float32 arrays hold the exact values the device sees).  Shared by every test of a case; never modified."""
    N, L, D = shape
    g = torch.Generator().manual_seed(1000 * N + 10 * L + D)
    tdt = torch.bfloat16 if dtype == 'bf16' else torch.float32

    def draw(*size):
        t = torch.randn(*size, generator=g)
        t = torch.where(t.abs() < 1e-3, torch.full_like(t, 0.5), t).to(tdt)
        assert (t != 0).all()
        return t
    return draw(N, L * D), draw(N, L * D), draw(N, D)


def _np(t):
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_act_dropout_matches_the_reference_model(case, dev):
    from ampnet_amd import act_dropout
    shape, dtype = case
    x, dy, _ = _inputs(shape, dtype)
    for p in PS:
        thr, _ = ref.mask_params(p)
        keep = ref.keep_mask(SEED, thr, x.shape)
        for a in ACTS:
            xg = x.to(dev).requires_grad_(True)
            y = act_dropout(xg, p, a, seed=SEED)
            assert y.dtype == x.dtype and y.shape == x.shape
            if a == 'identity':                                  # inputs hold no zero: the zero pattern IS the mask
                assert np.array_equal(_np(y) != 0, keep), (p, a)
                if p == 0:
                    assert y is xg                               # nothing to do: no launch, no copy
            y.backward(dy.to(dev))
            assert_close_scaled(_np(y), ref.act_dropout_fwd(_np(x), a, SEED, p), f'y {a} p={p}', **TOL[dtype])
            want_dx = ref.act_dropout_bwd(_np(x), _np(dy), a, SEED, p)
            assert_close_scaled(_np(xg.grad), want_dx, f'dx {a} p={p}', **TOL[dtype])
            assert np.array_equal(_np(xg.grad) != 0, want_dx != 0), (p, a)


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_pool_matches_the_reference_model(case, dev):
    from ampnet_amd import act_dropout_pool
    shape, dtype = case
    N, L, D = shape
    x, _, dpooled = _inputs(shape, dtype)
    for p in PS:
        for a in ACTS:
            for pooling in ('mean', 'token0'):
                xg = x.to(dev).requires_grad_(True)
                out = act_dropout_pool(xg, D, p, a, pooling, seed=SEED)
                assert out.dtype == x.dtype and out.shape == (N, D)
                out.backward(dpooled.to(dev))
                label = f'{a} {pooling} p={p}'
                assert_close_scaled(_np(out), ref.pool_fwd(_np(x), L, D, a, pooling, SEED, p), 'pooled ' + label, **TOL[dtype])
                assert_close_scaled(_np(xg.grad), ref.pool_bwd(_np(x), _np(dpooled), L, D, a, pooling, SEED, p), 'dx ' + label,
                                    **TOL[dtype])
                if pooling == 'token0':                          # rows behind token 0: exact zeros, written by the kernel
                    tail = xg.grad.view(N, L, D)[:, 1:]
                    assert tail.numel() == 0 or bool((tail.view(torch.int16 if dtype == 'bf16' else torch.int32) == 0).all())


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_against_torch_autograd_without_dropout(case, dev):
    from ampnet_amd import act_dropout, act_dropout_pool
    shape, dtype = case
    N, L, D = shape
    x, dy, dpooled = _inputs(shape, dtype)
    for a in ('relu', 'elu'):
        xt = x.to(dev).float().requires_grad_(True)              # torch's composite in fp32 on the same stored values
        TORCH_ACT[a](xt).backward(dy.to(dev).float())
        xg = x.to(dev).requires_grad_(True)
        y = act_dropout(xg, 0.0, a)
        y.backward(dy.to(dev))
        assert_close_scaled(_np(y), _np(TORCH_ACT[a](xt)), f'y {a}', **TOL[dtype])
        assert_close_scaled(_np(xg.grad), _np(xt.grad), f'dx {a}', **TOL[dtype])
        if a == 'relu':
            assert torch.equal(y.detach(), torch.relu(x.to(dev)))       # bit-identical to the activation alone
    for pooling in ('mean', 'token0'):
        xt = x.to(dev).float().requires_grad_(True)
        h = F.relu(xt).reshape(N, L, D)
        want = h.mean(dim=1) if pooling == 'mean' else h[:, 0]
        want.backward(dpooled.to(dev).float())
        xg = x.to(dev).requires_grad_(True)
        out = act_dropout_pool(xg, D, 0.0, 'relu', pooling)
        out.backward(dpooled.to(dev))
        assert_close_scaled(_np(out), _np(want), f'pooled {pooling}', **TOL[dtype])
        assert_close_scaled(_np(xg.grad), _np(xt.grad), f'dx pooled {pooling}', **TOL[dtype])


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_same_seed_same_bits_and_eval_ignores_p(case, dev):
    from ampnet_amd import ActDropout, TokenReadout, act_dropout, act_dropout_pool
    shape, dtype = case
    N, L, D = shape
    x = _inputs(shape, dtype)[0].to(dev)
    a, b = act_dropout(x, 0.6, 'elu', seed=SEED), act_dropout(x, 0.6, 'elu', seed=SEED)
    assert torch.equal(a, b) and not torch.equal(a, act_dropout(x, 0.6, 'elu', seed=SEED + 1))
    a, b = act_dropout_pool(x, D, 0.1, 'relu', seed=SEED), act_dropout_pool(x, D, 0.1, 'relu', seed=SEED)
    assert torch.equal(a, b)
    assert torch.equal(act_dropout(x, 0.6, 'relu', training=False), torch.relu(x))
    site, readout = ActDropout(0.6, 'relu', seed=5).eval(), TokenReadout(D, 0.6, 'relu', 'mean', seed=5).eval()
    assert torch.equal(site(x), torch.relu(x)) and site.last_seed is None
    assert torch.equal(readout(x), act_dropout_pool(x, D, 0.0, 'relu'))
    site.train()
    y1, s1 = site(x), site.last_seed
    y2, s2 = site(x), site.last_seed
    assert s1 != s2 and not torch.equal(y1, y2)                  # a fresh mask per training call ...
    assert torch.equal(y1, act_dropout(x, 0.6, 'relu', seed=s1))          # ... that last_seed rebuilds


def test_unaligned_base_takes_the_elementwise_kernels(dev):
    """A contiguous view that starts 4 bytes into an allocation: same mask, same values as the aligned tensor."""
    from ampnet_amd import act_dropout, act_dropout_pool
    shape = (64, 20, 128)
    N, L, D = shape
    x, dy, dpooled = _inputs(shape, 'f32')
    buf = torch.empty(x.numel() + 1, device=dev)
    xv = buf[1:].view(x.shape).copy_(x.to(dev))
    assert xv.data_ptr() % 16 == 4 and xv.is_contiguous()
    xa = x.to(dev).requires_grad_(True)
    xu = xv.requires_grad_(True)
    ya, yu = act_dropout(xa, 0.1, 'elu', seed=SEED), act_dropout(xu, 0.1, 'elu', seed=SEED)
    assert torch.equal(ya, yu)
    ya.backward(dy.to(dev))
    yu.backward(dy.to(dev))
    assert torch.equal(xa.grad, xu.grad)
    pa, pu = act_dropout_pool(xa, D, 0.1, 'relu', seed=SEED), act_dropout_pool(xu, D, 0.1, 'relu', seed=SEED)
    assert_close_scaled(_np(pu), _np(pa), 'pooled, element-wise against 16-byte kernel')


def test_library_rejects_bad_arguments(dev):
    from ampnet_amd import _lib
    lib = _lib.load()
    x = torch.ones(64, device=dev)
    y = torch.empty_like(x)
    assert lib.ampconv_act_dropout_fwd(x.data_ptr(), 64, 1, 0, 65536, 1.0, y.data_ptr(), 0, None) == -1      # T > 65535
    assert lib.ampconv_act_dropout_fwd(x.data_ptr(), 64, 3, 0, 0, 1.0, y.data_ptr(), 0, None) == -1          # activation
    assert lib.ampconv_act_dropout_fwd(x.data_ptr(), 64, 1, 0, 0, 1.0, y.data_ptr(), 7, None) == -2          # dtype
    assert lib.ampconv_pool_fwd(x.data_ptr(), 4, 4, 4, 1, 2, 0, 0, 1.0, y.data_ptr(), 0, None) == -1         # pooling
    assert lib.ampconv_act_dropout_fwd(None, 0, 1, 0, 0, 1.0, None, 0, None) == 0                            # empty
    torch.cuda.synchronize()


# ---- the whole model ---------------------------------------------------------------------------------------------------
def _cfg_value(v):
    if v in ('True', 'False'):
        return v == 'True'
    if v == 'None':
        return None
    try:
        return int(v)
    except ValueError:
        return float(v)


def _cfg(g):
    return {k: _cfg_value(v) for k, v in zip(g['cfg_keys'].tolist(), g['cfg_vals'].tolist())}


def _load_model(g, dev, **override):
    from ampnet_amd import AMPGCN
    model = AMPGCN(device=dev, **{**_cfg(g), **override}).to(dev)
    model.load_state_dict({k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')})
    model.train()
    data = types.SimpleNamespace(x=torch.from_numpy(g['x']).to(dev), edge_index=torch.from_numpy(g['edge_index']).to(dev))
    idx = g.get('sampled_node_feat_indices')
    return model, data, None if idx is None else torch.from_numpy(idx).to(dev)


@pytest.mark.parametrize('path', model_files(), ids=[__import__('os').path.basename(p)[:-4] for p in model_files()])
def test_fused_model_matches_reference_fixture(path, dev):
    """test_model_matches_reference_fixture (tests/test_gpu_featurizer.py) with fused_glue=True: same fixtures, labels
    and tolerances."""
    g = load_golden(path)
    model, data, idx = _load_model(g, dev, fused_glue=True)
    assert model.fused_glue
    logits = model(data, feature_indices=idx)
    (logits * torch.from_numpy(g['dlogits']).to(dev)).sum().backward()
    assert_close_scaled(logits.detach().cpu().numpy(), g['logits'], 'logits')
    assert_close_scaled(model.conv1_embedding.detach().cpu().numpy(), g['conv1_embedding'], 'conv1_embedding')
    assert_close_scaled(model.conv2_embedding.detach().cpu().numpy(), g['conv2_embedding'], 'conv2_embedding')
    for name, p in model.named_parameters():
        key = 'grad.' + name
        if key in g:
            assert_close_scaled(p.grad.cpu().numpy(), g[key], key + '.grad')
        else:
            assert p.grad is None, name


def test_fused_model_with_dropout_matches_the_unfused_composite_under_its_masks(dev):
    """dropout_rate = 0.1 in training mode on the model_cora inputs: the three masks rebuilt in numpy from the sites'
    last_seed, applied by plain PyTorch ops around the same layers, reproduce the fused model's logits."""
    path = [p for p in model_files() if p.endswith('model_cora.npz')][0]
    g = load_golden(path)
    dlogits = torch.from_numpy(g['dlogits']).to(dev)

    def run(rate):
        model, data, idx = _load_model(g, dev, fused_glue=True, dropout_rate=rate, dropout_adj_rate=0.0)
        logits = model(data, feature_indices=idx)
        (logits * dlogits).sum().backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        return model, data, idx, logits.detach(), grads

    _, _, _, logits0, grads0 = run(0.0)
    model, data, idx, logits, grads = run(0.1)
    assert torch.isfinite(logits).all() and not torch.allclose(logits, logits0)
    assert set(grads) == set(grads0)
    for n in grads:
        assert torch.isfinite(grads[n]).all(), n
        assert not torch.equal(grads[n], grads0[n]), n

    seeds = [site.last_seed for site in model._glue]
    assert all(s is not None for s in seeds) and len(set(seeds)) == 3
    thr, scale = ref.mask_params(0.1)

    def drop(t, seed):
        keep = torch.from_numpy(ref.keep_mask(seed, thr, tuple(t.shape))).to(dev)
        return torch.where(keep, t * float(scale), torch.zeros_like(t))

    with torch.no_grad():
        x, _ = model._tokens[0](data.x, idx)
        x = model.conv1(drop(x, seeds[0]), data.edge_index)
        assert_close_scaled(_np(model.conv1_embedding), _np(x), 'conv1_embedding')
        x = model.conv2(drop(F.relu(x), seeds[1]), data.edge_index)
        assert_close_scaled(_np(model.conv2_embedding), _np(x), 'conv2_embedding')
        x = drop(F.relu(x), seeds[2])
        x = x.reshape(x.shape[0], -1, model.emb_dim).mean(dim=1)
        want = F.log_softmax(model.final_linear_out(x), dim=1)
    assert_close_scaled(_np(logits), _np(want), 'logits')
