"""The per-token LayerNorm sites without a GPU: the numpy model of tests/norm_reference.py against torch's CPU composite
and its autograd in float64, the binding's signatures, the state-dict contract of the new modules and of
AMPGCN(layer_norm=...), and the argument errors that need no device."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import glue_reference as glue
import norm_reference as ref

SHAPES = [(5, 3, 4), (17, 2, 3), (9, 40, 100)]
ACTS = {'identity': lambda t: t, 'relu': F.relu, 'elu': F.elu}
PS = [0.0, 0.1, 0.6]
SEED = 0x0FEDCBA987654321
EPS = 1e-5
# rtol 1e-9 between two float64 computations of the same formulas; atol 1e-12 for the entries that cancel to (almost)
# nothing: sums of at most 9 * 40 terms of magnitude <= ~10 carry absolute rounding errors of ~1e-13
TOL = dict(rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('shape', SHAPES, ids=[f'N{n}_L{l}_D{d}' for n, l, d in SHAPES])
def test_numpy_model_matches_torch_composite_in_float64(shape):
    N, L, D = shape
    g = torch.Generator().manual_seed(100 * N + D)
    x = torch.randn(N, L * D, generator=g, dtype=torch.float64)
    dy = torch.randn(N, L * D, generator=g, dtype=torch.float64)
    dpooled = torch.randn(N, D, generator=g, dtype=torch.float64)
    gamma = 1 + 0.5 * torch.randn(D, generator=g, dtype=torch.float64)
    beta = 0.5 * torch.randn(D, generator=g, dtype=torch.float64)
    for p in PS:
        thr, scale = glue.mask_params(p)
        mask = torch.from_numpy(glue.keep_mask(SEED, thr, (N, L * D))).double() * float(scale)
        for name, act in ACTS.items():
            def composite(xt, gt, bt):
                return act(F.layer_norm(xt.view(N, L, D), (D,), gt, bt, EPS)).view(N, L * D) * mask

            xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
            y = composite(xt, gt, bt)
            y.backward(dy)
            got_y, stats = ref.norm_fwd(x.numpy(), D, gamma.numpy(), beta.numpy(), EPS, name, SEED, p)
            dx, dg, db = ref.norm_bwd(x.numpy(), dy.numpy(), D, gamma.numpy(), beta.numpy(), EPS, name, SEED, p)
            np.testing.assert_allclose(got_y, y.detach().numpy(), **TOL)
            np.testing.assert_allclose(dx, xt.grad.numpy(), **TOL)
            np.testing.assert_allclose(dg, gt.grad.numpy(), **TOL)
            np.testing.assert_allclose(db, bt.grad.numpy(), **TOL)
            tok = x.view(-1, D)
            np.testing.assert_allclose(stats[:, 0], tok.mean(1).numpy(), **TOL)
            np.testing.assert_allclose(stats[:, 1], (1 / torch.sqrt(tok.var(1, unbiased=False) + EPS)).numpy(), **TOL)
            for pooling in ('mean', 'token0'):
                xt, gt, bt = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
                h = composite(xt, gt, bt).view(N, L, D)
                pooled = h.mean(dim=1) if pooling == 'mean' else h[:, 0]
                pooled.backward(dpooled)
                args = (D, gamma.numpy(), beta.numpy(), EPS, name, pooling, SEED, p)
                got, pstats = ref.norm_pool_fwd(x.numpy(), L, *args)
                dx, dg, db = ref.norm_pool_bwd(x.numpy(), dpooled.numpy(), L, *args)
                assert pstats.shape == ((N * L, 2) if pooling == 'mean' else (N, 2))
                np.testing.assert_allclose(got, pooled.detach().numpy(), **TOL)
                np.testing.assert_allclose(dx, xt.grad.numpy(), **TOL)
                np.testing.assert_allclose(dg, gt.grad.numpy(), **TOL)
                np.testing.assert_allclose(db, bt.grad.numpy(), **TOL)
    # without weight and bias: gamma = 1, beta = 0
    got_y, _ = ref.norm_fwd(x.numpy(), D, None, None, EPS, 'identity', SEED, 0.0)
    np.testing.assert_allclose(got_y, F.layer_norm(x.view(N, L, D), (D,), None, None, EPS).view(N, -1).numpy(), **TOL)


def test_binding_declares_the_norm_entry_points():
    from ampnet_amd import _lib
    for name in ('ampconv_norm_fwd', 'ampconv_norm_bwd', 'ampconv_norm_pool_fwd', 'ampconv_norm_pool_bwd',
                 'ampconv_norm_workspace_bytes'):
        assert name in _lib.SIGNATURES, name
    assert _lib.EXPECTED_ABI == 111


DEFAULT_KEYS = ['feature_embedding_table.weight',
                'conv1.multi_head_attention.in_proj_weight', 'conv1.multi_head_attention.in_proj_bias',
                'conv1.multi_head_attention.out_proj.weight', 'conv1.multi_head_attention.out_proj.bias',
                'conv2.multi_head_attention.in_proj_weight', 'conv2.multi_head_attention.in_proj_bias',
                'conv2.multi_head_attention.out_proj.weight', 'conv2.multi_head_attention.out_proj.bias',
                'final_linear_out.weight', 'final_linear_out.bias']
NORM_KEYS = ['norm1.weight', 'norm1.bias', 'norm2.weight', 'norm2.bias']


def test_state_dicts_of_the_model_and_the_modules():
    from ampnet_amd import AMPGCN, NormTokenReadout, TokenLayerNorm
    small = dict(device='cpu', embedding_dim=16, num_heads=2, num_node_features=12, num_sampled_vectors=5, feat_emb_dim=15)
    default = AMPGCN(**small)
    assert sorted(default.state_dict()) == sorted(DEFAULT_KEYS)            # exactly the reference class's keys, as before
    assert not hasattr(default, 'norm1') and default.layer_norm is False
    assert sorted(AMPGCN(layer_norm=False, **small).state_dict()) == sorted(DEFAULT_KEYS)
    for flags in ({}, {'fused_glue': True}, {'fused_head': True}, {'fused_glue': True, 'fused_head': True}):
        model = AMPGCN(layer_norm=True, **flags, **small)
        assert sorted(model.state_dict()) == sorted(DEFAULT_KEYS + NORM_KEYS), flags
        assert model.norm1.activation == model.norm2.activation == 'relu' and model.norm2.pooling == 'mean'
    assert AMPGCN(layer_norm=True, average_pooling_flag=False, **small).norm2.pooling == 'token0'

    want = nn.LayerNorm(16).state_dict()
    for module in (TokenLayerNorm(16), NormTokenReadout(16)):
        got = module.state_dict()
        assert list(got) == list(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        module.load_state_dict({'weight': torch.full((16,), 2.0), 'bias': torch.full((16,), -1.0)})      # loads by key
        assert float(module.weight.detach()[3]) == 2.0 and float(module.bias.detach()[3]) == -1.0
    assert not TokenLayerNorm(16, elementwise_affine=False).state_dict()
    site = TokenLayerNorm(16, p=0.5, activation='elu', seed=3, site=2)
    assert site.last_seed is None and site._next_seed() == site.last_seed != site._next_seed()
    assert site.eval()._next_seed() == 0


def test_argument_errors_need_no_device():
    from ampnet_amd import TokenLayerNorm, norm_act_dropout, norm_act_dropout_pool
    x = torch.ones(4, 2 * 8)
    for fn in (norm_act_dropout, norm_act_dropout_pool):
        with pytest.raises(ValueError, match='on the GPU'):
            fn(x, 8)                                                        # a CPU tensor: no fallback
        with pytest.raises(ValueError, match='float32 or bfloat16'):
            fn(x.double(), 8)
        with pytest.raises(ValueError, match='embed_dim'):
            fn(x, 5)                                                        # 16 is no multiple of 5
        with pytest.raises(ValueError, match='1024'):
            fn(torch.ones(2, 1028), 1028)
        with pytest.raises(ValueError, match='eps'):
            fn(x, 8, eps=0.0)
        with pytest.raises(ValueError, match='dropout probability'):
            fn(x, 8, p=1.0)
        with pytest.raises(ValueError, match='activation'):
            fn(x, 8, activation='gelu')
    with pytest.raises(ValueError, match='pooling'):
        norm_act_dropout_pool(x, 8, pooling='max')
    with pytest.raises(ValueError, match='1024'):
        TokenLayerNorm(1028)
    with pytest.raises(ValueError, match='eps'):
        TokenLayerNorm(8, eps=0.0)
    with pytest.raises(ValueError, match='dropout probability'):
        TokenLayerNorm(8, p=1.0)
