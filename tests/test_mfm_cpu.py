"""Masked feature modelling on the CPU: the numpy model of tests/mfm_reference.py (which the GPU tests hold the kernels to)
against torch's CPU composite and autograd in double, the statistics of THE TOKEN MASK, the AMPGCN(masked_modelling=...)
state dict, and the argument errors that need no GPU."""
import numpy as np
import pytest
import torch

import mfm_reference as ref
from pipeline_reference import draw

CASES = [(65, 40, 100), (64, 2, 3), (7, 1, 1)]             # (N, L, D = De + 1)


def _inputs(N, L, D, seed=0, empty_rows=True):
    """Seeded featuriser inputs with some idx == -1 rows, a drawn mask at 0.5, decoder inputs."""
    g = np.random.default_rng(seed + 1000 * N + 10 * L + D)
    De, F = D - 1, 11
    x = g.standard_normal((N, F)).astype(np.float32)
    mean, inv_std = x.mean(axis=0).astype(np.float32), (1.0 / x.std(axis=0)).astype(np.float32)
    idx = g.integers(0, F, (N, L)).astype(np.int32)
    if empty_rows and N > 3:
        idx[2] = -1
    table = g.standard_normal((F, De)).astype(np.float32)
    token = (0.02 * g.standard_normal(D)).astype(np.float32)
    masked = ref.token_mask(idx, 5, 32768)
    h = g.standard_normal((N, L, D)).astype(np.float32)
    w = ((g.random(D) * 2 - 1) / D ** 0.5).astype(np.float32)
    b = ((g.random(1) * 2 - 1) / D ** 0.5).astype(np.float32)
    return dict(x=x, mean=mean, inv_std=inv_std, idx=idx, table=table, token=token, masked=masked, h=h, w=w, b=b, F=F)


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize('shape', CASES, ids=[f'N{n}_L{l}_D{d}' for n, l, d in CASES])
@pytest.mark.parametrize('mode', [ref.TOKEN, ref.VALUE], ids=['token', 'value'])
def test_model_matches_the_torch_composite(shape, mode):
    N, L, D = shape
    i = _inputs(N, L, D)
    out, masked, target = ref.build(i['x'], i['mean'], i['inv_std'], i['idx'], i['table'], i['token'], i['masked'], mode)
    assert not masked[i['idx'] < 0].any() and (target[i['idx'] < 0] == 0).all()
    m = torch.from_numpy(masked)
    # the forward composite of the issue: tokens[masked] = mask_token ... ((h[masked] @ w.T + b - target[masked]) ** 2).mean()
    table, token = _t(i['table'], True), _t(i['token'], True)
    ok = torch.from_numpy(i['idx'] >= 0)
    f = torch.from_numpy(np.where(i['idx'] >= 0, i['idx'], 0).astype(np.int64))
    z = (_t(i['x'].astype(np.float64))[torch.arange(N)[:, None], f] - _t(i['mean'])[f]) * _t(i['inv_std'])[f]
    tokens = torch.cat([table[f], z[..., None]], dim=-1) * ok[..., None]
    if mode == ref.TOKEN:
        tokens = torch.where(m[..., None], token, tokens)
    else:
        tokens = torch.cat([tokens[..., :D - 1], torch.where(m, token[D - 1], tokens[..., D - 1])[..., None]], dim=-1)
    np.testing.assert_allclose(out, tokens.detach().numpy(), rtol=0, atol=2e-6)       # z assembled in fp32 by the model
    np.testing.assert_allclose(target, (z * ok).numpy(), rtol=0, atol=2e-6)
    dout = np.random.default_rng(3).standard_normal((N, L, D))
    (tokens * _t(dout)).sum().backward()
    g, S = ref.token_grad(dout, masked, mode)
    np.testing.assert_allclose(g, token.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert (S >= np.abs(g) - 1e-12).all()
    # the table's gradient: the featuriser's on idx with the masked entries at -1 (token mode), on idx as it is (value mode)
    from pipeline_reference import table_grad
    rows = np.where(masked, -1, i['idx']) if mode == ref.TOKEN else i['idx']
    np.testing.assert_allclose(table_grad(dout, rows, i['F'])[0], table.grad.numpy(), rtol=1e-12, atol=1e-12)

    # decoder and loss
    h, w, b = _t(i['h'], True), _t(i['w'][None, :], True), _t(i['b'], True)
    fwd = ref.loss_fwd(i['h'], masked, target, i['w'], i['b'])
    loss = ((h[m] @ w.T + b - _t(target)[m][:, None]) ** 2).mean() if masked.any() else h.sum() * 0
    (3.0 * loss).backward()
    assert fwd['count'] == int(masked.sum())
    np.testing.assert_allclose(fwd['loss'], loss.item(), rtol=1e-12, atol=1e-14)
    assert (fwd['resid'][~masked] == 0).all()
    bwd = ref.loss_bwd(i['h'], masked, fwd['resid'], i['w'], fwd['count'], 3.0)
    np.testing.assert_allclose(bwd['dh'], h.grad.numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(bwd['dw'], w.grad.numpy()[0], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(bwd['db'], b.grad.numpy()[0], rtol=1e-11, atol=1e-13)
    assert (bwd['dh'][~masked] == 0).all()
    # the fixed-point sum of the fp32 residuals is the loss sum to 2^-33 per term
    r32 = fwd['resid'].astype(np.float32)
    want = float((r32.astype(np.float64) ** 2).sum())
    assert abs(ref.fixed_sum(r32) / 2.0 ** ref.SHIFT - want) <= fwd['count'] * 2.0 ** -33 + 1e-15


def test_model_never_touches_unmasked_rows_and_handles_no_mask():
    i = _inputs(16, 4, 8, empty_rows=False)
    masked = i['masked']
    h = i['h'].copy()
    h[~masked] = np.nan
    target = np.random.default_rng(0).standard_normal(masked.shape).astype(np.float32)
    fwd = ref.loss_fwd(h, masked, target, i['w'], i['b'])
    assert np.isfinite(fwd['loss']) and np.isfinite(fwd['resid']).all()
    bwd = ref.loss_bwd(h, masked, fwd['resid'], i['w'], fwd['count'])
    assert np.isfinite(bwd['dw']).all() and np.isfinite(bwd['dh']).all()
    none = np.zeros_like(masked)
    fwd = ref.loss_fwd(h, none, target, i['w'], i['b'])
    assert fwd == {'resid': fwd['resid'], 'count': 0, 'loss': 0.0} and not fwd['resid'].any()
    bwd = ref.loss_bwd(h, none, fwd['resid'], i['w'], 0)
    assert not bwd['dh'].any() and not bwd['dw'].any() and bwd['db'] == 0.0
    g, S = ref.token_grad(np.ones((16, 4, 8)), none, ref.TOKEN)
    assert not g.any() and not S.any()


@pytest.mark.parametrize('threshold', [1, 9830, 49152])
def test_masked_fraction_of_the_mask_model(threshold):
    """Over 2^20 tokens the masked fraction stays within 5 binomial standard deviations of threshold / 65536, and the mask
    is a function of (seed, n, l) alone: another factorisation of the same tokens into (N, L) is another set of (n, l)
    pairs, and where the pairs agree so does the mask."""
    T = 1 << 20
    p = threshold / 65536
    sd = (T * p * (1 - p)) ** 0.5
    idx = np.zeros((T // 64, 64), dtype=np.int32)
    m = ref.token_mask(idx, 12345, threshold)
    assert abs(int(m.sum()) - T * p) <= 5 * sd, (int(m.sum()), T * p, sd)
    wide = ref.token_mask(np.zeros((T // 1024, 1024), dtype=np.int32), 12345, threshold)
    assert abs(int(wide.sum()) - T * p) <= 5 * sd
    assert np.array_equal(wide[:, :64], m[:T // 1024])                     # the same (n, l) pairs: the same mask
    r = draw(12345, np.arange(3)[:, None], np.arange(64)[None, :])
    assert np.array_equal(m[:3], (r >> np.uint64(48)).astype(np.int64) < threshold)
    # idx == -1 is never masked; thresholds 0 and 65536 mask nothing and everything valid
    idx[5] = -1
    assert not ref.token_mask(idx, 12345, 65536)[5].any() and ref.token_mask(idx, 12345, 65536).sum() == T - 64
    assert not ref.token_mask(idx, 12345, 0).any()
    assert ref.threshold_of(0.15) == 9830 and ref.threshold_of(0.75) == 49152 and ref.threshold_of(1.0) == 65536


KW = dict(device='cpu', embedding_dim=16, num_heads=2, num_node_features=12, num_sampled_vectors=5, feat_emb_dim=15, output_dim=3)


@pytest.mark.parametrize('flags', [{}, {'average_pooling_flag': False}, {'layer_norm': True}, {'fused_glue': True},
                                   {'storage_dtype': torch.bfloat16}], ids=['plain', 'token0', 'layer_norm', 'fused_glue', 'bf16'])
def test_state_dict_and_initial_values(flags):
    """Flag off: today's keys.  Flag on: mask_token [1, D] and value_decoder.{weight [1, D], bias [1]} behind them, every
    pre-existing parameter with the values of the flag-off model under the same torch seed, both new ones fp32."""
    from ampnet_amd import AMPGCN
    torch.manual_seed(7)
    off = AMPGCN(**KW, **flags)
    torch.manual_seed(7)
    default = AMPGCN(**KW, **flags, masked_modelling=False)
    torch.manual_seed(7)
    on = AMPGCN(**KW, **flags, masked_modelling=True)
    keys = list(off.state_dict())
    assert 'mask_token' not in keys and not any(k.startswith('value_decoder') for k in keys)
    assert list(default.state_dict()) == keys and not hasattr(off, 'mask_token') and not hasattr(off, 'value_decoder')
    new = ['mask_token', 'value_decoder.weight', 'value_decoder.bias']
    assert [k for k in on.state_dict() if k not in new] == keys          # (torch lists a module's own parameters first)
    assert sorted(k for k in on.state_dict() if k in new) == sorted(new)
    for k, v in off.state_dict().items():
        assert torch.equal(v, on.state_dict()[k]) and v.dtype == on.state_dict()[k].dtype, k
    assert tuple(on.mask_token.shape) == (1, 16) and tuple(on.value_decoder.weight.shape) == (1, 16)
    assert tuple(on.value_decoder.bias.shape) == (1,)
    assert on.mask_token.dtype == on.value_decoder.weight.dtype == on.value_decoder.bias.dtype == torch.float32
    assert 0 < float(on.mask_token.detach().std()) < 0.1                           # normal_(std=.02)
    on._check_storage()
    with pytest.raises(ValueError, match='storage'):
        on.to(torch.bfloat16)._check_storage()                            # a whole-model cast is not a storage mode


def test_argument_errors_without_a_gpu():
    from ampnet_amd import AMPGCN, FeatureTokens, MaskedValueHead, build_masked_tokens, masked_value_loss
    from ampnet_amd.masked import mask_threshold
    import types
    data = types.SimpleNamespace(x=torch.randn(6, 12), edge_index=torch.randint(0, 6, (2, 10)))
    with pytest.raises(ValueError, match='masked_modelling=True'):
        AMPGCN(**KW).masked_feature_loss(data)
    with pytest.raises(ValueError, match='readout_token_only'):
        AMPGCN(**KW, average_pooling_flag=False, readout_token_only=True, masked_modelling=True).masked_feature_loss(data)
    assert mask_threshold(0) == 0 and mask_threshold(0.15) == 9830 and mask_threshold(1) == 65536
    for rate in (-0.1, 1.01, float('nan')):
        with pytest.raises(ValueError, match='mask rate'):
            mask_threshold(rate)
    h, masked, target = torch.randn(4, 2 * 8), torch.zeros(4, 2, dtype=torch.bool), torch.randn(4, 2)
    head = MaskedValueHead(8)
    assert list(head.state_dict()) == ['weight', 'bias']
    with pytest.raises(ValueError, match='no CPU fallback'):
        head(h, masked, target)
    with pytest.raises(ValueError, match='no CPU fallback'):
        masked_value_loss(h, masked, target, head.weight, head.bias)
    tokens = FeatureTokens(12, 7, 5)
    with pytest.raises(ValueError, match='GPU'):
        tokens.forward_masked(torch.randn(6, 12), rate=0.15, mask_token=torch.zeros(1, 8))
    with pytest.raises(ValueError, match='GPU'):
        build_masked_tokens(torch.randn(12, 7), torch.zeros(1, 8), torch.randn(6, 12), torch.zeros(12), torch.ones(12),
                            torch.zeros(6, 5, dtype=torch.int32), seed=0, rate=0.15)
