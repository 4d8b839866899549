"""Masked feature modelling through its Python layers (ampnet_amd/masked.py, FeatureTokens.forward_masked,
AMPGCN.masked_feature_loss) on the GPU: against the torch composite of the same maths under torch.autograd, a replayed
mask against the drawn run, the whole model against the same walk with the masking and the loss written as torch ops, the
training step without a device synchronisation, and the flag-off model against the untouched path.

Shapes (N, L, D): (65, 40, 100) the class-default token shape (a ragged last tile, fp32 in 16-byte and bf16 in 8-byte
pieces, downsampled tokens) and (64, 2, 3) the XOR toy (element-wise kernels, full-width tokens); the kernels' other paths
are on the ladder of tests/test_gpu_mfm_kernels.py.  The model: a 60-node graph, dropout 0.
Tolerances: the project's flat atol 1e-5, rtol 1e-4 on tokens, losses and fp32 dh; the scaled bar (labels `.grad`) on
parameter gradients; bf16 storage atol = rtol = 2e-2 (tests/test_gpu_glue.py); masks and counts exact."""
import types

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_scaled

pytestmark = pytest.mark.gpu

BF16 = dict(atol=2e-2, rtol=2e-2)
SHAPES = [((65, 40, 100), 'f32'), ((65, 40, 100), 'bf16'), ((64, 2, 3), 'f32')]
DT = {'f32': torch.float32, 'bf16': torch.bfloat16}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _np(t):
    return t.detach().float().cpu().numpy()


def _mask_tokens(tokens3, masked, mask_token, mode):
    """The composite of the issue: tokens[masked] = mask_token (mode 'token'); the value slot alone (mode 'value')."""
    D = tokens3.size(-1)
    mt = mask_token.reshape(-1).to(tokens3.dtype)
    if mode == 'token':
        return torch.where(masked[..., None], mt.view(1, 1, D), tokens3)
    return torch.cat([tokens3[..., :D - 1], torch.where(masked, mt[D - 1], tokens3[..., D - 1])[..., None]], dim=-1)


def _composite_loss(h3, masked, target, weight, bias):
    return ((h3[masked].float() @ weight.T + bias - target[masked][:, None]) ** 2).mean()


@pytest.mark.parametrize('mode', ['token', 'value'])
@pytest.mark.parametrize('case', SHAPES, ids=[f'N{s[0]}_L{s[1]}_D{s[2]}_{d}' for s, d in SHAPES])
def test_tokens_and_loss_match_the_torch_composite(case, mode, dev):
    from ampnet_amd import FeatureTokens, masked_value_loss
    (N, L, D), dtype = case
    tol = BF16 if dtype == 'bf16' else {}
    g = torch.Generator().manual_seed(N + D)
    full = L == 2
    Fdim = 2 if full else 50
    ft = FeatureTokens(Fdim, D - 1, L, seed=3, token_dtype=DT[dtype]).to(dev)
    x = (torch.randn(N, Fdim, generator=g) + 0.1).to(dev)
    mask_token = (0.5 * torch.randn(1, D, generator=g)).to(dev).requires_grad_(True)
    tokens, idx, masked, target = ft.forward_masked(x, rate=0.4, mode=mode, mask_token=mask_token,
                                                    full_width_repeats=1 if full else None)
    assert tokens.shape == (N, L * D) and tokens.dtype == DT[dtype] and masked.dtype == torch.bool and masked.shape == (N, L)
    assert (idx is None) == full and target.dtype == torch.float32
    share = float(masked.float().mean())
    assert abs(share - 0.4) <= 5 * (0.4 * 0.6 / (N * L)) ** 0.5 + 1e-3, share        # round(0.4 * 65536) / 65536
    dout = torch.randn(N, L * D, generator=g).to(dev).to(DT[dtype])
    tokens.backward(dout)
    got_table, got_token = ft.feature_embedding_table.weight.grad.clone(), mask_token.grad.clone()
    # the composite on the untouched featuriser
    ft.feature_embedding_table.weight.grad = None
    twin_token = mask_token.detach().clone().requires_grad_(True)
    plain, _ = ft.forward_all(x, 1) if full else ft(x, idx)
    want = _mask_tokens(plain.view(N, L, D), masked, twin_token, mode)
    assert torch.equal(tokens.view(N, L, D), want), 'tokens differ from the composite'            # bit for bit
    want.backward(dout.view(N, L, D))
    mean, inv_std = ft.zscore_stats(x)
    used = torch.arange(L, device=dev).repeat(N, 1) if full else idx.long()
    z = (x.gather(1, used) - mean[used]) * inv_std[used]
    assert_close_scaled(_np(target), _np(z), 'target')
    assert_close_scaled(_np(got_token), _np(twin_token.grad), 'mask_token.grad', **tol)
    assert_close_scaled(_np(got_table), _np(ft.feature_embedding_table.weight.grad), 'feature_embedding_table.weight.grad', **tol)

    # the loss behind it
    h = torch.randn(N, L * D, generator=g).to(dev).to(DT[dtype])
    W = ((torch.rand(1, D, generator=g) * 2 - 1) / D ** 0.5).to(dev)
    b = ((torch.rand(1, generator=g) * 2 - 1) / D ** 0.5).to(dev)
    leaves = [t.clone().requires_grad_(True) for t in (h, W, b)]
    twins = [t.clone().requires_grad_(True) for t in (h, W, b)]
    loss = masked_value_loss(leaves[0], masked, target, leaves[1], leaves[2])
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    (3 * loss).backward()
    ref = _composite_loss(twins[0].view(N, L, D), masked, target, twins[1], twins[2])
    (3 * ref).backward()
    assert_close_scaled(loss.item(), ref.item(), 'loss')
    assert leaves[0].grad.dtype == DT[dtype]
    assert_close_scaled(_np(leaves[0].grad), _np(twins[0].grad), 'dh', **tol)
    assert_close_scaled(_np(leaves[1].grad), _np(twins[1].grad), 'weight.grad')
    assert_close_scaled(_np(leaves[2].grad), _np(twins[2].grad), 'bias.grad')
    rows = leaves[0].grad.view(N, L, D)[~masked]
    assert bool((rows.view(torch.int16 if dtype == 'bf16' else torch.int32) == 0).all())
    # the 3-D layout of h is the same call
    assert torch.equal(masked_value_loss(h.view(N, L, D), masked, target, W, b), loss.detach())


def _model(dev, **flags):
    from ampnet_amd import AMPGCN
    torch.manual_seed(11)
    kw = dict(device=dev, embedding_dim=16, num_heads=2, num_node_features=12, num_sampled_vectors=5, feat_emb_dim=15,
              output_dim=3, dropout_rate=0.0, dropout_adj_rate=0.0)
    kw.update(flags)
    return AMPGCN(**kw).to(dev)


def _graph(dev, N=60, Fdim=12, L=5):
    g = torch.Generator().manual_seed(5)
    data = types.SimpleNamespace(x=(torch.randn(N, Fdim, generator=g) + 0.2).to(dev),
                                 edge_index=torch.randint(0, N, (2, 300), generator=g).to(dev))
    return data, torch.randint(0, Fdim, (N, L), generator=g).to(dev)


def _twin_loss(model, data, idx, masked, mode):
    """masked_feature_loss with the masking and the loss as torch ops around the library's own featuriser and convs."""
    N, D, found = data.x.size(0), model.emb_dim, {}

    def featurise(x):
        tokens, sampled = model._tokens[0](x, idx)
        mean, inv_std = model._tokens[0].zscore_stats(x)
        found['target'] = (x.gather(1, sampled.long()) - mean[sampled.long()]) * inv_std[sampled.long()]
        return _mask_tokens(tokens.view(N, -1, D), masked, model.mask_token, mode).reshape(N, -1), sampled

    h2 = model._run(data, featurise=featurise, readout=False)
    return _composite_loss(h2.view(N, -1, D), masked, found['target'], model.value_decoder.weight, model.value_decoder.bias)


VARIANTS = {'plain': {}, 'fused_glue': {'fused_glue': True}, 'layer_norm': {'layer_norm': True},
            'bf16': {'storage_dtype': torch.bfloat16}}


@pytest.mark.parametrize('mode', ['token', 'value'])
@pytest.mark.parametrize('variant', list(VARIANTS))
def test_model_loss_and_every_gradient_match_the_torch_walk(variant, mode, dev):
    model = _model(dev, masked_modelling=True, **VARIANTS[variant])
    model.train()
    data, idx = _graph(dev)
    tol = BF16 if variant == 'bf16' else {}
    drawn = model.masked_feature_loss(data, mask_rate=0.5, mask_mode=mode, feature_indices=idx)
    masked = model.token_mask
    assert masked.dtype == torch.bool and masked.shape == (60, 5) and 0 < int(masked.sum()) < 300
    assert torch.equal(model.sampled_node_feat_indices, idx.to(torch.int32))
    h2_drawn = model.conv2_embedding.detach().clone()
    # a replayed mask reproduces the drawn run bit for bit
    loss = model.masked_feature_loss(data, mask_rate=0.0, mask_mode=mode, feature_indices=idx, token_mask=masked)
    assert torch.equal(loss.detach().view(torch.int32), drawn.detach().view(torch.int32))
    assert torch.equal(model.conv2_embedding, h2_drawn) and torch.equal(model.token_mask, masked)
    assert model.conv1_embedding.shape == model.conv2_embedding.shape == (60, 5 * 16)
    loss.backward()
    got = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    want_loss = _twin_loss(model, data, idx, masked, mode)
    want_loss.backward()
    assert_close_scaled(loss.item(), want_loss.item(), 'loss', **tol)
    for n, p in model.named_parameters():
        if p.grad is None:
            assert n not in got, n                                  # behind conv2 (head, readout norm): none either way
        else:
            assert_close_scaled(_np(got[n]), _np(p.grad), f'{n}.grad', **tol)
    assert {'mask_token', 'value_decoder.weight', 'value_decoder.bias', 'feature_embedding_table.weight'} <= set(got)


def test_full_width_model_and_refusals(dev):
    """The XOR harness's branch (every feature column a token, the table tiled feature_repeats times) and what raises."""
    from ampnet_amd import AMPGCN
    torch.manual_seed(2)
    model = AMPGCN(device=dev, embedding_dim=3, num_heads=1, num_node_features=2, num_sampled_vectors=10, output_dim=2,
                   feat_emb_dim=2, downsample_feature_vectors=False, dropout_rate=0.0, dropout_adj_rate=0.0, feature_repeats=5,
                   masked_modelling=True).to(dev)
    g = torch.Generator().manual_seed(1)
    data = types.SimpleNamespace(x=torch.randn(64, 10, generator=g).to(dev), edge_index=torch.randint(0, 64, (2, 400), generator=g).to(dev))
    loss = model.masked_feature_loss(data, mask_rate=0.3, mask_mode='value')
    loss.backward()
    assert model.sampled_node_feat_indices is None and model.token_mask.shape == (64, 10)
    assert torch.isfinite(loss) and model.feature_embedding_table.weight.grad.shape == (2, 2)
    assert bool(torch.isfinite(model.mask_token.grad).all()) and bool((model.mask_token.grad[0, :2] == 0).all())
    first = model.token_mask
    again = model.masked_feature_loss(data, mask_rate=0.3, mask_mode='value')
    assert torch.isfinite(again) and not torch.equal(model.token_mask, first)      # a fresh draw per call: (seed, calls)
    with pytest.raises(ValueError, match='mask mode'):
        model.masked_feature_loss(data, mask_mode='tokens')
    with pytest.raises(ValueError, match='mask rate'):
        model.masked_feature_loss(data, mask_rate=1.5)
    with pytest.raises(ValueError, match='token mask'):
        model.masked_feature_loss(data, token_mask=torch.zeros(64, 9, dtype=torch.bool, device=dev))
    # rate 0: nothing masked, loss exactly 0, gradients exactly 0
    model.zero_grad(set_to_none=True)
    zero = model.masked_feature_loss(data, mask_rate=0.0)
    zero.backward()
    assert zero.item() == 0.0 and not bool(model.token_mask.any())
    for n, p in model.named_parameters():
        assert p.grad is None or bool((p.grad == 0).all()), n


def test_training_steps_without_a_device_synchronisation(dev):
    """Three steps of masked tokens -> a trained map -> masked_value_loss -> backward -> FusedAdam.step with no device
    synchronisation in between (the way tests/test_gpu_head.py checks its loss), the MaskedMetrics total against the
    per-step sums; then three steps of the whole model, which must lower nothing in particular but run."""
    from ampnet_amd import FusedAdam, MaskedMetrics, MaskedValueHead, build_masked_tokens
    N, L, D, Fdim = 65, 40, 100, 50
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, Fdim, generator=g).to(dev)
    idx = torch.randint(0, Fdim, (N, L), generator=g, dtype=torch.int32).to(dev)
    mean, inv_std = x.mean(0), 1.0 / x.std(0)
    table = torch.randn(Fdim, D - 1, generator=g).to(dev).requires_grad_(True)
    mask_token = (0.02 * torch.randn(1, D, generator=g)).to(dev).requires_grad_(True)
    scale = torch.ones(D, device=dev, requires_grad=True)
    head = MaskedValueHead(D).to(dev)
    opt = FusedAdam([table, mask_token, scale, *head.parameters()], lr=1e-2)
    total = MaskedMetrics(dev)
    losses, counts = [], []

    def step(k):
        # mode 'value': a masked token keeps its table row, so the loss -- which reads masked rows only -- trains the table
        tokens, masked, target = build_masked_tokens(table, mask_token, x, mean, inv_std, idx, seed=100 + k, rate=0.15,
                                                     mode='value')
        loss = head(tokens * scale, masked, target, total)
        loss.backward()
        opt.step(set_to_none=True)
        losses.append(loss.detach())
        counts.append(masked.sum())

    step(0)                                                       # warm up: library load, optimiser state, allocator
    torch.cuda.synchronize()
    total.reset()
    del losses[:], counts[:]
    before = [p.detach().clone() for p in (table, mask_token, scale, head.weight, head.bias)]
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for k in range(1, 4):
            step(k)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    for p, q in zip((table, mask_token, scale, head.weight, head.bias), before):
        assert not torch.equal(p.detach(), q), 'a parameter did not move'
    got = total.read()
    assert got['count'] == sum(int(c) for c in counts) and got['count'] > 0
    want_sq = sum(float(l) * int(c) for l, c in zip(losses, counts))
    assert_close_scaled(got['sq_sum'], want_sq, 'sum of squares over three steps', rtol=1e-6, atol=1e-6)
    assert abs(total.mse() - want_sq / got['count']) <= 1e-6 * max(1.0, total.mse())
    assert total.reset().read() == {'sq_sum': 0.0, 'count': 0}

    # the whole model under FusedAdam, fp32 and bf16 storage, metrics accumulated over the steps
    for flags in ({}, {'storage_dtype': torch.bfloat16, 'fused_glue': True}):
        model = _model(dev, masked_modelling=True, **flags)
        model.train()
        data, idx5 = _graph(dev)
        opt = FusedAdam(model.parameters(), lr=1e-2)
        metrics, per_step = MaskedMetrics(dev), []
        for _ in range(3):
            loss = model.masked_feature_loss(data, mask_rate=0.5, feature_indices=idx5, metrics=metrics)
            loss.backward()
            opt.step(set_to_none=True)
            per_step.append((loss.detach(), model.token_mask.sum()))
        seen = metrics.read()
        assert seen['count'] == sum(int(c) for _, c in per_step)
        assert_close_scaled(seen['sq_sum'], sum(float(l) * int(c) for l, c in per_step), 'model: sum of squares', rtol=1e-6,
                            atol=1e-6)
        assert all(torch.isfinite(l) for l, _ in per_step)


def test_flag_off_forward_is_the_untouched_path(dev):
    """masked_modelling=False (the default) and =True give the bits of the walk assembled here from the untouched pieces:
    the model's featuriser, its three sites, conv1, conv2, final_linear_out and log_softmax."""
    data, idx = _graph(dev)
    outs = {}
    for flag in (False, True):
        model = _model(dev, masked_modelling=flag)
        model.eval()
        with torch.no_grad():
            outs[flag] = model(data, feature_indices=idx)
            tokens, _ = model._tokens[0](data.x, idx)
            entry, between, readout = model._sites
            h2 = model.conv2(between(model.conv1(entry(tokens), data.edge_index)), data.edge_index)
            by_hand = F.log_softmax(model.final_linear_out(readout(h2).float()), dim=1)
        assert torch.equal(outs[flag].view(torch.int32), by_hand.view(torch.int32)), flag
        assert torch.equal(model.conv2_embedding, h2)
    assert torch.equal(outs[False].view(torch.int32), outs[True].view(torch.int32))
    assert not hasattr(_model(dev), 'mask_token')
