"""AMPConv.forward_token and AMPGCN(readout_token_only=True) on the GPU.

forward_token's specification is `forward(x, edge_index).view(N, L, D)[:, token]`, values and gradients, so it is held to
the bars the full layer is held to against the same oracle (oracle/ampconv_torch.py in fp64 on the CPU, sliced to the
token): tests/test_gpu_parity.py's fp32 bars -- conftest.assert_close_scaled, FLAT atol 1e-5 / rtol 1e-4 on per-row
tensors, magnitude-scaled atol on parameter gradients -- and, bf16 storage, the bar of tests/test_gpu_bf16_model.py
(rtol = atol = 2e-2 of the tensor's scale), the oracle evaluated on the bf16-rounded inputs and parameters.  The flagged
model is held to the same bars against the unflagged model on one state dict."""
import functools
import types

import numpy as np
import pytest
import torch

from conftest import assert_close_scaled

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
BF16_BAR = 2e-2          # tests/test_gpu_bf16_model.py (the project's bf16 bar: tests/test_gpu_parity.py::test_bf16_storage)
N = 40
SHAPES = [(5, 8, 2), (20, 128, 4), (40, 100, 2)]          # L, D, H


def _id(s):
    return 'L%d_D%d_H%d' % s


@functools.lru_cache(maxsize=None)
def _edges():
    """40 nodes, 170 edges: nodes 34..39 isolated, node 5 receives nothing, node 6 sends nothing, a multi-edge 1 -> 2
    (three times), self-loops."""
    g = torch.Generator().manual_seed(5)
    ei = torch.randint(0, 34, (2, 170), generator=g)
    ei[1, ei[1] == 5] = 7
    ei[0, ei[0] == 6] = 8
    ei[:, :3] = torch.tensor([[1, 1, 1], [2, 2, 2]])
    ei[:, 3:5] = torch.tensor([[9, 11], [9, 11]])
    return ei


def _f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def _layer_case(shape, bf16):
    """(state dict, x, dy [N, L*D] -- a token's gradient is a slice of it --, and per token the oracle's y, dx and the
    four parameter gradients in fp64), computed once per shape and storage."""
    from oracle.ampconv_torch import RefShapedAMPConv
    L, D, H = shape
    torch.manual_seed(31)
    ref = RefShapedAMPConv(D, H)
    with torch.no_grad():
        ref.multi_head_attention.in_proj_bias.normal_(0, 0.1)
        ref.multi_head_attention.out_proj.bias.normal_(0, 0.1)
    g = torch.Generator().manual_seed(32)
    x, dy = torch.randn(N, L * D, generator=g), torch.randn(N, L * D, generator=g)
    if bf16:                         # the oracle sees what the bf16 layer stores
        ref = ref.to(torch.bfloat16)
        x, dy = x.to(torch.bfloat16), dy.to(torch.bfloat16)
    state = {k: v.clone() for k, v in ref.state_dict().items()}
    ref = ref.double()
    want = {}
    for t in (0, L - 1):
        ref.zero_grad()
        xr = x.double().requires_grad_(True)
        y = ref(xr, _edges()).view(N, L, D)[:, t]
        y.backward(dy.double().view(N, L, D)[:, t])
        m = ref.multi_head_attention
        want[t] = {'y': y.detach().numpy(), 'dx': xr.grad.numpy(), 'g_in_proj_weight': m.in_proj_weight.grad.numpy().copy(),
                   'g_in_proj_bias': m.in_proj_bias.grad.numpy().copy(), 'g_out_proj_weight': m.out_proj.weight.grad.numpy().copy(),
                   'g_out_proj_bias': m.out_proj.bias.grad.numpy().copy()}
    return state, x, dy, want


def _layer(shape, state, bf16=False, **kw):
    from ampnet_amd import AMPConv
    L, D, H = shape
    layer = AMPConv(D, H, **kw)
    layer.load_state_dict({k: v.float() for k, v in state.items()})
    layer = layer.to(DEV)
    return layer.to(torch.bfloat16) if bf16 else layer


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_forward_token_against_the_oracle(shape, bf16):
    from ampnet_amd.conv import functional as F_
    L, D, H = shape
    state, x, dy, want = _layer_case(shape, bf16)
    assert F_.token_supported(L, D, H, torch.bfloat16 if bf16 else torch.float32)      # the fast path is what runs
    tol = dict(atol=BF16_BAR, rtol=BF16_BAR, scaled=True) if bf16 else {}
    failures = []
    for t in (0, L - 1):
        layer = _layer(shape, state, bf16)
        xg = x.to(DEV).requires_grad_(True)
        y = layer.forward_token(xg, _edges().to(DEV), t)
        assert y.shape == (N, D) and y.dtype == x.dtype
        y.backward(dy.view(N, L, D)[:, t].to(DEV))
        m = layer.multi_head_attention
        got = {'y': y, 'dx': xg.grad, 'g_in_proj_weight': m.in_proj_weight.grad, 'g_in_proj_bias': m.in_proj_bias.grad,
               'g_out_proj_weight': m.out_proj.weight.grad, 'g_out_proj_bias': m.out_proj.bias.grad}
        for name, ref in want[t].items():
            try:
                assert_close_scaled(_f64(got[name]), ref, f't={t} {name}', **tol)
            except AssertionError as e:                                # every tensor's figure is printed before any fails
                failures.append(str(e))
        yh = _f64(y)
        assert not yh[5].any() and not yh[34:].any()                   # rows nobody sends to: exactly 0, not the bias
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('how', ['unsupported shape', 'softmax=False', 'AMPCONV_FORCE_GENERIC=1'])
def test_fallback_is_the_full_layer_and_a_slice(how, monkeypatch):
    from ampnet_amd import AMPConv
    from ampnet_amd.conv import functional as F_
    L, D, H = (3, 130, 1) if how == 'unsupported shape' else (5, 8, 2)
    if how == 'unsupported shape':
        assert not F_.token_supported(L, D, H, torch.float32)
    if how.startswith('AMPCONV'):
        monkeypatch.setenv('AMPCONV_FORCE_GENERIC', '1')
    monkeypatch.setattr(F_.AMPConvTokenFunction, 'apply', None)        # the fast path may not be entered
    torch.manual_seed(33)
    layer = AMPConv(D, H, softmax=how != 'softmax=False').to(DEV)
    x = torch.randn(N, L * D, generator=torch.Generator().manual_seed(34)).to(DEV)
    ei = _edges().to(DEV)
    for t in (0, L - 1):
        a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
        ya = layer.forward_token(a, ei, t)
        yb = layer(b, ei).view(N, L, D)[:, t]
        assert ya.shape == (N, D) and torch.equal(ya, yb)
        ya.sum().backward()
        yb.sum().backward()
        assert torch.equal(a.grad, b.grad)
    assert layer.attn_output_weights is not None                       # the full layer ran: its side outputs are there


def test_side_outputs_raise_after_forward_token():
    from ampnet_amd import AMPConv
    L, D, H = 5, 8, 2
    layer = AMPConv(D, H).to(DEV)
    x, ei = torch.randn(N, L * D, device=DEV), _edges().to(DEV)
    layer(x, ei)
    assert layer.attn_output_weights.shape == (ei.size(1), L, L)
    layer.forward_token(x, ei, 0)
    feats = torch.zeros(N, L, dtype=torch.int32, device=DEV)
    for read_it in (lambda: layer.attn_output, lambda: layer.attn_output_weights,
                    lambda: layer.attention_heatmap(feats, num_features=4)):
        with pytest.raises(RuntimeError, match='forward_token'):
            read_it()
    layer(x, ei)                                                       # ... and the next full call brings them back
    assert layer.attn_output_weights.shape == (ei.size(1), L, L)
    with pytest.raises(ValueError, match='token must be in'):
        layer.forward_token(x, ei, L)


# ------------------------------------------------------------------------------------------------------ the model
FEATS, CLASSES, ML, MD, MH = 24, 4, 5, 8, 2
MODEL_FLAGS = {'plain': {}, 'fused_glue': dict(fused_glue=True), 'layer_norm': dict(layer_norm=True),
               'fused_head': dict(fused_head=True), 'bf16': dict(storage_dtype=torch.bfloat16)}
MN = 30


@functools.lru_cache(maxsize=None)
def _model_data():
    g = torch.Generator().manual_seed(41)
    x = (torch.rand(MN, FEATS, generator=g) < 0.3).float() * (1.0 + torch.rand(MN, FEATS, generator=g))
    x[torch.arange(MN), torch.randint(0, FEATS, (MN,), generator=g)] = 1.0
    ei = torch.randint(0, MN - 3, (2, 120), generator=g)              # nodes 27..29 isolated
    ei[:, :2] = torch.tensor([[1, 1], [2, 2]])
    rng = np.random.default_rng(42)
    idx = torch.from_numpy(np.stack([rng.choice(np.flatnonzero(row), ML) for row in x.numpy()]).astype(np.int32))
    y = torch.randint(0, CLASSES, (MN,), generator=g)
    w = torch.rand(MN, generator=g) + 0.5
    return x, ei, idx, y, w


def _models(flags):
    from ampnet_amd import AMPGCN
    out = []
    for token_only in (False, True):
        torch.manual_seed(43)
        out.append(AMPGCN(device=DEV, embedding_dim=MD, num_heads=MH, num_node_features=FEATS, num_sampled_vectors=ML,
                          output_dim=CLASSES, feat_emb_dim=MD - 1, average_pooling_flag=False, dropout_rate=0.0,
                          dropout_adj_rate=0.0, readout_token_only=token_only, **flags).to(DEV))
    plain, flagged = out
    with torch.no_grad():                                              # biases and norm parameters off their trivial init
        g = torch.Generator().manual_seed(44)
        for name, p in plain.named_parameters():
            if name.endswith('bias') or name.startswith('norm'):
                p.add_((torch.randn(p.shape, generator=g) * 0.1).to(DEV, p.dtype))
    flagged.load_state_dict(plain.state_dict())
    return plain, flagged


@pytest.mark.parametrize('name', list(MODEL_FLAGS))
def test_flagged_model_is_the_unflagged_model(name):
    flags = MODEL_FLAGS[name]
    bf16 = name == 'bf16'
    tol = dict(atol=BF16_BAR, rtol=BF16_BAR, scaled=True) if bf16 else {}
    x, ei, idx, y, w = _model_data()
    data = types.SimpleNamespace(x=x.to(DEV), edge_index=ei.to(DEV), y=y.to(DEV), node_norm=w.to(DEV))
    idx = idx.to(DEV)
    plain, flagged = _models(flags)
    failures = []

    def hold(got, want, label):
        try:
            assert_close_scaled(_f64(got), _f64(want), f'{name} {label}', **tol)
        except AssertionError as e:
            failures.append(str(e))

    plain.eval(), flagged.eval()
    with torch.no_grad():
        hold(flagged(data, feature_indices=idx), plain(data, feature_indices=idx), 'log-probabilities')
    assert flagged.conv2_embedding.shape == (MN, MD) and plain.conv2_embedding.shape == (MN, ML * MD)
    assert flagged.conv1_embedding.shape == (MN, ML * MD)
    with pytest.raises(RuntimeError, match='forward_token'):
        flagged.attention_heatmap(layer='conv2')
    assert flagged.attention_heatmap(layer='conv1').shape == plain.attention_heatmap(layer='conv1').shape
    plain.train(), flagged.train()
    losses = []
    for model in (plain, flagged):
        loss = model.nll_loss(data, feature_indices=idx)
        loss.backward()
        losses.append(loss)
    hold(losses[1].reshape(1), losses[0].reshape(1), 'nll_loss')
    named = dict(flagged.named_parameters())
    for k, p in plain.named_parameters():
        if p.grad is None:                                             # cls_token: in the state dict, never used
            assert named[k].grad is None, k
            continue
        hold(named[k].grad, p.grad, f'{k}.grad')
    assert not failures, '\n'.join(failures)
