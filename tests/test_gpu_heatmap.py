"""GPU tests of the fused attention heatmap (csrc/attn_heatmap.hip through AMPConv.attention_heatmap / AMPGCN /
heatmap.AttentionHeatmap): the reference's calculate_attn_heatmap tables (tests/golden/heatmap/, flat fp32 tolerance of
SURVEY.md 8c), exact counts, bitwise equality of the two accumulation targets and of split / repeated updates, and
consistency with the layer's own attn_output_weights on seeded random layers."""
import os
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, load_golden, assert_close_scaled
from test_heatmap_cpu import HEATMAP_FIXTURES, heat_restatement, load_heatmap_fixture, class_selection

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                      # unit roundoff of fp32


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from ampnet_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _golden_layer(g, dev):
    from ampnet_amd import AMPConv
    layer = AMPConv(int(g['D']), int(g['H'])).to(dev)
    layer.load_state_dict({'multi_head_attention.in_proj_weight': torch.from_numpy(g['in_proj_weight']),
                           'multi_head_attention.in_proj_bias': torch.from_numpy(g['in_proj_bias']),
                           'multi_head_attention.out_proj.weight': torch.from_numpy(g['out_proj_weight']),
                           'multi_head_attention.out_proj.bias': torch.from_numpy(g['out_proj_bias'])})
    with torch.no_grad():
        layer(torch.from_numpy(g['x']).to(dev), torch.from_numpy(g['edge_index']).to(dev))
    return layer


@pytest.mark.parametrize('path', HEATMAP_FIXTURES, ids=[os.path.basename(p)[:-4] for p in HEATMAP_FIXTURES])
def test_golden_parity(path, dev):
    from ampnet_amd import AttentionHeatmap
    f, g = load_heatmap_fixture(path)
    layer = _golden_layer(g, dev)
    ei, tok = g['edge_index'], f['token_features']
    mask = torch.from_numpy(f['edge_mask']).to(dev)
    W = np.zeros((ei.shape[1],) + g['attn_output_weights'].shape[1:])
    W[g['w_edges']] = g['attn_output_weights']
    # class-filtered table of the selected features
    acc = AttentionHeatmap(f['src_features'], f['dst_features'])
    acc.update(layer, tok, edge_mask=mask, node_class=f['node_class'], src_class=int(f['src_class']),
               dst_class=int(f['dst_class']))
    _, cnt, _ = heat_restatement(W, tok, ei, f['src_features'], f['dst_features'], class_selection(f, ei))
    assert np.array_equal(acc.counts().cpu().numpy(), cnt)
    assert_close_scaled(acc.result().cpu().numpy(), f['heat_class'], 'heatmap (class pair)')
    # the convenience call gives the same table
    heat = layer.attention_heatmap(tok, f['src_features'], f['dst_features'], edge_mask=mask,
                                   node_class=f['node_class'], src_class=int(f['src_class']),
                                   dst_class=int(f['dst_class']))
    assert heat.dtype == torch.float64 and torch.equal(heat, acc.result())
    # all (weighted) edges, every feature in use
    acc = AttentionHeatmap(f['all_features']).update(layer, tok, edge_mask=mask)
    _, cnt, _ = heat_restatement(W, tok, ei, f['all_features'], f['all_features'], f['edge_mask'])
    assert np.array_equal(acc.counts().cpu().numpy(), cnt)
    assert_close_scaled(acc.result().cpu().numpy(), f['heat_all'], 'heatmap (all features)')


def _random_case(N, E, L, D, H, dev, seed, vocab=50, dtype=torch.float32):
    """A seeded layer after one forward pass on a graph with a hub node (long CSR and CSC segments) and 20 isolated
    nodes, and token features with repeats inside nodes."""
    from ampnet_amd import AMPConv
    torch.manual_seed(seed)
    layer = AMPConv(D, H).to(dev)
    with torch.no_grad():
        layer.multi_head_attention.in_proj_bias.normal_(0, 0.1)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(N, L * D, generator=g)
    ei = torch.randint(0, N - 20, (2, E), generator=g)
    ei[1, : E // 10] = 3
    ei[0, E // 10: E // 5] = 7
    tok = torch.randint(0, vocab, (N, L), generator=g)
    if dtype != torch.float32:
        layer = layer.to(dtype)
        x = x.to(dtype)
    layer.retain_attention = True
    with torch.no_grad():
        layer(x.to(dev), ei.to(dev))
    return layer, ei, tok


def _weight_bound(layer, L):
    """Bound on |w_heatmap - w_attn_output_weights| for one weight, hence for every mean of weights.  Both are the
    softmax of scores s = q.k / sqrt(dh) evaluated in fp32 from the SAME fp32 Q and K, in two summation orders: each
    score is within dh * EPS * |q||k| / sqrt(dh) =: d of the exact one, a softmax weight w <= 1 moves by at most
    w * 2 max|ds| <= 2 d per evaluation (4 d between the two), exp / reciprocal / normalisation / head mean add a few
    units of EPS on a value <= 1 (16 EPS allowed), and the fixed point adds 2^-(SHIFT+1)."""
    from ampnet_amd import heatmap
    layer.attn_output_weights                       # makes the retained buffer fp32
    buf = layer._attn_ctx[0]
    D, H = layer.embed_dim, layer.num_heads
    dh = D // H
    q = buf[:, :D].reshape(-1, H, dh).double().norm(dim=-1).max().item()
    k = buf[:, D:2 * D].reshape(-1, H, dh).double().norm(dim=-1).max().item()
    d = dh * EPS * q * k / dh ** 0.5
    return 4 * d + 16 * EPS + 2.0 ** -(heatmap.SHIFT + 1)


SHAPES = {'cora_L20_D128_H4': (300, 3000, 20, 128, 4), 'cfg3_L20_D128_H8': (300, 3000, 20, 128, 8),
          'L13_dh32': (200, 1500, 13, 128, 4), 'class_default_L40_D100_H2': (120, 700, 40, 100, 2),
          'L1': (200, 1500, 1, 128, 8)}


def _check_consistency(layer, ei, tok, vocab=50):
    from ampnet_amd import AttentionHeatmap
    L = tok.size(1)
    src = np.arange(0, vocab, 2)[:20]                               # 20 + 15 of the 50 ids: most tokens are skipped
    dst = np.arange(1, vocab, 3)[:15]
    sel = torch.rand(ei.size(1), generator=torch.Generator().manual_seed(5)) < 0.7
    acc = AttentionHeatmap(src, dst).update(layer, tok, edge_mask=sel.to(ei.device))
    bound = _weight_bound(layer, L)
    W = layer.attn_output_weights.cpu().numpy()
    _, cnt, heat = heat_restatement(W, tok.numpy(), ei.numpy(), src, dst, sel.numpy())
    assert np.array_equal(acc.counts().cpu().numpy(), cnt)
    assert cnt.sum() > 0
    err = np.abs(acc.result().cpu().numpy() - heat).max()
    print(f'[heatmap] max |fused - restatement(attn_output_weights)| = {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    # the full table (global accumulation) holds the same cells
    full = AttentionHeatmap(num_features=vocab).update(layer, tok, edge_mask=sel.to(ei.device))
    assert torch.equal(full.sum[src][:, dst], acc.sum) and torch.equal(full.cnt[src][:, dst], acc.cnt)


@pytest.mark.parametrize('name', list(SHAPES))
def test_consistent_with_attn_output_weights(name, dev):
    layer, ei, tok = _random_case(*SHAPES[name], dev, seed=11)
    _check_consistency(layer, ei, tok)


def test_consistent_with_attn_output_weights_bf16(dev):
    layer, ei, tok = _random_case(300, 3000, 20, 128, 4, dev, seed=12, dtype=torch.bfloat16)
    _check_consistency(layer, ei, tok)


def test_consistent_with_attn_output_weights_plane_format(dev, monkeypatch):
    from ampnet_amd.conv import functional as F_
    monkeypatch.setattr(F_, 'PROJ_SCALED_MIN_ELEMENTS', 0)
    layer, ei, tok = _random_case(300, 3000, 20, 128, 4, dev, seed=13)
    assert layer._attn_plane_bounds is not None, 'the retained buffer is not in the plane format'
    _check_consistency(layer, ei, tok)


@pytest.mark.parametrize('name', ['cora_L20_D128_H4', 'class_default_L40_D100_H2'])
def test_both_accumulation_targets_bitwise(name, dev, monkeypatch):
    from ampnet_amd import AttentionHeatmap
    layer, ei, tok = _random_case(*SHAPES[name], dev, seed=21)
    src, dst = np.arange(30), np.arange(20, 50)
    lds = AttentionHeatmap(src, dst).update(layer, tok)                  # 900 cells: per-workgroup LDS tables
    monkeypatch.setenv('AMPCONV_HEATMAP_GLOBAL', '1')
    glob = AttentionHeatmap(src, dst).update(layer, tok)                 # the same call, global atomics
    monkeypatch.delenv('AMPCONV_HEATMAP_GLOBAL')
    assert lds.cnt.sum().item() > 0
    assert torch.equal(lds.sum, glob.sum) and torch.equal(lds.cnt, glob.cnt)
    big = AttentionHeatmap(num_features=80).update(layer, tok)           # 6400 cells: global by size
    assert torch.equal(big.sum[src][:, dst], lds.sum) and torch.equal(big.cnt[src][:, dst], lds.cnt)


@pytest.mark.parametrize('name', ['cfg3_L20_D128_H8', 'class_default_L40_D100_H2'])
def test_additive_and_reproducible(name, dev):
    from ampnet_amd import AttentionHeatmap
    layer, ei, tok = _random_case(*SHAPES[name], dev, seed=31)
    E = ei.size(1)
    part = (torch.rand(E, generator=torch.Generator().manual_seed(1)) < 0.4).to(dev)
    feats = np.arange(5, 45)
    one = AttentionHeatmap(feats).update(layer, tok)
    again = AttentionHeatmap(feats).update(layer, tok)
    two = AttentionHeatmap(feats).update(layer, tok, edge_mask=part).update(layer, tok, edge_mask=~part)
    assert torch.equal(one.sum, again.sum) and torch.equal(one.cnt, again.cnt)
    assert torch.equal(one.sum, two.sum) and torch.equal(one.cnt, two.cnt)
    merged = AttentionHeatmap(feats).update(layer, tok, edge_mask=part)
    merged.merge(AttentionHeatmap(feats).update(layer, tok, edge_mask=~part))
    assert torch.equal(one.sum, merged.sum) and torch.equal(one.cnt, merged.cnt)
    assert one.triples == E * tok.size(1) ** 2 and two.triples == 2 * one.triples


def test_edge_cases(dev):
    from ampnet_amd import AMPConv, AttentionHeatmap
    layer, ei, tok = _random_case(100, 600, 20, 128, 4, dev, seed=41)
    none = torch.zeros(ei.size(1), dtype=torch.bool, device=dev)
    acc = AttentionHeatmap(np.arange(30)).update(layer, tok, edge_mask=none)           # no edge selected
    assert acc.cnt.sum().item() == 0 and acc.sum.sum().item() == 0 and (acc.result() == 0).all()
    acc = AttentionHeatmap([900, 901, 902]).update(layer, tok)                         # ids that never occur
    assert acc.cnt.sum().item() == 0 and (acc.result() == 0).all()
    with pytest.raises(ValueError):
        AttentionHeatmap(np.arange(30)).update(layer, tok, src_class=1)                # class without node_class
    with pytest.raises(ValueError):
        AttentionHeatmap(np.arange(30)).update(layer, tok[:, :5])
    # E = 0
    with torch.no_grad():
        layer(torch.randn(10, 20 * 128, device=dev), torch.zeros(2, 0, dtype=torch.int64, device=dev))
    acc = AttentionHeatmap(np.arange(30)).update(layer, tok[:10])
    assert acc.cnt.sum().item() == 0 and acc.triples == 0
    # a dropped projection buffer raises the existing message
    layer.retain_attention = False
    with torch.no_grad():
        layer(torch.randn(10, 20 * 128, device=dev), torch.randint(0, 10, (2, 30), device=dev))
    with pytest.raises(RuntimeError, match='was not retained'):
        layer.attention_heatmap(tok[:10], np.arange(30))
    lin = AMPConv(128, 4, softmax=False).to(dev)
    with torch.no_grad():
        lin(torch.randn(10, 20 * 128, device=dev), torch.randint(0, 10, (2, 30), device=dev))
    with pytest.raises(NotImplementedError):
        lin.attention_heatmap(tok[:10], np.arange(30))


def test_c_entry_argument_checks(dev):
    from ampnet_amd import _lib, heatmap
    lib = _lib.load()
    v = _lib.View(0, 0, 0, 0)
    t = torch.zeros(4, 4, dtype=torch.int64, device=dev)
    args = lambda **k: (v, v, None, k.get('E', 0), 0, None, None, None, 20, 128, 4, k.get('rows', 4), 4,  # noqa: E731
                        k.get('sum', t.data_ptr()), t.data_ptr(), k.get('prior', 0), k.get('dtype', _lib.AMPCONV_F32), None)
    assert lib.ampconv_attn_heatmap(*args()) == 0                                      # E == 0 is OK
    assert lib.ampconv_attn_heatmap(*args(dtype=_lib.AMPCONV_BF16)) == -2
    assert lib.ampconv_attn_heatmap(*args(sum=None)) == -1
    assert lib.ampconv_attn_heatmap(*args(sum=t.data_ptr() + 4)) == -1                 # misaligned
    assert lib.ampconv_attn_heatmap(*args(rows=0)) == -1
    assert lib.ampconv_attn_heatmap(*args(prior=heatmap.MAX_TRIPLES + 1)) == -1
    assert lib.ampconv_attn_heatmap(*args(E=1000, prior=heatmap.MAX_TRIPLES - 1000 * 400 + 1)) == -1   # would overflow
    assert lib.ampconv_attn_heatmap_shift() == heatmap.SHIFT


def _cfg_value(v):
    if v in ('True', 'False'):
        return v == 'True'
    if v == 'None':
        return None
    try:
        return int(v)
    except ValueError:
        return float(v)


def test_ampgcn_attention_heatmap(dev):
    from ampnet_amd import AMPGCN
    g = load_golden(os.path.join(GOLDEN_DIR, 'model_cora.npz'))
    cfg = {k: _cfg_value(v) for k, v in zip(g['cfg_keys'].tolist(), g['cfg_vals'].tolist())}
    model = AMPGCN(device=dev, **cfg).to(dev)
    model.load_state_dict({k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')})
    model.eval()
    data = types.SimpleNamespace(x=torch.from_numpy(g['x']).to(dev), edge_index=torch.from_numpy(g['edge_index']).to(dev))
    idx = torch.from_numpy(g['sampled_node_feat_indices']).to(dev)
    with torch.no_grad():
        model(data, feature_indices=idx)
    tok = model.sampled_node_feat_indices.cpu().numpy()
    ids, n = np.unique(tok, return_counts=True)
    src, dst = ids[np.argsort(-n)[:30]], ids[np.argsort(-n)[10:40]]
    cls = np.arange(tok.shape[0]) % 2
    sel = (cls[g['edge_index'][0]] == 0) & (cls[g['edge_index'][1]] == 1)
    heat = model.attention_heatmap('conv1', src, dst, node_class=cls, src_class=0, dst_class=1)
    W = model.conv1.attn_output_weights.cpu().numpy()
    _, cnt, want = heat_restatement(W, tok, g['edge_index'], src, dst, sel)
    assert cnt.sum() > 0
    bound = _weight_bound(model.conv1, tok.shape[1])
    err = np.abs(heat.cpu().numpy() - want).max()
    print(f'[heatmap] AMPGCN conv1: max err {err:.3e}, bound {bound:.3e}')
    assert err <= bound
    full = model.attention_heatmap('conv2')                                            # the full F x F table
    assert tuple(full.shape) == (model.num_node_features,) * 2
    _, _, want = heat_restatement(model.conv2.attn_output_weights.cpu().numpy(), tok, g['edge_index'], ids, ids)
    assert np.abs(full.cpu().numpy()[ids][:, ids] - want).max() <= _weight_bound(model.conv2, tok.shape[1])
