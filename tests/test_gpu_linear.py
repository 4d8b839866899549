"""GPU parity of the softmax-free AMPConv variant (ampnet_amd/conv/linear.py):
against the outputs of the reference's own softmax-free attention class (tests/golden/linear_*.npz,
written by oracle/make_golden.py from custom_multihead_attn.py) and against the per-edge numpy
oracle on seeded graphs.  Same fp32 tolerance as the softmax path."""
import os

import numpy as np
import pytest
import torch

from conftest import golden_files, load_golden, assert_close_scaled

pytestmark = pytest.mark.gpu

LINEAR = golden_files(linear=True)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from ampnet_amd import _lib
    _lib.load()
    return torch.device('cuda:0')


def _layer(g, dev):
    from ampnet_amd import AMPConv
    layer = AMPConv(int(g['D']), int(g['H']), softmax=False).to(dev)
    layer.load_state_dict({'multi_head_attention.in_proj_weight': torch.from_numpy(g['in_proj_weight']),
                           'multi_head_attention.in_proj_bias': torch.from_numpy(g['in_proj_bias']),
                           'multi_head_attention.out_proj.weight': torch.from_numpy(g['out_proj_weight']),
                           'multi_head_attention.out_proj.bias': torch.from_numpy(g['out_proj_bias'])})
    return layer


def _grads(layer):
    m = layer.multi_head_attention
    return [t.grad.cpu().numpy() for t in (m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias)]


@pytest.mark.parametrize('path', LINEAR, ids=[os.path.basename(p)[:-4] for p in LINEAR])
def test_golden_softmax_free(path, dev):
    g = load_golden(path)
    layer = _layer(g, dev)
    x = torch.from_numpy(g['x']).to(dev).requires_grad_(True)
    ei = torch.from_numpy(g['edge_index']).to(dev)
    y = layer(x, ei)
    (y * torch.from_numpy(g['dy']).to(dev)).sum().backward()
    yh = y.detach().cpu().numpy()
    assert_close_scaled(yh, g['y'], 'y')
    deg = np.bincount(g['edge_index'][1], minlength=int(g['N']))
    assert (yh[deg == 0] == 0).all()
    assert_close_scaled(x.grad.cpu().numpy(), g['dx'], 'dx')
    for got, name in zip(_grads(layer), ('g_in_proj_weight', 'g_in_proj_bias', 'g_out_proj_weight', 'g_out_proj_bias')):
        assert_close_scaled(got, g[name], name)
    w = layer.attn_output_weights.cpu().numpy()
    assert_close_scaled(w[g['w_edges']], g['attn_output_weights'], 'attn_output_weights')
    ao = layer.attn_output.cpu().numpy()
    assert_close_scaled(ao[g['w_edges'][:4]], g['attn_output'], 'attn_output')


@pytest.mark.parametrize('shape', [(1500, 14000, 20, 128, 4), (900, 8000, 20, 256, 8), (300, 2500, 40, 100, 2)],
                         ids=['D128', 'D256', 'L40_dh50'])
def test_seeded_vs_oracle_softmax_free(shape, dev):
    from ampnet_amd import AMPConv
    from oracle.ampconv_numpy import AMPConvOracle
    N, E, L, D, H = shape
    g = torch.Generator().manual_seed(N + E)
    ei = torch.randint(0, N, (2, E), generator=g)
    ei[1, : E // 8] = 3                              # a hub destination
    ei[0, E // 8: E // 4] = 5                        # a hub source
    ei[1, ei[1] == 7] = 8                            # node 7 receives nothing
    x = torch.randn(N, L * D, generator=g) * 0.5
    dy = torch.randn(N, L * D, generator=g)
    torch.manual_seed(5)
    layer = AMPConv(D, H, softmax=False).to(dev)
    with torch.no_grad():
        layer.multi_head_attention.in_proj_bias.normal_(0, 0.1)
        layer.multi_head_attention.out_proj.bias.normal_(0, 0.1)
    xg = x.to(dev).requires_grad_(True)
    y = layer(xg, ei.to(dev))
    y.backward(dy.to(dev))
    m = layer.multi_head_attention
    o = AMPConvOracle(m.in_proj_weight.detach().cpu().numpy(), m.in_proj_bias.detach().cpu().numpy(),
                      m.out_proj.weight.detach().cpu().numpy(), m.out_proj.bias.detach().cpu().numpy(), H,
                      softmax=False)
    y_ref, _ = o.forward(x.numpy(), ei.numpy(), need_weights=False)
    ref = o.backward(dy.numpy())
    yh = y.detach().cpu().numpy()
    assert_close_scaled(yh, y_ref, 'y')
    assert (yh[7] == 0).all()
    assert_close_scaled(xg.grad.cpu().numpy(), ref[0], 'dx')
    for got, want, name in zip(_grads(layer), ref[1:], ('gW_in', 'gb_in', 'gW_out', 'gb_out')):
        assert_close_scaled(got, want, name)


def test_message_softmax_free(dev):
    # message(x_i, x_j) on pre-gathered pairs = per-edge softmax-free attention + out-projection
    from ampnet_amd import AMPConv
    from oracle.ampconv_numpy import AMPConvOracle
    E, L, D, H = 60, 6, 32, 4
    g = torch.Generator().manual_seed(3)
    x_i, x_j = torch.randn(E, L * D, generator=g), torch.randn(E, L * D, generator=g)
    torch.manual_seed(9)
    layer = AMPConv(D, H, softmax=False).to(dev)
    out = layer.message(x_i.to(dev), x_j.to(dev)).detach().cpu().numpy()
    m = layer.multi_head_attention
    o = AMPConvOracle(m.in_proj_weight.detach().cpu().numpy(), m.in_proj_bias.detach().cpu().numpy(),
                      m.out_proj.weight.detach().cpu().numpy(), m.out_proj.bias.detach().cpu().numpy(), H,
                      softmax=False)
    # graph with 2E nodes: edge e goes from node E + e (x_j) to node e (x_i)
    xx = np.concatenate([x_i.numpy(), x_j.numpy()])
    ei = np.stack([np.arange(E) + E, np.arange(E)])
    y_ref, _ = o.forward(xx, ei, need_weights=False)
    assert_close_scaled(out, y_ref[:E], 'message')


def test_gather_segment_sum_rejects_bad_arguments(dev):
    from ampnet_amd import _lib
    lib = _lib.load()
    t = torch.zeros(8, device=dev)
    p = torch.zeros(2, dtype=torch.int32, device=dev)
    assert lib.ampconv_gather_segment_sum(t.data_ptr(), p.data_ptr(), p.data_ptr(), None, 0, 1, 6,
                                          t.data_ptr(), None) == -1     # AMPCONV_E_BADARG: F % 4 != 0
    assert lib.ampconv_gather_segment_sum(None, p.data_ptr(), p.data_ptr(), None, 0, 1, 8,
                                          t.data_ptr(), None) == -1


# ------------------------------------------------------------------------------- layer level, against the fp64 oracle
GRAD_LABELS = ('gW_in', 'gb_in', 'gW_out', 'gb_out')
SMALL_SHAPES = [(1, 8, 4), (5, 12, 2), (7, 24, 4), (33, 48, 3), (20, 128, 4), (40, 100, 2), (64, 64, 1)]


def _small_graph():
    """60 nodes, 400 edges in random order: node 3 receives 50 edges, node 5 sends 50, self-loops on 7, 8, 9, the edge
    10 -> 11 twice, nodes 54..59 isolated."""
    N, E = 60, 400
    rng = np.random.default_rng(60400)
    src, dst = rng.integers(0, 54, E), rng.integers(0, 54, E)
    dst[:50] = 3
    src[50:100] = 5
    src[100:103] = dst[100:103] = [7, 8, 9]
    src[103:105], dst[103:105] = 10, 11
    order = rng.permutation(E)
    return N, np.stack([src[order], dst[order]])


def _linear_layer(D, H, dev, seed=5):
    from ampnet_amd import AMPConv
    torch.manual_seed(seed)
    layer = AMPConv(D, H, softmax=False).to(dev)
    with torch.no_grad():
        layer.multi_head_attention.in_proj_bias.normal_(0, 0.1)
        layer.multi_head_attention.out_proj.bias.normal_(0, 0.1)
    return layer


def _oracle(layer, H):
    from oracle.ampconv_numpy import AMPConvOracle
    m = layer.multi_head_attention
    return AMPConvOracle(m.in_proj_weight.detach().cpu().numpy(), m.in_proj_bias.detach().cpu().numpy(),
                         m.out_proj.weight.detach().cpu().numpy(), m.out_proj.bias.detach().cpu().numpy(), H, softmax=False)


def _inputs(N, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, L * D, generator=g) * 0.5, torch.randn(N, L * D, generator=g)


@pytest.mark.parametrize('shape', SMALL_SHAPES, ids=lambda s: 'L{}_D{}_H{}'.format(*s))
def test_small_shapes_vs_oracle_softmax_free(shape, dev):
    """One token, dh = 2, 6, 16 (three heads), 32, 50 and 64.  The bars are the existing labels' (y, dx flat; parameter
    gradients scaled): on this graph a float32 run of the oracle against its float64 run uses at most 9.8 % of them
    (dx at (64, 64, 1)), so they leave a correct fp32 implementation a tenfold margin and need no new number."""
    L, D, H = shape
    N, ei = _small_graph()
    x, dy = _inputs(N, L, D, 1000 * L + D)
    layer = _linear_layer(D, H, dev)
    xg = x.to(dev).requires_grad_(True)
    y = layer(xg, torch.from_numpy(ei).to(dev))
    y.backward(dy.to(dev))
    o = _oracle(layer, H)
    y_ref, _ = o.forward(x.numpy(), ei, need_weights=False)
    ref = o.backward(dy.numpy())
    yh = y.detach().cpu().numpy()
    assert_close_scaled(yh, y_ref, 'y')
    assert not yh[54:].any() and not yh[np.bincount(ei[1], minlength=N) == 0].any()
    assert_close_scaled(xg.grad.cpu().numpy(), ref[0], 'dx')
    for got, want, name in zip(_grads(layer), ref[1:], GRAD_LABELS):
        assert_close_scaled(got, want, name)


@pytest.mark.parametrize('shape', [(6, 32, 4), (40, 100, 2)], ids=lambda s: 'L{}_D{}_H{}'.format(*s))
def test_message_softmax_free_gradients(shape, dev):
    """LinearAMPConvFunction's bipartite branch (shared=False: the Q and the K | V projections apart, dq2 / dkv, two
    weight-gradient blocks), forward and backward, on the 2 E-node graph of test_message_softmax_free."""
    L, D, H = shape
    E = 60
    g = torch.Generator().manual_seed(3)
    x_i, x_j = torch.randn(E, L * D, generator=g) * 0.5, torch.randn(E, L * D, generator=g) * 0.5
    dy = torch.randn(E, L * D, generator=g)
    layer = _linear_layer(D, H, dev, seed=9)
    xi, xj = x_i.to(dev).requires_grad_(True), x_j.to(dev).requires_grad_(True)
    out = layer.message(xi, xj)
    out.backward(dy.to(dev))
    o = _oracle(layer, H)
    ei = np.stack([np.arange(E) + E, np.arange(E)])
    y_ref, _ = o.forward(np.concatenate([x_i.numpy(), x_j.numpy()]), ei, need_weights=False)
    ref = o.backward(np.concatenate([dy.numpy(), np.zeros_like(dy.numpy())]))
    assert_close_scaled(out.detach().cpu().numpy(), y_ref[:E], 'message')
    assert_close_scaled(xi.grad.cpu().numpy(), ref[0][:E], 'dx_i')
    assert_close_scaled(xj.grad.cpu().numpy(), ref[0][E:], 'dx_j')
    for got, want, name in zip(_grads(layer), ref[1:], GRAD_LABELS):
        assert_close_scaled(got, want, name)


def test_message_aggregate_match_fused_softmax_free(dev):
    """message() -> aggregate() equals the fused propagate, outputs and every gradient, at the bar
    test_message_aggregate_gradients_match_fused holds the softmax path to."""
    N, E, L, D, H = 40, 300, 20, 128, 4
    layer = _linear_layer(D, H, dev, seed=3)
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(N, L * D, generator=g) * 0.5).to(dev)
    dy = torch.randn(N, L * D, generator=g).to(dev)
    ei = torch.randint(0, N, (2, E), generator=g).to(dev)
    ei[1, ei[1] == 3] = 4                                      # node 3 receives nothing
    xa = x.clone().requires_grad_(True)
    ya = layer(xa, ei)
    ya.backward(dy)
    ga = [xa.grad.clone()] + [p.grad.clone() for p in layer.parameters()]
    layer.zero_grad(set_to_none=True)
    xb = x.clone().requires_grad_(True)
    msg = layer.message(xb.index_select(0, ei[1]), xb.index_select(0, ei[0]))
    yb = layer.aggregate(msg, ei[1], dim_size=N)
    assert yb.requires_grad
    yb.backward(dy)
    gb = [xb.grad] + [p.grad for p in layer.parameters()]
    assert_close_scaled(yb.detach().cpu().numpy(), ya.detach().cpu().numpy(), 'y (message+aggregate vs fused)')
    assert (yb[3] == 0).all()
    for name, a, b in zip(['dx', 'g_in_w', 'g_in_b', 'g_out_w', 'g_out_b'], ga, gb):
        assert_close_scaled(b.cpu().numpy(), a.cpu().numpy(), name + ' (message+aggregate vs fused)')


@pytest.mark.parametrize('N', [1, 12])
def test_softmax_free_without_edges(N, dev):
    """An empty edge set: every node is isolated, y = 0, dx = 0, the out-projection's bias receives no gradient, and
    the per-edge side output has no rows."""
    L, D, H = 5, 12, 2
    x, dy = _inputs(N, L, D, 7)
    layer = _linear_layer(D, H, dev)
    xg = x.to(dev).requires_grad_(True)
    y = layer(xg, torch.zeros(2, 0, dtype=torch.int64, device=dev))
    y.backward(dy.to(dev))
    assert tuple(y.shape) == (N, L * D) and not y.any() and not xg.grad.any()
    assert not layer.multi_head_attention.out_proj.bias.grad.any()
    assert tuple(layer.attn_output_weights.shape) == (0, L, L)


def test_softmax_free_is_deterministic(dev):
    L, D, H = 20, 128, 4
    N, ei = _small_graph()
    x, dy = _inputs(N, L, D, 11)
    layer = _linear_layer(D, H, dev)
    runs = []
    for _ in range(2):
        layer.zero_grad(set_to_none=True)
        xg = x.to(dev).requires_grad_(True)
        y = layer(xg, torch.from_numpy(ei).to(dev))
        y.backward(dy.to(dev))
        runs.append([y.detach().clone(), xg.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize('shape', [(5, 12, 2), (20, 128, 4)], ids=lambda s: 'L{}_D{}_H{}'.format(*s))
def test_side_outputs_softmax_free(shape, dev):
    """attn_output_weights (the head mean of the raw scaled scores) and attn_output in the ORIGINAL, shuffled edge
    order against the oracle's need_weights output."""
    L, D, H = shape
    N, ei = _small_graph()
    x, _ = _inputs(N, L, D, 13)
    layer = _linear_layer(D, H, dev)
    with torch.no_grad():
        layer(x.to(dev), torch.from_numpy(ei).to(dev))
    o = _oracle(layer, H)
    _, w_ref = o.forward(x.numpy(), ei, need_weights=True)
    assert_close_scaled(layer.attn_output_weights.cpu().numpy(), w_ref, 'attn_output_weights')
    assert_close_scaled(layer.attn_output.cpu().numpy(), o.attn_output(), 'attn_output')


def test_softmax_free_refuses_what_it_cannot_compute(dev):
    from ampnet_amd import AMPConv, _lib
    ei = torch.tensor([[0, 1, 2], [1, 2, 0]], device=dev)
    with pytest.raises(ValueError):                             # an odd head width
        AMPConv(9, 3, softmax=False).to(dev)(torch.randn(4, 2 * 9, device=dev), ei)
    with pytest.raises(ValueError):                             # bf16 rows
        AMPConv(8, 2, softmax=False).to(dev)(torch.randn(4, 2 * 8, device=dev).bfloat16(), ei)
    # dh = 128: ampconv_linear_apply would need (L + 128) * 129 * 4 bytes of LDS, more than its 64 KiB at any L
    with pytest.raises(_lib.AmpconvError, match='ampconv_linear_apply'):
        AMPConv(128, 1, softmax=False).to(dev)(torch.randn(4, 2 * 128, device=dev), ei)
