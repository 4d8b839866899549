"""CPU checks of the GCN baseline: known answers of the fp64 model (tests/gcn_reference.py) that pin the specification
-- PyG is not installed, the restated semantics of include/ampconv.h are what the kernels are held to -- and the host-side
classes: state-dict keys and shapes of the reference's GCN, initialisation, the ValueErrors."""
import math

import numpy as np
import pytest
import torch

import gcn_reference as R

# the reference's 5-node toy graph (testing_message_passing_pyg.py:24-33): 0, 1, 3, 4 -> 2
TOY = np.array([[0, 1, 3, 4], [2, 2, 2, 2]])


def _h(n=5, c=3, seed=0):
    return np.random.default_rng(seed).standard_normal((n, c))


def test_toy_graph_known_answer():
    h = _h()
    src, dst, norm, dinv = R.gcn_norm(TOY, 5)
    np.testing.assert_allclose(dinv ** -2.0, [1, 1, 5, 1, 1], rtol=1e-15)
    out = R.aggregate(h, TOY)
    np.testing.assert_allclose(out[2], (h[0] + h[1] + h[3] + h[4]) / math.sqrt(5) + h[2] / 5, rtol=1e-14, atol=1e-15)
    for n in (0, 1, 3, 4):
        np.testing.assert_allclose(out[n], h[n], rtol=1e-15)


def test_loops_collapse_and_duplicates_count():
    h = _h()
    twice = np.concatenate([TOY, [[2, 2], [2, 2]]], axis=1)                     # 2 -> 2 given twice
    np.testing.assert_array_equal(R.aggregate(h, twice), R.aggregate(h, TOY))
    dup = np.concatenate([TOY, [[0], [2]]], axis=1)                             # 0 -> 2 a second time
    _, _, _, dinv = R.gcn_norm(dup, 5)
    assert abs(dinv[2] ** -2.0 - 6.0) < 1e-14
    out = R.aggregate(h, dup)
    np.testing.assert_allclose(out[2], (2 * h[0] + h[1] + h[3] + h[4]) / math.sqrt(6) + h[2] / 6, rtol=1e-14, atol=1e-15)


def test_improved_doubles_the_loop_weight():
    h = _h()
    _, _, _, dinv = R.gcn_norm(TOY, 5, improved=True)
    np.testing.assert_allclose(dinv ** -2.0, [2, 2, 6, 2, 2], rtol=1e-15)
    out = R.aggregate(h, TOY, improved=True)
    np.testing.assert_allclose(out[2], (h[0] + h[1] + h[3] + h[4]) / math.sqrt(12) + 2 * h[2] / 6, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(out[0], h[0], rtol=1e-14)                        # 2 * h / 2


def test_no_self_loops_isolated_node_is_exactly_the_bias():
    h, bias = _h(6), np.array([0.5, -1.0, 2.0])
    ei = np.concatenate([TOY, [[2], [2]]], axis=1)                               # a loop is kept as an ordinary edge
    _, _, _, dinv = R.gcn_norm(ei, 6, add_self_loops=False)
    np.testing.assert_array_equal(dinv[[0, 1, 3, 4, 5]], 0.0)                    # no incoming edge: dinv = 0
    assert abs(dinv[2] ** -2.0 - 5.0) < 1e-14
    out = R.aggregate(h, ei, bias, add_self_loops=False)
    np.testing.assert_array_equal(out[5], bias)                                  # node 5 is isolated
    np.testing.assert_allclose(out[2], h[2] / 5 + bias, rtol=1e-14)              # sources with dinv = 0 give nothing


@pytest.mark.parametrize('improved, loops', [(False, True), (True, True), (False, False)])
def test_gradients_against_autograd_through_a_dense_operator(improved, loops):
    rng = np.random.default_rng(3)
    N, C = 12, 4
    ei = rng.integers(0, N, (2, 40))
    h, g, bias = rng.standard_normal((N, C)), rng.standard_normal((N, C)), rng.standard_normal(C)
    A = torch.from_numpy(R.dense_operator(ei, N, improved, loops))
    ht, bt = torch.from_numpy(h).requires_grad_(True), torch.from_numpy(bias).requires_grad_(True)
    out = A @ ht + bt
    out.backward(torch.from_numpy(g))
    np.testing.assert_allclose(R.aggregate(h, ei, bias, improved, loops), out.detach().numpy(), rtol=1e-12, atol=1e-13)
    dh, db = R.aggregate_backward(g, ei, improved, loops)
    np.testing.assert_allclose(dh, ht.grad.numpy(), rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(db, bt.grad.numpy(), rtol=1e-12, atol=1e-13)


def test_whole_model_gradients_against_autograd():
    rng = np.random.default_rng(5)
    N, F, De, Hd, C = 20, 6, 3, 4, 3
    x = (rng.random((N, F)) < 0.4).astype(np.float32)
    ei = rng.integers(0, N, (2, 60))
    y, nn_, mask = rng.integers(0, C, N), rng.random(N) + 0.5, rng.random(N) < 0.7
    P = {'feature_embedding_table.weight': rng.standard_normal((F, De)), 'conv1.lin.weight': rng.standard_normal((Hd, F * (De + 1))),
         'conv1.bias': rng.standard_normal(Hd), 'conv2.lin.weight': rng.standard_normal((C, Hd)), 'conv2.bias': rng.standard_normal(C)}
    ref = R.model(x, ei, P, 'embedded', y, nn_, mask)
    T = {k: torch.from_numpy(v).requires_grad_(True) for k, v in P.items()}
    A = torch.from_numpy(R.dense_operator(ei, N))
    z = torch.from_numpy(R.zscore(x))
    X0 = torch.cat([T['feature_embedding_table.weight'].unsqueeze(0).expand(N, F, De), z.unsqueeze(-1)], dim=2).reshape(N, -1)
    a1 = A @ (X0 @ T['conv1.lin.weight'].T) + T['conv1.bias']
    a2 = A @ (torch.relu(a1) @ T['conv2.lin.weight'].T) + T['conv2.bias']
    logp = torch.log_softmax(a2, dim=1)
    loss = (torch.nn.functional.nll_loss(logp, torch.from_numpy(y), reduction='none') * torch.from_numpy(nn_))[torch.from_numpy(mask)].sum()
    loss.backward()
    np.testing.assert_allclose(ref['logp'], logp.detach().numpy(), rtol=1e-11, atol=1e-12)
    assert abs(ref['loss'] - loss.item()) < 1e-10
    for k in P:
        np.testing.assert_allclose(ref['grads'][k], T[k].grad.numpy(), rtol=1e-10, atol=1e-11, err_msg=k)


@pytest.mark.parametrize('N, F, De, C', [(7, 5, 3, 4), (40, 33, 9, 5)])
def test_materialised_and_factored_input_agree(N, F, De, C):
    rng = np.random.default_rng(N)
    x = (rng.random((N, F)) < 0.3).astype(np.float32)
    x[:, 0] = 1.0                                                               # a constant column
    table, W = rng.standard_normal((F, De)), rng.standard_normal((C, F * (De + 1)))
    a, b = R.input_linear(x, W, table), R.input_linear_factored(x, W, table)
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())
    # and the gradients the kernels form from the factored expression
    g = rng.standard_normal((N, C))
    dW, dtable = R.input_linear_backward(x, W, table, g)
    s, z, W3 = g.sum(axis=0), R.zscore(x), W.reshape(C, F, De + 1)
    fW = np.concatenate([s[:, None, None] * table[None], (g.T @ z)[:, :, None]], axis=2).reshape(C, -1)
    np.testing.assert_allclose(dW, fW, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(dtable, np.einsum('j,jfk->fk', s, W3[:, :, :De]), rtol=1e-12, atol=1e-12)


def test_gcnconv_state_dict_and_init():
    from ampnet_amd import GCNConv
    torch.manual_seed(0)
    m = GCNConv(24, 6)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {'bias': (6,), 'lin.weight': (6, 24)}
    assert list(m.state_dict()) == ['bias', 'lin.weight']
    bound = math.sqrt(6.0 / (24 + 6))
    assert float(m.lin.weight.abs().max()) <= bound and float(m.lin.weight.abs().max()) > 0.5 * bound
    assert torch.equal(m.bias, torch.zeros(6))
    assert m.improved is False and m.add_self_loops is True
    assert list(GCNConv(3, 2, bias=False).state_dict()) == ['lin.weight']
    with pytest.raises(ValueError, match='normalize=False'):
        GCNConv(3, 2, normalize=False)
    with pytest.raises(ValueError, match='GPU'):
        m(torch.randn(4, 24), torch.tensor([[0], [1]]))


@pytest.mark.parametrize('mode, cols', [('embedded', 8 * 5), ('zscore', 8), ('raw', 8)])
def test_gcn_state_dict_equals_the_reference_class(mode, cols):
    from ampnet_amd import GCN
    m = GCN('cpu', num_node_features=8, hidden_dim=3, num_sampled_vectors=8, output_dim=2, feat_emb_dim=4, input=mode)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {
        'feature_embedding_table.weight': (8, 4), 'conv1.bias': (3,), 'conv1.lin.weight': (3, cols),
        'conv2.bias': (2,), 'conv2.lin.weight': (2, 3)}
    assert list(m.state_dict()) == ['feature_embedding_table.weight', 'conv1.bias', 'conv1.lin.weight', 'conv2.bias',
                                    'conv2.lin.weight']                          # PyG's order: bias before lin.weight
    assert float(m.conv1.lin.weight.abs().max()) <= math.sqrt(6.0 / (cols + 3))
    assert torch.equal(m.conv1.bias, torch.zeros(3)) and torch.equal(m.conv2.bias, torch.zeros(2))


def test_gcn_constructor_follows_the_reference_argument_order():
    import inspect
    from ampnet_amd import GCN
    names = list(inspect.signature(GCN.__init__).parameters)[1:]
    assert names[:11] == ['device', 'num_node_features', 'hidden_dim', 'num_sampled_vectors', 'output_dim', 'softmax_out',
                          'feat_emb_dim', 'val_emb_dim', 'downsample_feature_vectors', 'dropout_rate', 'dropout_adj_rate']
    kinds = inspect.signature(GCN.__init__).parameters
    assert all(kinds[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ('input', 'seed', 'fused_glue', 'fused_head'))


def test_gcn_value_errors():
    from ampnet_amd import GCN
    with pytest.raises(ValueError, match=r'gcn_classifier\.py:106'):
        GCN('cpu')                                                              # the reference's own defaults: 40 vs 1433
    GCN('cpu', input='zscore')                                                  # no reshape there: the defaults are fine
    with pytest.raises(ValueError, match='val_emb_dim'):
        GCN('cpu', num_sampled_vectors=1433, val_emb_dim=2)
    with pytest.raises(ValueError, match='input must be'):
        GCN('cpu', input='pca')
    m = GCN('cpu', num_node_features=4, num_sampled_vectors=4, feat_emb_dim=2, softmax_out=False)
    with pytest.raises(ValueError, match='softmax_out'):
        m.nll_loss(None)
    import types
    with pytest.raises(ValueError, match='GPU'):
        m(types.SimpleNamespace(x=torch.zeros(3, 4), edge_index=torch.zeros(2, 1, dtype=torch.int64)))
    with pytest.raises(ValueError, match='fused_head'):
        GCN('cpu', input='raw', output_dim=65, fused_head=True)


def test_gcn_functions_refuse_cpu_and_other_dtypes():
    from ampnet_amd import gcn_aggregate, gcn_norm
    from ampnet_amd.gcn import LONG_SEGMENT, gcn_input_linear
    assert LONG_SEGMENT == 256
    with pytest.raises(ValueError, match='GPU'):
        gcn_aggregate(torch.zeros(3, 2), torch.zeros(2, 1, dtype=torch.int64))
    with pytest.raises(ValueError, match='GPU'):
        gcn_norm(torch.zeros(2, 1, dtype=torch.int64), 3)                        # EdgeCSR's own error
    with pytest.raises(ValueError, match='GPU'):
        gcn_input_linear(torch.zeros(3, 2), torch.zeros(4, 2))
