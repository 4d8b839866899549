"""The read-out-token path on the CPU: the identity the one-query-token kernels rest on (the fp64 edge model fed ONE
query row equals the full model sliced to that row), AMPGCN(readout_token_only=True)'s validation and walk with
stand-ins as in tests/test_ampgcn_walk_cpu.py, and AMPConv.forward_token's argument check.  No kernel runs here."""
import numpy as np
import pytest
import torch

import edge_reference as er
from test_ampgcn_walk_cpu import D, L, N, SITE_FLAGS, _Conv, _model

WALK_TOKEN = ['tokens', 'entry.call', 'conv1', 'between.call', 'conv2.forward_token', 'readout.call']


def _graph(name):
    """Graphs A and B of tests/edge_runner.py without importing it (it loads the GPU library's binding)."""
    if name == 'A':
        rng = np.random.default_rng(11)
        src = [np.arange(150) % 50, np.full(150, 7), rng.permutation(np.tile(np.arange(50), 8)), [3, 5, 7]]
        d = rng.integers(0, 57, 400)
        dst = [np.full(150, 3), np.arange(150) % 50, d + (d >= 50), [3, 5, 7]]
        return np.concatenate(src), np.concatenate(dst), 64
    rng = np.random.default_rng(12)
    src = rng.permutation(np.repeat(np.arange(40), np.arange(40) % 10))[:160]
    dst = rng.permutation(np.repeat(np.arange(36), np.arange(36) % 9 + 1))[:160]
    src[:4], dst[:4] = [1, 1, 9, 34], [2, 2, 9, 35]
    return src, dst, 40


@pytest.mark.parametrize('gname', ['A', 'B'])
@pytest.mark.parametrize('shape', [(5, 6, 3), (17, 16, 2)], ids=lambda s: 'L%ddh%dH%d' % s)
def test_one_query_row_is_the_sliced_model(gname, shape):
    """er.fwd / er.bwd with Q and dObar of ONE token against K, V of L tokens = the full model's token t: O and dQ are
    its rows; dK and dV are those of a full backward pass whose dObar is zero at every other token."""
    Lt, dh, H = shape
    src, dst, n = _graph(gname)
    rowptr, col = er.csr_of(src, dst, n)
    rng = np.random.default_rng(7)
    Q, K, V, dO = (rng.standard_normal((n, Lt, H, dh)) for _ in range(4))
    O_full = er.fwd(Q, K, V, rowptr, col)
    for t in (0, Lt - 1):
        sl = slice(t, t + 1)
        np.testing.assert_allclose(er.fwd(Q[:, sl], K, V, rowptr, col), O_full[:, sl], rtol=0, atol=1e-13)
        only_t = np.zeros_like(dO)
        only_t[:, sl] = dO[:, sl]
        dQ_full, dK_full, dV_full = er.bwd(Q, K, V, only_t, rowptr, col)
        dQ, dK, dV = er.bwd(Q[:, sl], K, V, dO[:, sl], rowptr, col)
        assert dQ.shape == (n, 1, H, dh) and dK.shape == dV.shape == (n, Lt, H, dh)
        np.testing.assert_allclose(dQ, dQ_full[:, sl], rtol=0, atol=1e-13)
        np.testing.assert_allclose(dK, dK_full, rtol=0, atol=1e-12)
        np.testing.assert_allclose(dV, dV_full, rtol=0, atol=1e-12)
        assert not np.delete(dQ_full, t, axis=1).any()


def test_readout_token_only_needs_token0_pooling():
    from ampnet_amd import AMPGCN
    with pytest.raises(ValueError, match='average_pooling_flag=False'):
        AMPGCN(device='cpu', embedding_dim=D, num_heads=2, num_node_features=12, num_sampled_vectors=L, feat_emb_dim=D - 1,
               output_dim=3, average_pooling_flag=True, readout_token_only=True)
    m = AMPGCN(device='cpu', embedding_dim=D, num_heads=2, num_node_features=12, num_sampled_vectors=L, feat_emb_dim=D - 1,
               output_dim=3, average_pooling_flag=False, readout_token_only=True)
    assert m.readout_token_only is True
    assert 'cls_token' in m.state_dict()                   # the state dict is the unflagged model's


class _TokenConv(_Conv):
    """conv2's stand-in: forward_token writes its own name and hands token `token` of its input on."""

    def forward_token(self, x, edge_index, token=0):
        self.log.append(self.name + '.forward_token')
        self.tokens = getattr(self, 'tokens', []) + [token]
        return x.reshape(x.shape[0], -1, D)[:, token]


class _SeesShape:
    """Wraps a site stand-in and records the shape it was called with."""

    def __init__(self, inner):
        self.inner, self.shapes = inner, []

    def __call__(self, x):
        self.shapes.append(tuple(x.shape))
        return self.inner(x)

    def activate(self, x):
        return self.inner.activate(x)


@pytest.mark.parametrize('name', list(SITE_FLAGS))
def test_flagged_walk_calls_forward_token_once(name):
    model, data, log, _ = _model(SITE_FLAGS[name], False, readout_token_only=True)
    model.conv2 = _TokenConv('conv2', log)
    readout = _SeesShape(model._sites[2])
    model._sites = model._sites[:2] + (readout,)
    for training in (True, False):
        model.train(training)
        del log[:]
        out = model._run(data)
        assert log == WALK_TOKEN, (training, log)
        assert log.count('conv2.forward_token') == 1 and 'conv2' not in log
        assert readout.shapes[-1] == (N, D)                 # the readout site sees ONE token
        assert out.shape == (N, D) and model.conv2_embedding.shape == (N, D) and model.conv1_embedding.shape == (N, L * D)
    assert model.conv2.tokens == [0, 0]
    sites = {}
    model._run(data, None, sites)
    assert sites['AmpConv 2'].shape == (N, D) and sites[list(sites)[3]].shape == (N, D)


def test_flagged_plain_walk_is_the_unflagged_one_in_eval_mode():
    """The real _TorchSite readout on [N, D]: token0 pooling over L = 1 gives what the unflagged walk reads."""
    flagged, data, log, _ = _model({}, False, readout_token_only=True)
    flagged.conv2 = _TokenConv('conv2', log)
    plain, _, _, _ = _model({}, False)
    flagged.eval(), plain.eval()
    assert torch.equal(flagged._run(data), plain._run(data))


@pytest.mark.parametrize('name', list(SITE_FLAGS))
@pytest.mark.parametrize('mean', [True, False], ids=['mean', 'token0'])
def test_default_walk_never_calls_forward_token(name, mean):
    model, data, log, _ = _model(SITE_FLAGS[name], mean)
    assert model.readout_token_only is False
    model.conv2 = _TokenConv('conv2', log)
    model._run(data)
    assert 'conv2.forward_token' not in log and log.count('conv2') == 1


def test_forward_token_validates_token(monkeypatch):
    from ampnet_amd import AMPConv
    layer = AMPConv(8, 2)
    monkeypatch.setattr(layer, '_check_x', lambda x, name='x': None)       # (the device check: there is no GPU here)
    x, ei = torch.zeros(4, 5 * 8), torch.zeros(2, 3, dtype=torch.int64)
    for bad in (-1, 5, 40):
        with pytest.raises(ValueError, match=r'token must be in \[0, 5\)'):
            layer.forward_token(x, ei, bad)
    with pytest.raises(ValueError, match='GPU only'):                     # ... and its inputs like forward does
        AMPConv(8, 2).forward_token(x, ei, 0)
