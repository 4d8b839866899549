"""AMPGCN's layer walk (_run) on the CPU: the three site configurations x both poolings, with conv1, conv2, the token
builder and the site objects replaced by stand-ins that write their name into a log and hand their input on.  The fused
sites (ampnet_amd/glue.py, norm.py) need the GPU, so they are replaced outright; the unfused model's adapters around
drop1 / drop2 / drop3 are PyTorch ops and are wrapped, so their own code runs.  What is held: the ONE sequence, the same
for training, eval and the recording pass; that forward, nll_loss, _pooled and activation_stats reach it through _run alone;
and that the unfused walk is drop3(relu(drop2(relu(drop1(x))))) pooled, bit for bit, under torch's generator."""
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

N, L, D = 6, 5, 16
SITE_FLAGS = {'plain': {}, 'fused_glue': {'fused_glue': True}, 'layer_norm': {'layer_norm': True}}
WALK = ['tokens', 'entry.call', 'conv1', 'between.call', 'conv2', 'readout.call']


class _Conv(nn.Module):
    """conv1 / conv2 are registered sub-modules, so their stand-in is one; its parameter answers _check_storage."""

    def __init__(self, name, log):
        super().__init__()
        self.name, self.log, self.anchor = name, log, nn.Parameter(torch.zeros(1))

    def forward(self, x, edge_index):
        self.log.append(self.name)
        return x


class _Tokens:
    def __init__(self, log):
        self.log = log

    def __call__(self, x, idx=None):
        self.log.append('tokens')
        return x, idx

    def forward_all(self, x, feature_repeats):
        self.log.append('tokens')
        return x, None


class _Site:
    """inner: the real adapter of the unfused model (its code runs); None for a fused site: the input comes back, cut to
    `width` columns where the site pools."""

    def __init__(self, name, log, inner=None, width=None):
        self.name, self.log, self.inner, self.width = name, log, inner, width

    def __call__(self, x):
        self.log.append(self.name + '.call')
        if self.inner is not None:
            return self.inner(x)
        return x if self.width is None else x[:, :self.width]

    def activate(self, x):
        self.log.append(self.name + '.activate')
        return x if self.inner is None else self.inner.activate(x)


def _model(flags, mean, **kw):
    from ampnet_amd import AMPGCN
    from ampnet_amd.module.amp_gcn import _TorchSite
    torch.manual_seed(0)
    model = AMPGCN(device='cpu', embedding_dim=D, num_heads=2, num_node_features=12, num_sampled_vectors=L, feat_emb_dim=D - 1,
                   output_dim=3, average_pooling_flag=mean, **flags, **kw)
    log = []
    model.conv1, model.conv2, model._tokens[0] = _Conv('conv1', log), _Conv('conv2', log), _Tokens(log)
    real = model._sites
    model._sites = tuple(_Site(name, log, site if isinstance(site, _TorchSite) else None, D if name == 'readout' else None)
                         for name, site in zip(('entry', 'between', 'readout'), real))
    g = torch.Generator().manual_seed(1)
    data = types.SimpleNamespace(x=torch.randn(N, L * D, generator=g), edge_index=torch.randint(0, N, (2, 40), generator=g),
                                 y=torch.randint(0, 3, (N,), generator=g))
    return model, data, log, real


@pytest.mark.parametrize('mean', [True, False], ids=['mean', 'token0'])
@pytest.mark.parametrize('name', list(SITE_FLAGS))
def test_one_sequence_for_training_eval_and_recording(name, mean):
    from ampnet_amd.module.amp_gcn import _TorchSite
    model, data, log, real = _model(SITE_FLAGS[name], mean)
    # which objects the constructor picked
    if name == 'plain':
        assert all(isinstance(s, _TorchSite) for s in real)
        assert [s.drop for s in real] == [model.drop1, model.drop2, model.drop3] and model._glue == []
    elif name == 'fused_glue':
        assert real == tuple(model._glue) and [s._site for s in real] == [1, 2, 3]
    else:
        assert isinstance(real[0], _TorchSite) and real[0].drop is model.drop1 and real[1:] == (model.norm1, model.norm2)
        assert (model.norm1._site, model.norm2._site) == (4, 5)
    for training in (True, False):
        model.train(training)
        del log[:]
        out = model._run(data)
        assert log == WALK, (training, log)
        assert out.shape == (N, D) and model.conv1_embedding.shape == model.conv2_embedding.shape == (N, L * D)
        assert all(s.training == training for s in model._glue)
    act = 'LayerNorm+ReLU' if name == 'layer_norm' else 'ReLU'
    for training in (True, False):
        model.train(training)
        del log[:]
        sites = {}
        out = model._run(data, None, sites)
        assert [e for e in log if not e.endswith('.activate')] == WALK, log
        assert [e for e in log if e.endswith('.activate')] == ['between.activate', 'readout.activate'], log
        assert log.index('conv1') < log.index('between.activate') and log.index('conv2') < log.index('readout.activate')
        assert list(sites) == ['AmpConv 1', act + ' 1', 'AmpConv 2', act + ' 2', 'Average Pooling' if mean else 'Class Token']
        assert all(v.is_contiguous() for v in sites.values())
        assert torch.equal(sites['AmpConv 1'], model.conv1_embedding) and torch.equal(sites['AmpConv 2'], model.conv2_embedding)
        assert torch.equal(sites[list(sites)[-1]], out) and sites[act + ' 2'].shape == (N, L * D)


def test_layer_norm_with_fused_glue_takes_the_fused_entry():
    model, _, _, real = _model({'layer_norm': True, 'fused_glue': True}, True)
    assert real == (model._glue[0], model.norm1, model.norm2) and [s._site for s in model._glue] == [1, 2, 3]


@pytest.mark.parametrize('name', list(SITE_FLAGS))
def test_entry_points_reach_the_sequence_through_run_alone(name, monkeypatch):
    from ampnet_amd.module import amp_gcn, diagnostics
    model, data, log, _ = _model(SITE_FLAGS[name], True)
    walk = model._run
    calls, pooled = [], torch.randn(N, D, generator=torch.Generator().manual_seed(2))

    def run(*args):
        calls.append(args)
        return pooled

    model._run = run
    idx = torch.zeros(N, L, dtype=torch.int32)
    assert model._pooled(data, idx) is pooled and calls.pop() == (data, idx)
    logits = model(data, idx)
    assert calls.pop() == (data, idx)
    assert torch.equal(logits, F.log_softmax(model.final_linear_out(pooled), dim=1))
    monkeypatch.setattr(amp_gcn, 'saint_nll_loss', lambda p, w, b, y, *rest: (p, w, b, y))
    got = model.nll_loss(data, feature_indices=idx)
    assert calls.pop() == (data, idx)
    assert got[0] is pooled and got[1] is model.final_linear_out.weight and got[2] is model.final_linear_out.bias
    assert torch.equal(got[3], data.y)
    assert log == [] and calls == []                                  # no layer, site or token builder was touched
    # activation_stats: the real walk, in eval mode, with the sixth site behind it and every flag restored
    model._run = lambda *args: calls.append(args) or walk(*args)
    monkeypatch.setattr(diagnostics, 'tensor_stats', lambda sites, bins, median: sites)
    model.train()
    model.conv2.eval()                                                # a flag of its own, to be restored as it was
    sites = model.activation_stats(data, feature_indices=idx)
    assert len(calls) == 1 and calls[0][0] is data and calls[0][1] is idx and calls[0][2] is sites
    act = 'LayerNorm+ReLU' if name == 'layer_norm' else 'ReLU'
    assert list(sites) == ['AmpConv 1', act + ' 1', 'AmpConv 2', act + ' 2', 'Average Pooling', 'Linear Out']
    assert [e for e in log if not e.endswith('.activate')] == WALK
    assert torch.equal(sites['Linear Out'], F.linear(sites['Average Pooling'], model.final_linear_out.weight,
                                                      model.final_linear_out.bias))
    assert model.training and model.conv1.training and not model.conv2.training
    assert all(s.training for s in model._glue)


@pytest.mark.parametrize('mean', [True, False], ids=['mean', 'token0'])
def test_unfused_walk_is_the_reference_chain_bit_for_bit(mean):
    model, data, log, _ = _model({}, mean, dropout_rate=0.5, dropout_adj_rate=0.0)
    model.train()
    torch.manual_seed(11)
    got = model._run(data)
    torch.manual_seed(11)
    want = model.drop3(F.relu(model.drop2(F.relu(model.drop1(data.x))))).reshape(N, L, D)
    want = want.mean(dim=1) if mean else want[:, 0]
    assert log == WALK and torch.equal(got, want) and float(got.abs().sum()) > 0
    model.eval()
    quiet = model._run(data)
    assert not torch.equal(quiet, got)                                 # the masks were really drawn
    assert torch.equal(quiet, F.relu(data.x).reshape(N, L, D).mean(dim=1) if mean else F.relu(data.x)[:, :D])
