"""AMPGCN's diagnostics (gradient_stats, activation_stats and the three reference-named figure methods) on the GPU, on the
smallest down-sampling whole-model fixture (tests/golden/model_cora.npz: 48 nodes, L = 20, D = 128) in four
configurations, each with dropout_rate = 0.1.  The numbers are held to the numpy model of tests/stats_reference.py run on
host copies of the very tensors: counts, extrema and histograms exactly, absmean / std at rtol 1e-6 (fp64 sums on both
sides, see tests/test_gpu_stats.py).

"No stream advanced": the training step after an activation_stats call is compared with the same step of a twin that never
made the call -- the sampled feature indices, every seeded site's call counter and last seed, the loss and every parameter
gradient bit for bit, with ONE exception: feature_embedding_table.weight.grad is summed with float atomics
(csrc/featurizer.hip: "the last bits may differ run to run"), so two identical runs already differ there; it is held to
1e-6 of its largest entry, which a redrawn mask or index set (what the check is about) misses by orders of magnitude."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stats_reference as ref
from conftest import load_golden, model_files

pytestmark = pytest.mark.gpu

CONFIGS = {'plain': {}, 'fused_glue': {'fused_glue': True}, 'layer_norm': {'layer_norm': True},
           'fused_head': {'fused_head': True}}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _cfg_value(v):
    if v in ('True', 'False'):
        return v == 'True'
    if v == 'None':
        return None
    try:
        return int(v)
    except ValueError:
        return float(v)


def _build(dev, flags, fixture='model_cora.npz'):
    from ampnet_amd import AMPGCN
    g = load_golden([f for f in model_files() if f.endswith(fixture)][0])
    cfg = {k: _cfg_value(v) for k, v in zip(g['cfg_keys'].tolist(), g['cfg_vals'].tolist())}
    cfg.update(dropout_rate=0.1, dropout_adj_rate=0.0, **flags)
    state = {k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')}
    x, ei = torch.from_numpy(g['x']).to(dev), torch.from_numpy(g['edge_index']).to(dev)
    y = torch.randint(0, cfg['output_dim'], (x.shape[0],), generator=torch.Generator().manual_seed(3)).to(dev)
    torch.manual_seed(0)
    model = AMPGCN(device=dev, seed=5, **cfg).to(dev)
    model.load_state_dict(state, strict=False)                     # (layer_norm: norm1 / norm2 keep their ones, zeros)
    return model, types.SimpleNamespace(x=x, edge_index=ei, y=y)


def _train_step(model, data):
    """One forward + backward in training mode; returns the loss."""
    model.train()
    model.zero_grad(set_to_none=True)
    if model.fused_head:
        loss = model.nll_loss(data)
    else:
        loss = F.nll_loss(model(data), data.y, reduction='sum')
    loss.backward()
    return loss.detach()


def _np(t):
    return t.detach().float().cpu().numpy()


def _exact(got, want, what, keys=('numel', 'finite', 'nan', 'inf', 'zeros', 'negative', 'min', 'max', 'absmax', 'below', 'above')):
    for k in keys:
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got['hist'], want['hist']), (what, 'hist')
    assert np.float32(got['median']).tobytes() == np.float32(want['median']).tobytes(), (what, got['median'], want['median'])
    for k in ('absmean', 'std') + (('mean',) if abs(want['mean']) > 1e-3 * want['absmean'] else ()):
        err = abs(got[k] - want[k]) / abs(want[k]) if want[k] else abs(got[k] - want[k])
        print(f'[tol] {what} {k}: rel err {err:.2e} (bar 1e-6)')
        assert err <= 1e-6, (what, k, got[k], want[k])


def _sites(flags, pooling='Average Pooling'):
    act = 'LayerNorm+ReLU' if flags.get('layer_norm') else 'ReLU'
    return ['AmpConv 1', act + ' 1', 'AmpConv 2', act + ' 2', pooling, 'Linear Out']


@pytest.mark.parametrize('name', list(CONFIGS))
def test_gradient_stats(dev, name):
    model, data = _build(dev, CONFIGS[name])
    _train_step(model, data)
    want_names = [n for n, p in model.named_parameters() if 'weight' in n and p.grad is not None]
    assert len(want_names) == (8 if name == 'layer_norm' else 6)        # table, 2 x (in_proj, out_proj), head (, 2 norms)
    got = model.gradient_stats().read()
    assert list(got) == want_names and 'final_linear_out.bias' not in got
    params = dict(model.named_parameters())
    for n in want_names:
        _exact(got[n], ref.stats(_np(params[n].grad), bins=30, median=True), f'{name} {n}.grad')
        assert got[n]['hist'].shape == (30,)
    # a NaN in one gradient is counted, and only counted
    victim = want_names[-1]
    g = params[victim].grad
    g.view(-1)[min(5, g.numel() - 1)] = float('nan')
    after = model.gradient_stats().read()
    want = ref.stats(_np(g), bins=30, median=True)
    assert after[victim]['nan'] == 1 and after[victim]['finite'] == g.numel() - 1
    _exact(after[victim], want, f'{name} {victim}.grad with a NaN')
    assert all(np.isfinite(after[victim][k]) for k in ('min', 'max', 'absmax', 'mean', 'absmean', 'std', 'median'))
    assert all(after[n]['nan'] == 0 for n in want_names[:-1])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_activation_stats(dev, name):
    model, data = _build(dev, CONFIGS[name])
    _train_step(model, data)
    idx = model.sampled_node_feat_indices.clone()
    model.train()
    got = model.activation_stats(data).read()
    assert model.training                                              # the flag is restored (the reference leaves eval)
    assert list(got) == _sites(CONFIGS[name])
    assert torch.equal(model.sampled_node_feat_indices, idx)           # the batch that was just trained on
    for k, emb in (('AmpConv 1', model.conv1_embedding), ('AmpConv 2', model.conv2_embedding)):
        assert not emb.requires_grad and emb.shape == (48, 20 * 128)
        _exact(got[k], ref.stats(_np(emb), bins=50, median=True), f'{name} {k}')
    for k in got:
        assert got[k]['nan'] == 0 and got[k]['inf'] == 0 and got[k]['hist'].shape == (50,)
        if 'ReLU' in k:
            assert got[k]['negative'] == 0 and got[k]['min'] == 0.0 and got[k]['zeros'] > 0, (k, got[k])
    assert got['AmpConv 1']['negative'] > 0
    # the logits: recomputed with torch from the model's own pooled tensor of the same eval-mode pass
    model.eval()
    with torch.no_grad():
        pooled = model._pooled(data, feature_indices=idx)
        logits = F.linear(pooled, model.final_linear_out.weight, model.final_linear_out.bias)
    _exact(got['Average Pooling'], ref.stats(_np(pooled), bins=50, median=True), f'{name} pooled')
    _exact(got['Linear Out'], ref.stats(_np(logits), bins=50, median=True), f'{name} logits')
    model.eval()
    model.activation_stats(data, bins=8)
    assert not model.training                                          # ... whatever it was


def test_class_token_site_and_explicit_indices(dev):
    """The token-0 pooling is named "Class Token"; a full-width model has no indices to sample."""
    model, data = _build(dev, {}, 'model_xor_tok0.npz')
    got = model.activation_stats(data, bins=10).read()
    assert list(got) == _sites({}, 'Class Token') and model.sampled_node_feat_indices is None
    assert got['Class Token']['numel'] == 64 * 3 and got['Linear Out']['numel'] == 64 * 2
    # a down-sampling model before any forward pass draws indices without touching the sampler's call counter
    model, data = _build(dev, {})
    assert model.sampled_node_feat_indices is None and model._tokens[0]._calls == 0
    a = model.activation_stats(data).read()
    drawn = model.sampled_node_feat_indices.clone()
    b = model.activation_stats(data, feature_indices=drawn).read()
    assert model._tokens[0]._calls == 0 and drawn.shape == (48, 20)
    assert a['Linear Out']['mean'] == b['Linear Out']['mean'] and np.array_equal(a['AmpConv 2']['hist'], b['AmpConv 2']['hist'])


@pytest.mark.parametrize('name', list(CONFIGS))
def test_activation_stats_advances_no_stream(dev, name):
    runs = []
    for call in (True, False):
        model, data = _build(dev, CONFIGS[name])
        torch.manual_seed(7)
        _train_step(model, data)
        if call:
            model.activation_stats(data)
        loss = _train_step(model, data)
        sites = list(model._glue) + ([model.norm1, model.norm2] if model.layer_norm else [])
        runs.append((loss.cpu(), {n: p.grad.detach().cpu() for n, p in model.named_parameters()},
                     model.sampled_node_feat_indices.cpu(), model._tokens[0]._calls,
                     [(s._calls, s.last_seed) for s in sites]))
    (loss_a, grads_a, idx_a, calls_a, seeds_a), (loss_b, grads_b, idx_b, calls_b, seeds_b) = runs
    assert calls_a == calls_b == 2 and seeds_a == seeds_b and torch.equal(idx_a, idx_b)
    assert torch.equal(loss_a, loss_b), (float(loss_a), float(loss_b))
    for n in grads_a:
        if n == 'feature_embedding_table.weight':                      # float atomics: see the module docstring
            top = float(grads_b[n].abs().max())
            assert float((grads_a[n] - grads_b[n]).abs().max()) <= 1e-6 * top, n
        else:
            assert torch.equal(grads_a[n], grads_b[n]), n


@pytest.mark.parametrize('name,fixture', [(n, 'model_cora.npz') for n in CONFIGS]
                         + [('plain', 'model_xor_tok0.npz'), ('fused_glue', 'model_xor_tok0.npz')])
def test_sites_are_the_forward_pass(dev, name, fixture):
    """What the diagnostics record is the forward pass itself: in eval mode _run with a `sites` dict returns _pooled's
    tensor bit for bit, a site's activate() is the site (dropout is off) without its pooling, and nothing is advanced.
    The token mean against a float64 mean of activate(): (L - 1) additions of the ascending fp32 sum, each rounding a
    partial sum <= k max, then one reciprocal and one product -- ((L + 1) / 2 + 2) 2^-24 max_l |a[n, l, c]| per element."""
    model, data = _build(dev, CONFIGS[name], fixture)
    D, mean = model.emb_dim, model.average_pooling_flag
    idx = model._tokens[0].sample(data.x, seed=17)[0] if model.downsampling_vectors else None    # a seed given: no counter
    seeded = list(model._glue) + ([model.norm1, model.norm2] if model.layer_norm else [])
    assert len(seeded) == {'fused_glue': 3, 'layer_norm': 2}.get(name, 0)
    counters = lambda: ([(s._calls, s.last_seed) for s in seeded], model._tokens[0]._calls)
    before = counters()
    model.eval()
    with torch.no_grad():
        pooled = model._pooled(data, idx)
        sites = {}
        out = model._run(data, idx, sites)
        assert torch.equal(out, pooled) and pooled.shape == (data.x.shape[0], D) and float(pooled.abs().sum()) > 0
        assert list(sites) == _sites(CONFIGS[name], 'Average Pooling' if mean else 'Class Token')[:-1]
        h1, h2 = sites['AmpConv 1'], sites['AmpConv 2']
        assert torch.equal(h1, model.conv1_embedding) and torch.equal(h2, model.conv2_embedding)
        _, between, readout = model._sites
        a1, a2 = between.activate(h1), readout.activate(h2)
        assert torch.equal(between(h1), a1) and a1.shape == h1.shape and a2.shape == h2.shape
        act = 'LayerNorm+ReLU' if model.layer_norm else 'ReLU'
        assert torch.equal(sites[act + ' 1'], a1) and torch.equal(sites[act + ' 2'], a2)
        got = readout(h2)
        assert torch.equal(got, pooled)
        if mean:
            L = a2.shape[1] // D
            a = a2.view(-1, L, D).double()
            bound = ((L + 1) / 2 + 2) * 2.0 ** -24 * a.abs().amax(dim=1)
            err = (got.double() - a.mean(dim=1)).abs()
            live = bound > 0
            print(f'[tol] {name} token mean, L = {L}: largest share of the bound '
                  f'{float((err[live] / bound[live]).max()):.3f}, dead channels {int((~live).sum())}')
            assert bool((err <= bound).all()), (name, float((err - bound).max()))
        else:
            assert torch.equal(got, a2[:, :D])
    assert counters() == before


def test_reference_named_figures(dev, tmp_path):
    """The harness's calls (experiments/cora_benchmark_graphsaint.py:111-114), argument for argument."""
    pytest.importorskip('matplotlib')
    model, data = _build(dev, {'fused_glue': True, 'fused_head': True})
    _train_step(model, data)
    grads_path, activ_path, epoch, idx = str(tmp_path / 'grads'), str(tmp_path / 'activ'), 2, 4
    os.makedirs(grads_path)
    os.makedirs(activ_path)
    flow = model.plot_grad_flow(grads_path, epoch, idx)
    dist = model.visualize_gradients(grads_path, epoch, idx)
    act = model.visualize_activations(activ_path, data, epoch, idx)
    for path in (os.path.join(grads_path, 'gradient_flow_plots', 'gradient_flow_ep2_itr4.png'),
                 os.path.join(grads_path, 'gradient_distrib_plots', 'gradient_distrib_epoch2_itr4.png'),
                 os.path.join(activ_path, 'act_distrib_ep2_iter4.png')):
        assert os.path.getsize(path) > 1000, path
    names = [n for n, p in model.named_parameters() if 'weight' in n and p.grad is not None]
    assert list(flow) == list(dist) == names and list(act) == _sites({})
    assert all(dist[n]['hist'].shape == (30,) and flow[n]['absmax'] == dist[n]['absmax'] for n in names)
    assert all(s['hist'].shape == (50,) for s in act.values()) and model.training
