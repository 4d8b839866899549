"""The fused optimizer step (csrc/optim.hip behind ampnet_amd/optim.py) on the GPU against the numpy fp64 model of
tests/optim_reference.py, against torch.optim.Adam on the GPU, across state-dict hand-overs and inside the whole model.

Tensors: numels 1, 3, 7 (tails only), 1024 = CHUNK, 1025 = CHUNK + 1, 4100 = 4 CHUNK + 4 (several chunks, a tail of one
piece), a [7, 100] matrix, and a contiguous 37-element slice one float into a larger buffer: 4-byte aligned only, the
element-wise path (its gradient is such a slice as well, for the norm's element-wise path).
Gradients: fresh per step, magnitudes log-uniform in [1e-6, 1e2], random sign, ~10 % exact zeros; parameters N(0, 1).
Tolerances: p at the project's flat fp32 bar (atol 1e-5, rtol 1e-4): an update is at most ~3.2 lr and carries a few fp32
roundings, 5 steps at lr = 0.1 accumulate under 2e-6.  exp_avg, exp_avg_sq relative to the tensor,
max|got - want| <= 1e-5 max|want|: 5-term convex combinations, at most ~15 roundings.  grad_norm rtol 1e-5: a butterfly sum
of squares and a handful of ordered slot additions."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import optim_reference as ref
from conftest import assert_close_scaled, load_golden, model_files

pytestmark = pytest.mark.gpu

SHAPES = ref.SIZES + [(37,)]               # the last one: the unaligned slice
LR, WD, STEPS = 0.1, 1e-4, 5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _data(steps=STEPS):
    """(parameters, per-step gradients) as float32 numpy arrays: drawn once, shared, never modified."""
    return ref.make_params(SHAPES, 1), [ref.make_grads(SHAPES, 10 + k) for k in range(steps)]


@functools.lru_cache(maxsize=None)
def _reference(decoupled=False, weight_decay=WD, grad_scale=1.0, max_grad_norm=None):
    """The fp64 model after every step: [(p, m, v, norm)], computed once per configuration."""
    params, grads = _data()
    opt = ref.Adam(params, lr=LR, weight_decay=weight_decay, decoupled=decoupled, max_grad_norm=max_grad_norm)
    out = []
    for g in grads:
        opt.step(g, grad_scale)
        out.append(([a.copy() for a in opt.p], [a.copy() for a in opt.m], [a.copy() for a in opt.v], opt.norm))
    return out


def _unaligned(a, dev, lead):
    """A contiguous device copy of `a` that starts `lead` floats into a larger buffer: 4-byte aligned only."""
    base = torch.zeros(a.size + 64, dtype=torch.float32, device=dev)
    view = base[lead:lead + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


def _params(dev, arrays=None):
    arrays = _data()[0] if arrays is None else arrays
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in arrays[:-1]]
    ps.append(torch.nn.Parameter(_unaligned(arrays[-1], dev, 1)))
    assert ps[-1].data_ptr() % 16 == 4 and ps[3].data_ptr() % 16 == 0
    return ps


def _grads(dev, arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays[:-1]] + [_unaligned(arrays[-1], dev, 3)]


def _rel(got, want, name):
    got, want = np.asarray(_np(got), np.float64), np.asarray(want, np.float64)
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f'[tol] {name}: max err {err:.3e} = {err / top if top else 0.0:.3e} of max |want| {top:.3e} (bar 1e-5)')
    assert err <= 1e-5 * top, f'{name}: max err {err:.3e} over 1e-5 * {top:.3e}'


def _check(opt, ps, want, what):
    p, m, v, _ = want
    for i, t in enumerate(ps):
        assert_close_scaled(_np(t), p[i], f'p[{i}] {what}', scaled=False)
        _rel(opt.state[t]['exp_avg'], m[i], f'exp_avg[{i}] {what}')
        _rel(opt.state[t]['exp_avg_sq'], v[i], f'exp_avg_sq[{i}] {what}')


def _check_norm(opt, want, what):
    got = float(opt.grad_norm)
    print(f'[tol] grad_norm {what}: {got:.9e} vs {want:.9e}, rel err {abs(got - want) / want:.3e} (bar 1e-5)')
    assert opt.grad_norm.dtype == torch.float32 and opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda
    assert abs(got - want) <= 1e-5 * want


def _run(dev, steps=STEPS, grads_kw=False, nan_grads=False, step_kw=None, **kw):
    """FusedAdam over the tensor set for `steps` steps; yields (step, opt, params) after every step."""
    from ampnet_amd import FusedAdam
    ps = _params(dev)
    opt = FusedAdam(ps, lr=LR, **kw)
    for k in range(steps):
        gs = _grads(dev, _data()[1][k])
        if grads_kw:
            for p in ps:
                p.grad = torch.full_like(p, float('nan')) if nan_grads else None
            opt.step(grads=gs, **(step_kw or {}))
        else:
            for p, g in zip(ps, gs):
                p.grad = g
            opt.step(**(step_kw or {}))
        yield k, opt, ps


def test_adam_matches_the_reference_after_every_step(dev):
    want = _reference()
    for k, opt, ps in _run(dev, weight_decay=WD):
        _check(opt, ps, want[k], f'adam step {k + 1}')
        assert all(opt.state[p]['step'] == k + 1 and type(opt.state[p]['step']) is int for p in ps)
        assert opt.grad_norm is None


def test_adam_matches_torch_adam_on_the_gpu(dev):
    ps = _params(dev)
    stock = torch.optim.Adam(ps, lr=LR, weight_decay=WD, foreach=False)
    mine = _run(dev, weight_decay=WD)
    for k in range(STEPS):
        for p, g in zip(ps, _grads(dev, _data()[1][k])):
            p.grad = g
        stock.step()
        _, opt, qs = next(mine)
        want = ([_np(p) for p in ps], [_np(stock.state[p]['exp_avg']) for p in ps],
                [_np(stock.state[p]['exp_avg_sq']) for p in ps], None)
        _check(opt, qs, want, f'torch.optim.Adam step {k + 1}')


def test_decoupled_weight_decay_matches_the_reference(dev):
    want = _reference(decoupled=True, weight_decay=1e-2)
    for k, opt, ps in _run(dev, weight_decay=1e-2, decoupled=True):
        _check(opt, ps, want[k], f'adamw step {k + 1}')


def test_grads_list_and_grad_scale(dev):
    """grads= is read instead of p.grad (NaN-filled here), grad_scale rides on the pass: stepping on 0.25 g."""
    params, grads = _data()
    quarter = ref.Adam(params, lr=LR, weight_decay=WD)
    for k, opt, ps in _run(dev, grads_kw=True, nan_grads=True, step_kw={'grad_scale': 0.25}, weight_decay=WD,
                           track_grad_norm=True):
        quarter.step([0.25 * g.astype(np.float64) for g in grads[k]])
        _check(opt, ps, (quarter.p, quarter.m, quarter.v, None), f'grad_scale 0.25 step {k + 1}')
        _check_norm(opt, quarter.norm, f'grad_scale 0.25 step {k + 1}')
        assert all(torch.isnan(p.grad).all() for p in ps)                      # still there, never read
    # None entries of the list are skipped like missing gradients
    for k, opt, ps in _run(dev, steps=1, grads_kw=True, weight_decay=WD):
        pass
    gs = _grads(dev, grads[1])
    gs[2] = None
    before = ps[2].detach().clone()
    opt.step(grads=gs)
    assert torch.equal(ps[2], before) and opt.state[ps[2]]['step'] == 1 and opt.state[ps[0]]['step'] == 2


def test_clipping_and_the_tracked_norm(dev):
    _, grads = _data()
    norms = [ref.grad_norm(g) for g in grads]
    for what, max_norm in (('clips', 0.5 * min(norms)), ('coefficient 1', 2.0 * max(norms))):
        want = _reference(max_grad_norm=max_norm)
        for k, opt, ps in _run(dev, weight_decay=WD, max_grad_norm=max_norm):
            _check(opt, ps, want[k], f'{what} step {k + 1}')
            _check_norm(opt, want[k][3], f'{what} step {k + 1}')
    plain = [[p.detach().clone() for p in ps] for _, _, ps in _run(dev, steps=2, weight_decay=WD)]
    for k, opt, ps in _run(dev, steps=2, weight_decay=WD, track_grad_norm=True):
        assert all(torch.equal(p, q) for p, q in zip(ps, plain[k]))           # tracking alone changes no bit
        _check_norm(opt, norms[k], f'tracked step {k + 1}')


def test_parameter_without_gradient_is_skipped(dev):
    from ampnet_amd import FusedAdam
    params, grads = _data()
    ps = _params(dev)
    opt = FusedAdam(ps, lr=LR, weight_decay=WD, max_grad_norm=1e3)
    model = ref.Adam(params, lr=LR, weight_decay=WD, max_grad_norm=1e3)
    before = ps[4].detach().clone()
    for k in range(3):
        gs, want = _grads(dev, grads[k]), list(grads[k])
        if k < 2:
            gs[4], want[4] = None, None
        for p, g in zip(ps, gs):
            p.grad = g
        opt.step()
        model.step(want)
        _check_norm(opt, model.norm, f'missing gradient step {k + 1}')         # the norm runs over what has a gradient
        if k < 2:
            assert torch.equal(ps[4], before) and ps[4] not in opt.state
    assert opt.state[ps[4]]['step'] == 1 and opt.state[ps[0]]['step'] == 3 and model.t[4] == 1
    for i, p in enumerate(ps):
        assert_close_scaled(_np(p), model.p[i], f'p[{i}] after a late first gradient', scaled=False)
        _rel(opt.state[p]['exp_avg'], model.m[i], f'exp_avg[{i}] after a late first gradient')


def test_more_tensors_than_one_launch_holds(dev):
    from ampnet_amd import FusedAdam, optim
    n = 2 * optim.MAX_TENSORS + 1
    shapes = [(5,)] * n
    shapes.insert(30, (0,))                                                    # a zero-numel tensor inside the second launch
    params = ref.make_params(shapes, 5)
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in params]
    opt = FusedAdam(ps, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    model = ref.Adam(params, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    for k in range(2):
        grads = ref.make_grads(shapes, 50 + k)
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(dev)
        opt.step()
        model.step(grads)
        _check_norm(opt, model.norm, f'{n} tensors step {k + 1}')
    assert_close_scaled(np.concatenate([_np(p) for p in ps]), np.concatenate(model.p), f'p of {n} + 1 tensors', scaled=False)
    _rel(torch.cat([opt.state[p]['exp_avg'] for p in ps]), np.concatenate(model.m), f'exp_avg of {n} + 1 tensors')
    _rel(torch.cat([opt.state[p]['exp_avg_sq'] for p in ps]), np.concatenate(model.v), f'exp_avg_sq of {n} + 1 tensors')


def test_bitwise_reproducible(dev):
    runs = []
    for _ in range(2):
        for k, opt, ps in _run(dev, steps=3, weight_decay=WD, max_grad_norm=10.0):
            pass
        runs.append([t.clone() for p in ps for t in (p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq'])]
                    + [opt.grad_norm.clone()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_set_to_none_folds_zero_grad_into_the_step(dev):
    plain = [p.detach().clone() for p in [ps for _, _, ps in _run(dev, steps=2, weight_decay=WD)][-1]]
    for k, opt, ps in _run(dev, steps=2, step_kw={'set_to_none': True}, weight_decay=WD):
        assert all(p.grad is None for p in ps)
    assert all(torch.equal(p, q) for p, q in zip(ps, plain))


def test_no_device_synchronisation(dev):
    from ampnet_amd import FusedAdam
    _, grads = _data()
    for kw, with_list in (({}, False), ({'max_grad_norm': 1.0}, False), ({'track_grad_norm': True}, True)):
        ps = _params(dev)
        opt = FusedAdam(ps, lr=LR, weight_decay=WD, **kw)
        gs = [_grads(dev, grads[k]) for k in range(2)]
        for p, g in zip(ps, gs[0]):
            p.grad = g
        opt.step()                                                             # warm up: library load, state, allocator
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode('error')
        try:
            if with_list:
                opt.step(grads=gs[1], grad_scale=0.5, set_to_none=True)
            else:
                for p, g in zip(ps, gs[1]):
                    p.grad = g
                opt.step(set_to_none=True)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert all(opt.state[p]['step'] == 2 for p in ps) and all(torch.isfinite(p).all() for p in ps)


def test_checkpoint_hand_over_in_both_directions(dev):
    from ampnet_amd import FusedAdam
    want = _reference()
    _, grads = _data()

    def steps(opt, ps, ks):
        for k in ks:
            for p, g in zip(ps, _grads(dev, grads[k])):
                p.grad = g
            opt.step()

    # torch.optim.Adam for 3 steps, FusedAdam for 2 more
    ps = _params(dev)
    stock = torch.optim.Adam(ps, lr=LR, weight_decay=WD, foreach=False)
    steps(stock, ps, range(3))
    opt = FusedAdam(ps)
    opt.load_state_dict(stock.state_dict())
    assert all(opt.state[p]['step'] == 3 for p in ps) and opt.param_groups[0]['lr'] == LR
    steps(opt, ps, range(3, 5))
    _check(opt, ps, want[4], 'torch.optim.Adam x 3 -> FusedAdam x 2')
    # FusedAdam for 3 steps, torch.optim.Adam for 2 more
    ps = _params(dev)
    opt = FusedAdam(ps, lr=LR, weight_decay=WD)
    steps(opt, ps, range(3))
    stock = torch.optim.Adam(ps, foreach=False)
    stock.load_state_dict(opt.state_dict())
    steps(stock, ps, range(3, 5))
    _check(stock, ps, want[4], 'FusedAdam x 3 -> torch.optim.Adam x 2')
    assert all(float(stock.state[p]['step']) == 5.0 for p in ps)


def test_refused_arguments_at_the_c_boundary(dev):
    from ampnet_amd import _lib
    lib = _lib.load()
    p, g, m, v = (torch.randn(2000, device=dev) for _ in range(4))
    before = [t.clone() for t in (p, m, v)]
    norm, ws = torch.full((), 7.0, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)

    def table(*rows):
        return (_lib.AdamTensor * len(rows))(*rows)

    good = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 2000, 0.1, 1.0)
    hyper = dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, grad_scale=1.0, norm=None,
                 max_grad_norm=0.0)

    def step(t, n, **kw):
        a = {**hyper, **kw}
        return lib.ampconv_adam_step(t, n, a['lr'], a['beta1'], a['beta2'], a['eps'], a['weight_decay'], a['decoupled'],
                                     a['grad_scale'], a['norm'], a['max_grad_norm'], None)

    one = table(good)
    assert step(one, -1) == -1
    assert step(None, 1) == -1
    for hole in range(4):                                                      # a NULL p, g, m or v with numel > 0
        row = list(good)
        row[hole] = None
        assert step(table(tuple(row)), 1) == -1
        assert lib.ampconv_adam_grad_norm(table(tuple(row)), 1, 1.0, norm.data_ptr(), ws.data_ptr(), 64, None) == -1
    assert step(table(good[:4] + (-1,) + good[5:]), 1) == -1                   # negative numel
    for kw in ({'lr': -0.1}, {'eps': 0.0}, {'eps': -1e-8}, {'beta1': 1.0}, {'beta1': -0.1}, {'beta2': 1.0}, {'beta2': -0.1},
               {'weight_decay': -1e-4}, {'norm': norm.data_ptr(), 'max_grad_norm': 0.0},
               {'norm': norm.data_ptr(), 'max_grad_norm': -1.0}):
        assert step(one, 1, **kw) == -1, kw
    need = lib.ampconv_adam_workspace_bytes(one, 1)
    assert need == 2 * 4                                                        # a slot per chunk: ceil(2000 / 1024)
    assert lib.ampconv_adam_grad_norm(one, 1, 1.0, None, ws.data_ptr(), 64, None) == -1
    assert lib.ampconv_adam_grad_norm(one, -1, 1.0, norm.data_ptr(), ws.data_ptr(), 64, None) == -1
    assert lib.ampconv_adam_grad_norm(one, 1, 1.0, norm.data_ptr(), ws.data_ptr(), need - 1, None) == -3
    assert lib.ampconv_adam_grad_norm(one, 1, 1.0, norm.data_ptr(), None, 0, None) == -3
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)) and float(norm) == 7.0     # nothing was launched
    # nothing to do is no error; the norm of nothing is 0
    assert step(None, 0) == 0 and step(table(good[:4] + (0,) + good[5:]), 1) == 0
    assert step(table((None, None, None, None, 0, 0.1, 1.0)), 1) == 0
    assert lib.ampconv_adam_workspace_bytes(None, 0) == 0
    assert lib.ampconv_adam_grad_norm(None, 0, 1.0, norm.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((p, m, v), before)) and float(norm) == 0.0
    assert ctypes.sizeof(_lib.AdamTensor) == 48


@pytest.mark.parametrize('flags', [{}, {'layer_norm': True, 'fused_glue': True, 'fused_head': True}], ids=['plain', 'fused'])
def test_model_trains_like_under_torch_adam(dev, flags):
    """The smallest AMPGCN of the model tests (the XOR fixture's configuration, no dropout): twins from one state dict,
    3 training steps through nll_loss under FusedAdam and under torch.optim.Adam(foreach=False), lr 0.01 so that the
    feedback of rounding differences through the model stays inside the flat bar.
    The key third of each in_proj_bias is set to +-1 in the common state dict.  The softmax does not see a key bias, so its
    gradient is rounding noise (~1e-9) around the decay term weight_decay * p, and Adam divides by the gradient's own
    magnitude: a twin's 1-ulp difference in any parameter redraws that noise (delta ~ 1e-9 .. 1e-8) and moves the entry by
    up to lr * 0.5 * delta / (weight_decay * |p|) per step -- 1e-4 at the fixture's |p| = 5e-3, whatever the optimizer's
    own accuracy; at |p| = 1 it is 5e-7, well inside the bar."""
    from ampnet_amd import AMPGCN, FusedAdam
    path = [f for f in model_files() if f.endswith('model_xor.npz')][0]
    g = load_golden(path)
    cfg = {k: _cfg_value(v) for k, v in zip(g['cfg_keys'].tolist(), g['cfg_vals'].tolist())}
    cfg.update(dropout_rate=0.0, dropout_adj_rate=0.0, **flags)
    state = {k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')}
    D = cfg['embedding_dim']
    for conv in ('conv1', 'conv2'):
        state[f'{conv}.multi_head_attention.in_proj_bias'][D:2 * D] = torch.tensor([1.0, -1.0] * D)[:D]
    idx = g.get('sampled_node_feat_indices')
    idx = None if idx is None else torch.from_numpy(idx).to(dev)
    x, ei = torch.from_numpy(g['x']).to(dev), torch.from_numpy(g['edge_index']).to(dev)
    y = torch.randint(0, cfg['output_dim'], (x.shape[0],), generator=torch.Generator().manual_seed(3)).to(dev)
    data = types.SimpleNamespace(x=x, edge_index=ei, y=y)
    twins = []
    for make in (lambda ps: FusedAdam(ps, lr=0.01, weight_decay=1e-4),
                 lambda ps: torch.optim.Adam(ps, lr=0.01, weight_decay=1e-4, foreach=False)):
        torch.manual_seed(0)
        model = AMPGCN(device=dev, **cfg).to(dev)
        model.load_state_dict(state, strict=False)                             # (layer_norm: norm1 / norm2 keep their ones, zeros)
        model.train()
        opt = make(list(model.parameters()))
        for _ in range(3):
            opt.zero_grad()
            model.nll_loss(data, feature_indices=idx).backward()
            opt.step()
        twins.append(model)
    assert not torch.equal(twins[0].final_linear_out.bias.detach().cpu(), state['final_linear_out.bias'])     # it did train
    for (name, p), (_, q) in zip(twins[0].named_parameters(), twins[1].named_parameters()):
        assert_close_scaled(_np(p), _np(q), f'{name} after 3 steps', scaled=False)


def _cfg_value(v):
    if v in ('True', 'False'):
        return v == 'True'
    try:
        return int(v)
    except ValueError:
        return float(v)
