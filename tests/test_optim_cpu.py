"""The fused optimizer step without a GPU: the numpy model of tests/optim_reference.py against torch.optim.Adam / AdamW and
clip_grad_norm_ in float64, the host-only behaviour of FusedAdam (laziness, LR schedulers, refusals, state dicts to and
from torch.optim.Adam), the binding's signatures, and GradientAllReducer.allreduce(unpack=False)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.distributed as dist

import optim_reference as ref

# both sides are float64 and differ only in the order of operations: a few ulp (1e-16 relative) per step
TOL = dict(rtol=1e-10, atol=1e-12)
LR, WD, STEPS = 0.1, 1e-4, 5


def _torch_run(cls, params, grads_per_step, max_norm, **kw):
    ps = [torch.nn.Parameter(torch.from_numpy(np.asarray(p, np.float64).copy())) for p in params]
    opt = cls(ps, lr=LR, foreach=False, **kw)
    norms = []
    for grads in grads_per_step:
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(np.asarray(g, np.float64).copy())
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)))
        opt.step()
    return ps, opt, norms


@pytest.mark.parametrize('decoupled', [False, True], ids=['adam', 'adamw'])
@pytest.mark.parametrize('clip', [None, 'below', 'above'])
def test_numpy_model_matches_torch_in_float64(decoupled, clip):
    params = ref.make_params(ref.SIZES, 1)
    grads = [ref.make_grads(ref.SIZES, 10 + k) for k in range(STEPS)]
    true_norm = ref.grad_norm(grads[0])
    max_norm = None if clip is None else true_norm * (0.5 if clip == 'below' else 1e3)     # clips / coefficient 1
    if clip == 'above':
        assert all(ref.grad_norm(g) < max_norm for g in grads)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ps, opt, norms = _torch_run(cls, params, grads, max_norm, weight_decay=WD)
    mine = ref.Adam(params, lr=LR, weight_decay=WD, decoupled=decoupled, max_grad_norm=max_norm)
    for k, g in enumerate(grads):
        mine.step(g)
        if max_norm is not None:
            np.testing.assert_allclose(mine.norm, norms[k], rtol=1e-12)
    for i, p in enumerate(ps):
        np.testing.assert_allclose(mine.p[i], p.detach().numpy(), **TOL)
        np.testing.assert_allclose(mine.m[i], opt.state[p]['exp_avg'].numpy(), **TOL)
        np.testing.assert_allclose(mine.v[i], opt.state[p]['exp_avg_sq'].numpy(), **TOL)
    assert ref.clip_coefficient(3.0, None) == 1.0 and ref.clip_coefficient(0.5, 1.0) == 1.0
    assert ref.clip_coefficient(4.0, 1.0) == 1.0 / (4.0 + 1e-6)


def test_numpy_model_skips_missing_gradients_and_scales():
    params = ref.make_params([(5,), (4,)], 3)
    g = ref.make_grads([(5,), (4,)], 4)
    a = ref.Adam(params, lr=LR).step([g[0], None]).step(g)
    assert a.t == [2, 1] and np.array_equal(ref.Adam(params, lr=LR).step([g[0], None]).p[1], params[1].astype(np.float64))
    b = ref.Adam(params, lr=LR).step(g, grad_scale=0.25)
    c = ref.Adam(params, lr=LR).step([0.25 * x.astype(np.float64) for x in g])
    np.testing.assert_allclose(b.p[0], c.p[0], **TOL)
    np.testing.assert_allclose(b.norm, c.norm, rtol=1e-12)


def test_binding_declares_the_optimizer_entry_points():
    from ampnet_amd import _lib, optim
    for name in ('ampconv_adam_workspace_bytes', 'ampconv_adam_grad_norm', 'ampconv_adam_step'):
        assert name in _lib.SIGNATURES, name
    assert _lib.EXPECTED_ABI == 111
    assert ctypes.sizeof(_lib.AdamTensor) == 48 and _lib.AdamTensor.numel.offset == 32          # 4 pointers, int64, 2 floats
    assert optim.CHUNK == _lib.ADAM_CHUNK == 1024 and optim.MAX_TENSORS == _lib.ADAM_MAX_TENSORS == 24


def test_header_constants_match_the_binding():
    import os
    import re
    from conftest import ROOT
    from ampnet_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'ampconv.h')).read()
    assert int(re.search(r'#define\s+AMPCONV_ADAM_MAX_TENSORS\s+(\d+)', src).group(1)) == _lib.ADAM_MAX_TENSORS
    assert int(re.search(r'#define\s+AMPCONV_ADAM_CHUNK\s+(\d+)', src).group(1)) == _lib.ADAM_CHUNK


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.ReLU(), torch.nn.Linear(5, 3))


def test_construction_is_lazy_and_schedulers_drive_it():
    from ampnet_amd import FusedAdam
    model = _model()
    opt = FusedAdam(model.parameters(), lr=0.1, weight_decay=1e-4)
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.state) == 0 and opt.grad_norm is None
    assert isinstance(opt.param_groups[0]['lr'], float)
    twin = torch.optim.Adam(_model().parameters(), lr=0.1, weight_decay=1e-4)
    a = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=4, T_mult=2)
    b = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(twin, T_0=4, T_mult=2)
    seen = []
    for _ in range(14):                                     # no gradients anywhere: step() has nothing to do, on any device
        opt.step()
        twin.step()
        a.step()
        b.step()
        assert opt.param_groups[0]['lr'] == twin.param_groups[0]['lr']
        seen.append(opt.param_groups[0]['lr'])
    assert len(set(seen)) > 4 and seen[3] == 0.1 and seen[11] == 0.1        # the restarts after 4 and 4 + 8 steps
    assert len(opt.state) == 0


def test_cpu_parameters_are_refused_at_step():
    from ampnet_amd import FusedAdam
    model = _model()
    opt = FusedAdam(model.parameters(), lr=0.1, max_grad_norm=1.0)
    model(torch.randn(4, 6)).sum().backward()
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(ValueError, match='GPU'):
        opt.step()
    with pytest.raises(ValueError, match='GPU'):
        opt.step(grads=[p.grad for p in model.parameters()], grad_scale=0.5, set_to_none=True)
    assert len(opt.state) == 0 and all(p.grad is not None for p in model.parameters())         # a refused call changes nothing
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    with pytest.raises(ValueError, match='4 parameters'):
        opt.step(grads=[None])


def test_refused_constructor_arguments():
    from ampnet_amd import FusedAdam
    ps = list(_model().parameters())
    for kw in ({'amsgrad': True}, {'maximize': True}, {'capturable': True}):
        with pytest.raises(ValueError, match='amsgrad, maximize or capturable'):
            FusedAdam(ps, **kw)
    FusedAdam(ps, amsgrad=False, maximize=False, capturable=False)               # torch.optim.Adam's spelled-out defaults
    with pytest.raises(TypeError):
        FusedAdam(ps, nesterov=True)
    for kw, what in (({'lr': -1.0}, 'lr'), ({'eps': 0.0}, 'eps'), ({'betas': (0.9, 1.0)}, 'betas'), ({'betas': (-0.1, 0.9)}, 'betas'),
                     ({'weight_decay': -1e-4}, 'weight_decay'), ({'max_grad_norm': 0.0}, 'max_grad_norm'),
                     ({'lr': torch.tensor(0.1)}, 'lr')):
        with pytest.raises(ValueError, match=what):
            FusedAdam(ps, **kw)
    opt = FusedAdam(ps)
    opt.param_groups[0]['amsgrad'] = True                   # e.g. from a loaded checkpoint
    ps[0].grad = torch.zeros_like(ps[0])
    with pytest.raises(ValueError, match='amsgrad'):
        opt.step()


def test_state_dicts_go_to_and_come_from_torch_adam():
    from ampnet_amd import FusedAdam
    model = _model()
    stock = torch.optim.Adam(model.parameters(), lr=0.1, weight_decay=1e-4)
    for _ in range(3):
        stock.zero_grad()
        model(torch.randn(4, 6)).pow(2).sum().backward()
        stock.step()
    sd = stock.state_dict()
    assert all(isinstance(s['step'], torch.Tensor) for s in sd['state'].values())
    opt = FusedAdam(model.parameters(), lr=0.5, decoupled=True)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert g['lr'] == 0.1 and g['weight_decay'] == 1e-4 and g['decoupled_weight_decay'] is False       # the checkpoint's groups
    for p in model.parameters():
        st = opt.state[p]
        assert sorted(st) == ['exp_avg', 'exp_avg_sq', 'step'] and st['step'] == 3 and type(st['step']) is int
        assert torch.equal(st['exp_avg'], stock.state[p]['exp_avg']) and st['exp_avg'].dtype == torch.float32
        assert torch.equal(st['exp_avg_sq'], stock.state[p]['exp_avg_sq'])
    # ... and the way back: torch.optim.Adam continues from FusedAdam's state dict
    back = torch.optim.Adam(model.parameters(), lr=0.7)
    back.load_state_dict(opt.state_dict())
    assert back.param_groups[0]['lr'] == 0.1 and back.param_groups[0]['decoupled_weight_decay'] is False
    model(torch.randn(4, 6)).pow(2).sum().backward()
    back.step()
    assert all(float(back.state[p]['step']) == 4.0 for p in model.parameters())
    # a decoupled FusedAdam arrives in torch.optim.Adam as AdamW
    adamw = torch.optim.Adam(model.parameters())
    adamw.load_state_dict(FusedAdam(model.parameters(), decoupled=True, weight_decay=1e-2).state_dict())
    assert adamw.param_groups[0]['decoupled_weight_decay'] is True and adamw.param_groups[0]['weight_decay'] == 1e-2


def test_allreduce_without_unpack_leaves_the_flat_buffer(tmp_path):
    from ampnet_amd.distributed import GradientAllReducer
    dist.init_process_group('gloo', store=dist.FileStore(str(tmp_path / 'store'), 1), rank=0, world_size=1)
    try:
        model = _model()
        params = list(model.parameters())
        model(torch.randn(4, 6)).pow(2).sum().backward()
        grads = [p.grad for p in params]
        kept = [g.clone() for g in grads]
        reducer = GradientAllReducer(params)
        flat = reducer.allreduce(unpack=False)
        assert torch.equal(flat, torch.cat([g.reshape(-1) for g in kept]))
        assert all(p.grad is g and torch.equal(g, k) for p, g, k in zip(params, grads, kept))       # the same objects, untouched
        views = reducer.views
        assert len(views) == len(params)
        for v, p, k in zip(views, params, kept):
            assert v.shape == p.shape and torch.equal(v, k)
            assert v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        # a missing gradient counts as zero and stays missing
        params[1].grad = None
        flat = reducer.allreduce(unpack=False)
        assert params[1].grad is None and not reducer.views[1].any() and torch.equal(reducer.views[0], kept[0])
        # the default call: as before -- the mean written back into every p.grad, a missing one created
        out = reducer.allreduce()
        assert out is flat and params[1].grad is not None and not params[1].grad.any()
        assert params[0].grad is grads[0] and torch.equal(params[0].grad, kept[0])
    finally:
        dist.destroy_process_group()
