"""The mixed-precision optimizer step (csrc/optim.hip, ampconv_adam_mixed_*; FusedAdam over bfloat16 parameters) on the GPU.

What is held bit for bit, because the mapping of elements to lanes and the arithmetic per element are those of the fp32
step: the master / moments / gradient norm of a mixed run against an fp32 FusedAdam on the widened parameters; a bf16
gradient against the same values as an fp32 gradient; all-fp32 descriptors through the mixed entry points against the fp32
entry points on 16-byte aligned tensors; an unaligned tensor against an aligned one (the fp32 twin's tensors are all
aligned).  Against the numpy
model (tests/optim_mixed_reference.py) only where more than one launch is involved, at the bars of tests/test_gpu_optim.py.

Tensors: optim_reference.SIZES (1, 3, 7, 1024 = CHUNK, 1025, 4100, [7, 100]) plus numel 4 (one whole piece), 5 (a piece and
a tail) and 1023 (a chunk less one element), dtypes alternating fp32 / bf16; a bf16 [1:] slice of a buffer, 2-byte aligned
only (the element-wise path), whose gradient is such a slice too; an empty tensor; a parameter without a gradient."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import optim_mixed_reference as mixed
import optim_reference as ref
from conftest import assert_close_scaled

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SHAPES = ref.SIZES + [(4,), (5,), (1023,), (37,), (0,), (6,)]
DTYPES = [F32, BF16] * 5 + [BF16, F32, BF16]                  # ..., the slice (bf16), the empty one (fp32), no gradient (bf16)
SLICE, NO_GRAD = 10, 12
LR, WD, STEPS = 0.1, 1e-4, 5
CONFIGS = {'l2': (dict(weight_decay=WD), {}),
           'decoupled': (dict(weight_decay=1e-2, decoupled=True), {}),
           'clip': (dict(weight_decay=WD, max_grad_norm=3.0), dict(grad_scale=0.5)),
           'track': (dict(weight_decay=WD, track_grad_norm=True), {})}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _data():
    """(parameters, per-step gradients) as float32 numpy arrays; the gradients hold bf16 values only, so that one set of
    values can be handed over in either dtype.  Drawn once, shared, never modified."""
    params = ref.make_params(SHAPES, 1)
    grads = [[mixed.bf16_round(g) for g in ref.make_grads(SHAPES, 10 + k)] for k in range(STEPS)]
    return params, grads


def _sliced(a, dev, dtype):
    """A contiguous device copy of `a` one element into a larger buffer: aligned to the element only."""
    base = torch.zeros(a.size + 64, dtype=dtype, device=dev)
    view = base[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % (4 * view.element_size()) != 0
    return view


def _tensors(arrays, dtypes, dev, sliced=True):
    out = []
    for i, (a, dt) in enumerate(zip(arrays, dtypes)):
        out.append(_sliced(a, dev, dt) if sliced and i == SLICE else torch.from_numpy(a).to(dev, dt))
    return out


def _attach(ps, gs):
    for i, (p, g) in enumerate(zip(ps, gs)):
        p.grad = None if i == NO_GRAD else g


def _bits(a, b):
    """The same dtype, shape and bit patterns (torch.equal alone takes -0.0 for 0.0 and no NaN for itself)."""
    ints = lambda t: t.detach().contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ints(a), ints(b))


def _diff(a, b):
    """Where two float32 tensors differ, for an assertion message."""
    a, b = a.detach().reshape(-1).cpu(), b.detach().reshape(-1).cpu()
    at = (a.view(torch.int32) != b.view(torch.int32)).nonzero().reshape(-1)
    return (f'{at.numel()} of {a.numel()} elements differ, the first at {at[0].item()}: {a[at[0]].item()!r} '
            f'({a.view(torch.int32)[at[0]].item():#x}) vs {b[at[0]].item()!r} ({b.view(torch.int32)[at[0]].item():#x})') \
        if at.numel() else 'no element differs'


@pytest.mark.parametrize('grad_dtype', [BF16, F32], ids=['bf16-grads', 'fp32-grads'])
@pytest.mark.parametrize('config', list(CONFIGS))
def test_mixed_step_has_the_bits_of_the_fp32_step(dev, config, grad_dtype):
    from ampnet_amd import FusedAdam
    kw, step_kw = CONFIGS[config]
    params, grads = _data()
    ps = [torch.nn.Parameter(t) for t in _tensors(params, DTYPES, dev)]
    twins = [torch.nn.Parameter(p.detach().float().clone()) for p in ps]          # the widened parameters, all aligned
    assert ps[SLICE].data_ptr() % 8 == 2 and twins[SLICE].data_ptr() % 16 == 0
    opt, twin = FusedAdam(ps, lr=LR, **kw), FusedAdam(twins, lr=LR, **kw)
    for k in range(STEPS):
        gs = _tensors(grads[k], [grad_dtype] * len(ps), dev)                     # (p.grad itself has to be of p's dtype)
        gs[NO_GRAD] = None
        _attach(twins, _tensors(grads[k], [F32] * len(ps), dev, sliced=False))
        opt.step(grads=gs, **step_kw)
        twin.step(**step_kw)
        for i, (p, q) in enumerate(zip(ps, twins)):
            what = f'{config}, step {k + 1}, tensor {i} {tuple(p.shape)} {p.dtype}'
            if i == NO_GRAD:
                assert p not in opt.state and q not in twin.state
                continue
            st, tw = opt.state[p], twin.state[q]
            assert st['step'] == tw['step'] == k + 1
            assert _bits(st['exp_avg'], tw['exp_avg']), f"{what}: exp_avg: {_diff(st['exp_avg'], tw['exp_avg'])}"
            assert _bits(st['exp_avg_sq'], tw['exp_avg_sq']), f"{what}: exp_avg_sq: {_diff(st['exp_avg_sq'], tw['exp_avg_sq'])}"
            if p.dtype == BF16:
                assert st['master'].dtype == F32 and _bits(st['master'], q.detach()), f"{what}: {_diff(st['master'], q)}"
                assert _bits(p.detach(), st['master'].to(BF16)), what
            else:
                assert 'master' not in st and _bits(p.detach(), q.detach()), f'{what}: {_diff(p, q)}'
        if opt.grad_norm is not None or twin.grad_norm is not None:
            assert _bits(opt.grad_norm, twin.grad_norm), f'{config}, step {k + 1}: {float(opt.grad_norm)} vs {float(twin.grad_norm)}'
    assert (opt.grad_norm is not None) == (config in ('clip', 'track'))
    assert not _bits(ps[3].detach().float(), torch.from_numpy(mixed.bf16_round(params[3])).to(dev))       # it did step


def _table(kind, rows):
    return (kind * len(rows))(*rows)


def test_fp32_descriptors_through_the_mixed_entry_points(dev):
    """The same fp32 values through ampconv_adam_* and through ampconv_adam_mixed_* (dtype codes F32, master NULL): every
    output and the norm bit for bit over three steps -- and once more through the mixed entry points with EVERY tensor
    4-byte aligned only, which changes no bit.  (The fp32 step itself is not held to that: on a tensor that is not 16-byte
    aligned it rounds its denominator twice, see "ROUNDING" in csrc/optim.hip; its tensors are the aligned ones here.)"""
    from ampnet_amd import _lib
    lib = _lib.load()
    shapes = ref.SIZES + [(4,), (5,), (1023,), (37,)]
    params = ref.make_params(shapes, 3)
    zeros = [np.zeros_like(a) for a in params]
    place = {False: lambda a: torch.from_numpy(a).to(dev), True: lambda a: _sliced(a, dev, F32)}
    sets = {name: {k: [place[cut](a) for a in arrays] for k, arrays in (('p', params), ('m', zeros), ('v', zeros))}
            for name, cut in (('fp32 entry points', False), ('mixed', False), ('mixed, unaligned', True))}
    norms = {name: torch.zeros((), device=dev) for name in sets}
    n = len(shapes)
    for k in range(3):
        grads = ref.make_grads(shapes, 20 + k)
        tail = (LR / (1 - 0.9 ** (k + 1)), 1.0 / np.sqrt(1 - 0.999 ** (k + 1)))
        for name, ts in sets.items():
            gs = [place[name.endswith('unaligned')](g) for g in grads]
            if name == 'fp32 entry points':
                kind, fill, prefix = _lib.AdamTensor, lambda row: row[:4] + row[5:8], 'ampconv_adam_'
            else:
                kind, fill, prefix = _lib.AdamMixedTensor, lambda row: row, 'ampconv_adam_mixed_'
            table = _table(kind, [fill((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, p.numel()) + tail
                                       + (_lib.AMPCONV_F32, _lib.AMPCONV_F32)) for p, g, m, v in zip(ts['p'], gs, ts['m'], ts['v'])])
            need = getattr(lib, prefix + 'workspace_bytes')(table, n)
            assert need == 4 * sum(-(-int(np.prod(s)) // 1024) for s in shapes)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            assert getattr(lib, prefix + 'grad_norm')(table, n, 0.5, norms[name].data_ptr(), ws.data_ptr(), need, None) == 0
            assert getattr(lib, prefix + 'step')(table, n, LR, 0.9, 0.999, 1e-8, WD, 0, 0.5, norms[name].data_ptr(), 1.0,
                                                 None) == 0
            torch.cuda.synchronize()
        want = sets['fp32 entry points']
        assert float(norms['fp32 entry points']) > 1.0                             # (so the clipping coefficient is at work)
        for name in ('mixed', 'mixed, unaligned'):
            assert _bits(norms[name], norms['fp32 entry points']), name
            for key in ('p', 'm', 'v'):
                for i, (a, b) in enumerate(zip(sets[name][key], want[key])):
                    assert _bits(a, b), f'{name}: {key}[{i}] {shapes[i]} after step {k + 1}: {_diff(a, b)}'
    assert ctypes.sizeof(_lib.AdamMixedTensor) == 64


def _rel(got, want, name):
    got, want = got.detach().double().cpu().numpy(), np.asarray(want, np.float64)
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f'[tol] {name}: max err {err:.3e} = {err / top if top else 0.0:.3e} of max |want| {top:.3e} (bar 1e-5)')
    assert err <= 1e-5 * top, f'{name}: max err {err:.3e} over 1e-5 * {top:.3e}'


@pytest.mark.parametrize('n', [25, 49])
def test_more_tensors_than_one_launch_holds(dev, n):
    """25 and 49 five-element tensors: two and three launches of at most 24 descriptors.  bf16 parameters carry bf16
    gradients, fp32 ones fp32; one more, empty, tensor sits inside the second launch (bf16 behind 25, fp32 behind 49).  Tolerances of tests/test_gpu_optim.py: the master at the flat fp32 bar, the
    moments at 1e-5 of the tensor's largest value, the norm at rtol 1e-5."""
    from ampnet_amd import FusedAdam, optim
    assert optim.MAX_TENSORS == 24
    shapes = [(5,)] * n
    shapes.insert(30 if n > 30 else 25, (0,))
    kinds = [mixed.BF16 if i % 2 else mixed.F32 for i in range(len(shapes))]
    dts = [BF16 if k == mixed.BF16 else F32 for k in kinds]
    params = ref.make_params(shapes, 5)
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev, dt)) for a, dt in zip(params, dts)]
    opt = FusedAdam(ps, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    model = mixed.MixedAdam(params, kinds, lr=LR, weight_decay=WD, max_grad_norm=1.0)
    for k in range(2):
        grads = [mixed.bf16_round(g) if kd == mixed.BF16 else g for g, kd in zip(ref.make_grads(shapes, 50 + k), kinds)]
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(dev, p.dtype)
        opt.step()
        model.step(grads)
        got, want = float(opt.grad_norm), model.norm
        print(f'[tol] grad_norm of {n} tensors, step {k + 1}: rel err {abs(got - want) / want:.3e} (bar 1e-5)')
        assert abs(got - want) <= 1e-5 * want
    values = [opt.state[p]['master'] if p.dtype == BF16 else p.detach() for p in ps]
    assert_close_scaled(torch.cat(values).cpu().numpy(), np.concatenate(model.master), f'master of {n} tensors', scaled=False)
    _rel(torch.cat([opt.state[p]['exp_avg'] for p in ps]), np.concatenate(model.m), f'exp_avg of {n} tensors')
    _rel(torch.cat([opt.state[p]['exp_avg_sq'] for p in ps]), np.concatenate(model.v), f'exp_avg_sq of {n} tensors')
    assert all(_bits(p.detach(), opt.state[p]['master'].to(BF16)) for p in ps if p.dtype == BF16)


def _run(dev, ks, opt=None, ps=None, **kw):
    from ampnet_amd import FusedAdam
    params, grads = _data()
    if ps is None:
        ps = [torch.nn.Parameter(t) for t in _tensors(params, DTYPES, dev)]
        opt = FusedAdam(ps, lr=LR, weight_decay=WD, max_grad_norm=3.0, **kw)
    for k in ks:
        _attach(ps, _tensors(grads[k], [p.dtype for p in ps], dev))
        opt.step()
    return opt, ps


def _snapshot(opt, ps):
    out = []
    for i, p in enumerate(ps):
        st = opt.state.get(p, {})
        out += [p.detach().clone()] + [st[k].clone() for k in ('exp_avg', 'exp_avg_sq', 'master') if k in st]
    return out + [opt.grad_norm.clone()]


def test_state_dict_round_trip_and_a_state_without_master(dev):
    from ampnet_amd import FusedAdam
    straight = _snapshot(*_run(dev, range(5)))
    opt, ps = _run(dev, range(2))
    sd = opt.state_dict()
    assert sorted(sd['state'][1]) == ['exp_avg', 'exp_avg_sq', 'master', 'step'] and sd['state'][1]['master'].dtype == F32
    assert sorted(sd['state'][0]) == ['exp_avg', 'exp_avg_sq', 'step'] and NO_GRAD not in sd['state']
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    again = FusedAdam(qs)
    again.load_state_dict(sd)
    assert again.max_grad_norm is None
    again.max_grad_norm = 3.0                                                      # (an optimizer attribute, not a group key)
    for q in qs:
        if q in again.state:
            assert all(again.state[q][k].dtype == F32 for k in ('exp_avg', 'exp_avg_sq'))
    _run(dev, range(2, 5), again, qs)
    resumed = _snapshot(again, qs)
    assert len(resumed) == len(straight) and all(_bits(a, b) for a, b in zip(resumed, straight))
    # a state that lacks the master (e.g. written by torch.optim.Adam over the bf16 tensors): recreated from p at the step
    sd = {'state': {i: {k: v for k, v in st.items() if k != 'master'} for i, st in sd['state'].items()},
          'param_groups': sd['param_groups']}
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    bare = FusedAdam(rs)
    bare.load_state_dict(sd)
    assert all('master' not in bare.state[r] for r in rs if r in bare.state)
    before = rs[3].detach().clone()
    _run(dev, [2], bare, rs)
    m = bare.state[rs[3]]['master']
    assert m.dtype == F32 and _bits(rs[3].detach(), m.to(BF16)) and not torch.equal(m, before.float())
    assert (m - before.float()).abs().max() <= 1.01 * LR * 3.2                     # one Adam update away from p


CFG = dict(embedding_dim=8, num_heads=2, num_node_features=11, num_sampled_vectors=4, output_dim=3, feat_emb_dim=7,
           dropout_rate=0.0, dropout_adj_rate=0.0)


def test_full_precision_state_dict_under_the_references_keys(dev):
    from ampnet_amd import AMPGCN, FusedAdam
    torch.manual_seed(7)
    model = AMPGCN(device=dev, storage_dtype=BF16, **CFG).to(dev)
    opt = FusedAdam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(8)
    for _ in range(3):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(dev, p.dtype)
        opt.step()
    sd = opt.full_precision_state_dict(model)
    plain = AMPGCN(device=dev, **CFG).to(dev)
    assert list(sd) == list(plain.state_dict()) and all(t.dtype == F32 for t in sd.values())
    named = dict(model.named_parameters())
    for k, t in sd.items():
        if named[k].dtype == BF16:
            assert _bits(t, opt.state[named[k]]['master']) and t.data_ptr() != opt.state[named[k]]['master'].data_ptr()
            assert not torch.equal(t, named[k].detach().float())                   # the master holds bits the parameter cannot
        else:
            assert _bits(t, named[k].detach())
    plain.load_state_dict(sd, strict=True)                                         # an fp32 model takes it as it is
    # ... and the way back into a fresh bf16 model and optimizer: exact masters, rounded parameters
    fresh = AMPGCN(device=dev, storage_dtype=BF16, **CFG).to(dev)
    other = FusedAdam(fresh.parameters(), lr=1e-3)
    other.load_full_precision_state_dict(fresh, sd)
    for (k, p), (_, q) in zip(fresh.named_parameters(), model.named_parameters()):
        assert _bits(p.detach(), q.detach()), k
        if p.dtype == BF16:
            assert _bits(other.state[p]['master'], sd[k]) and 'step' not in other.state[p]
    for p in fresh.parameters():
        p.grad = torch.ones_like(p)
    other.step()                                                                   # the first step keeps the loaded master
    p = fresh.conv1.multi_head_attention.in_proj_weight
    assert other.state[p]['step'] == 1
    torch.testing.assert_close(other.state[p]['master'], sd['conv1.multi_head_attention.in_proj_weight'] - 1e-3,
                               rtol=0, atol=1e-6)
    with pytest.raises(KeyError, match='missing'):
        other.load_full_precision_state_dict(fresh, {k: v for k, v in sd.items() if 'bias' not in k})


def test_refused_arguments_at_the_c_boundary(dev):
    from ampnet_amd import _lib
    lib = _lib.load()
    F, B = _lib.AMPCONV_F32, _lib.AMPCONV_BF16
    p, g, m, v, master = (torch.randn(2000, device=dev) for _ in range(5))
    p16, g16 = torch.randn(2000, device=dev).to(BF16), torch.randn(2000, device=dev).to(BF16)
    watched = (p, m, v, master, p16)
    before = [t.clone() for t in watched]
    norm, ws = torch.full((), 7.0, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    good = (p16.data_ptr(), g16.data_ptr(), m.data_ptr(), v.data_ptr(), master.data_ptr(), 2000, 0.1, 1.0, B, B)
    good32 = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, 2000, 0.1, 1.0, F, F)
    hyper = dict(lr=0.1, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=0, grad_scale=1.0, norm=None,
                 max_grad_norm=0.0)

    def table(*rows):
        return _table(_lib.AdamMixedTensor, rows)

    def step(t, n, **kw):
        a = {**hyper, **kw}
        return lib.ampconv_adam_mixed_step(t, n, a['lr'], a['beta1'], a['beta2'], a['eps'], a['weight_decay'], a['decoupled'],
                                           a['grad_scale'], a['norm'], a['max_grad_norm'], None)

    def refused(row):
        t = table(good32, tuple(row))                                              # behind a good one: nothing may be launched
        assert step(t, 2) == -1, row
        assert lib.ampconv_adam_mixed_grad_norm(t, 2, 1.0, norm.data_ptr(), ws.data_ptr(), 64, None) == -1, row
        assert lib.ampconv_adam_mixed_workspace_bytes(t, 2) == 0, row

    for code in (2, -1, 7):                                                        # a dtype code other than F32 / BF16
        refused(good[:8] + (code, B))
        refused(good[:8] + (B, code))
    refused(good[:4] + (None,) + good[5:])                                         # a bf16 p without a master
    refused(good32[:4] + (master.data_ptr(),) + good32[5:])                        # an fp32 p with one
    refused(good32[:4] + (master.data_ptr(), 0) + good32[6:])                      # ... also where there is nothing to do
    for hole in range(4):                                                          # what the fp32 entry points refuse
        row = list(good)
        row[hole] = None
        refused(row)
    refused(good[:5] + (-1,) + good[6:])
    one = table(good)
    assert step(one, -1) == -1 and step(None, 1) == -1
    for kw in ({'lr': -0.1}, {'eps': 0.0}, {'beta1': 1.0}, {'beta2': -0.1}, {'weight_decay': -1e-4},
               {'norm': norm.data_ptr(), 'max_grad_norm': 0.0}):
        assert step(one, 1, **kw) == -1, kw
    need = lib.ampconv_adam_mixed_workspace_bytes(one, 1)
    assert need == 2 * 4
    assert lib.ampconv_adam_mixed_grad_norm(one, 1, 1.0, None, ws.data_ptr(), 64, None) == -1
    assert lib.ampconv_adam_mixed_grad_norm(one, 1, 1.0, norm.data_ptr(), ws.data_ptr(), need - 1, None) == -3
    assert lib.ampconv_adam_mixed_grad_norm(one, 1, 1.0, norm.data_ptr(), None, 0, None) == -3
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(watched, before)) and float(norm) == 7.0
    # nothing to do is no error: no tensors, empty tensors of either dtype (a bf16 one needs no master then)
    assert step(None, 0) == 0 and step(table(good[:5] + (0,) + good[6:]), 1) == 0
    assert step(table((None, None, None, None, None, 0, 0.1, 1.0, B, F)), 1) == 0
    assert lib.ampconv_adam_mixed_grad_norm(None, 0, 1.0, norm.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(watched, before)) and float(norm) == 0.0


def test_other_dtypes_are_refused_at_step(dev):
    from ampnet_amd import FusedAdam
    for dt in (torch.float16, torch.float64):
        p = torch.nn.Parameter(torch.ones(8, device=dev, dtype=dt))
        p.grad = torch.ones_like(p)
        opt = FusedAdam([p])
        with pytest.raises(ValueError, match='float32 or bfloat16 parameters'):
            opt.step()
        assert len(opt.state) == 0 and torch.equal(p.detach(), torch.ones_like(p))
    p = torch.nn.Parameter(torch.ones(8, device=dev, dtype=BF16))
    p.grad = None
    opt = FusedAdam([p])
    with pytest.raises(ValueError, match='float32 or bfloat16 gradients'):
        opt.step(grads=[torch.ones(8, device=dev, dtype=torch.float16)])
    assert len(opt.state) == 0


def test_the_stall_case_moves_on_the_device(dev):
    """tests/test_bf16_model_cpu.py: torch.optim.Adam leaves this bf16 parameter at exactly 1.0.  Here the master walks
    down by lr a step and the parameter follows it in bf16 steps."""
    from ampnet_amd import FusedAdam
    p = torch.nn.Parameter(torch.ones(1, device=dev, dtype=BF16))
    opt = FusedAdam([p], lr=1e-3)
    g = torch.ones(1, device=dev, dtype=BF16)
    seen = set()
    for _ in range(100):
        opt.step(grads=[g])
        seen.add(p.item())
    master = opt.state[p]['master'].item()
    assert abs(master - 0.9) < 1e-4 and p.item() == 0.8984375 and p.dtype == BF16
    assert len(seen) > 20                                                          # bf16 values between 1.0 and 0.9: ulp 2^-8


def test_mixed_step_does_not_synchronise(dev):
    opt, ps = _run(dev, range(1), track_grad_norm=True)                            # warm up: library, state, allocator
    params, grads = _data()
    gs = _tensors(grads[1], [p.dtype for p in ps], dev)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        _attach(ps, gs)
        opt.step(set_to_none=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert all(p.grad is None for p in ps) and opt.state[ps[1]]['step'] == 2
