"""CPU checks of AMPConvFunction's path choice (functional.choose_plan, LayerPlan.backward): which projections,
projection arithmetic, edge family and node lists a layer call gets, and which data-dependent inputs the choice asks
for.  The support predicates it calls are host-only; the data-dependent inputs are plain lambdas here."""
import pytest
import torch

from test_abi import built  # noqa: F401  (builds libampconv.so)

F32, BF16 = torch.float32, torch.bfloat16
CFG4, CFG3, CFG3_L4 = (1_000_000, 20, 256, 8), (100_000, 20, 128, 8), (100_000, 4, 128, 8)
CLASS_DEFAULT, CORA = (100_000, 40, 100, 2), (2708, 20, 128, 4)


def _choose(shape, shared=True, dtype=F32, gemm='native', x=True, xkv=True, nodes=None, full_graph=True,
            capturing=False):
    """(plan, the data-dependent inputs it asked for, in order)."""
    from ampnet_amd.conv import functional as F_
    N, L, D, H = shape
    asked = []

    def ask(name, value):
        return lambda: asked.append(name) or value
    plan = F_.choose_plan(L, D, H, shared, dtype, gemm, N * L * D, ask('x', x), ask('xkv', xkv),
                          ask('nodes', nodes) if full_graph else None, ask('capturing', capturing))
    return plan, [a for a in asked if a != 'capturing']


LISTS = {'in': 'i', 'out': 'o', 'any': 'a'}
CASES = {
    # name: (shape, choose kwargs, module switches, expected (native, scaled, edge, lists), inputs asked for)
    'cfg4-narrow': (CFG4, {}, {}, (True, True, 'planes', None), ['x']),
    'cfg3-narrow': (CFG3, {}, {}, (True, True, 'planes', None), ['x']),
    'cfg4-wide': (CFG4, {'x': False}, {}, (True, False, 'plain', None), ['x']),
    'cfg3-wide': (CFG3, {'x': False}, {}, (True, False, 'plain', None), ['x']),
    'cfg3-L4': (CFG3_L4, {}, {}, (True, True, 'plain', None), ['x']),
    'class-default': (CLASS_DEFAULT, {}, {}, (True, True, 'views', None), ['x']),
    'class-default-no-stats': (CLASS_DEFAULT, {}, {'SOFTMAX_STATS': False}, (True, True, 'plain', None), ['x']),
    'cora': (CORA, {}, {}, (True, False, 'plain', None), []),
    'captured': (CFG4, {'capturing': True}, {}, (True, False, 'plain', None), []),
    'gemm-fp32': (CFG4, {'gemm': 'fp32'}, {}, (False, False, 'plain', None), []),
    'bf16-lists': (CFG4, {'dtype': BF16, 'nodes': LISTS}, {}, (True, False, 'plain', LISTS), ['nodes']),
    'bf16-no-lists': (CFG4, {'dtype': BF16}, {}, (True, False, 'plain', None), ['nodes']),
    'bf16-node-lists-off': (CFG4, {'dtype': BF16, 'nodes': LISTS}, {'NODE_LISTS': False}, (True, False, 'plain', None),
                            []),
    'bf16-message': (CFG4, {'dtype': BF16, 'shared': False, 'nodes': LISTS}, {}, (True, False, 'plain', None), []),
    'bf16-not-the-graph': (CFG4, {'dtype': BF16, 'nodes': LISTS, 'full_graph': False}, {},
                           (True, False, 'plain', None), []),
    'message-narrow': (CFG4, {'shared': False}, {}, (True, True, 'plain', None), ['x', 'xkv']),
    'message-wide-xkv': (CFG4, {'shared': False, 'xkv': False}, {}, (True, False, 'plain', None), ['x', 'xkv']),
    'message-wide-x': (CFG4, {'shared': False, 'x': False}, {}, (True, False, 'plain', None), ['x']),
    'edge-planes-off': (CFG4, {}, {'EDGE_PLANES': False}, (True, True, 'plain', None), ['x']),
    'class-default-edge-planes-off': (CLASS_DEFAULT, {}, {'EDGE_PLANES': False}, (True, True, 'plain', None), ['x']),
    'proj-scaled-off': (CFG4, {}, {'PROJ_SCALED': False}, (True, False, 'plain', None), []),
}


@pytest.mark.parametrize('name', list(CASES))
def test_choose_plan(built, monkeypatch, name):  # noqa: F811
    from ampnet_amd import _lib
    from ampnet_amd.conv import functional as F_
    shape, kw, switches, (native, scaled, edge, lists), asked = CASES[name]
    for k, v in switches.items():
        monkeypatch.setattr(F_, k, v)
    plan, got = _choose(shape, **kw)
    assert (plan.native, plan.scaled, plan.edge, plan.lists) == (native, scaled, edge, lists)
    assert got == asked
    assert (plan.L, plan.D, plan.H) == shape[1:] and plan.shared == kw.get('shared', True)
    assert plan.dtype == (_lib.AMPCONV_BF16 if kw.get('dtype') == BF16 else _lib.AMPCONV_F32)
    assert not plan.qkv_to_f32
    assert plan.backward(True) is plan                  # a narrow dY keeps the forward pass's plan


@pytest.mark.parametrize('name', ['cfg4-narrow', 'class-default', 'cfg3-L4', 'cora'])
def test_wide_gradient_sends_the_backward_pass_to_the_exact_kernels(built, name):  # noqa: F811
    shape, kw, _, _, _ = CASES[name]
    plan, _ = _choose(shape, **kw)
    back = plan.backward(False)
    assert (back.native, back.scaled, back.edge) == (plan.native, False, 'plain')
    assert back.qkv_to_f32 == (plan.edge == 'planes')   # only the plane format has to read qkv back as fp32
    assert (back.L, back.D, back.H, back.shared, back.dtype, back.gemm) == \
        (plan.L, plan.D, plan.H, plan.shared, plan.dtype, plan.gemm)
