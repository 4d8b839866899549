"""The per-node products of the softmax-free path and the per-edge side outputs, ONE C CALL AT A TIME through ctypes:
ampconv_linear_outer, ampconv_linear_apply (csrc/linear_ops.hip), ampconv_attn_scores, ampconv_attn_weights
(csrc/edge_generic.hip), each against its fp64 model of tests/linear_reference.py.

View operands lie in NaN margins and gaps and view outputs in sentinel ones (edge_layouts.place), M and W inside a
larger allocation of the same kind (edge_layouts.place_flat); after every call nothing outside the output may have
changed and everything inside must have been written.  The bars are linear_reference's: exact data (small integers,
scale 1 or 1/2) bit-equal to the model, random data within (n + 4) 2^-24 S; attn_weights at the project's flat bar with
rows that sum to 1.  tests/test_linear_reference_cpu.py shows that these bars reject an M for an M^T, a wrong head
stride and an ignored scale.  Every sweep names all its failing cases in one assertion."""
import numpy as np
import pytest
import torch

import linear_reference as lr
from edge_layouts import LAYOUTS, place, place_flat
from edge_runner import graph, stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

F32 = torch.float32
N = 40
SHAPES = [(1, 2, 1), (5, 6, 3), (3, 7, 2), (17, 16, 8), (20, 32, 4), (40, 50, 2), (64, 64, 1)]
EDGE_SHAPES = [(1, 2, 1), (5, 6, 3), (3, 7, 2), (20, 32, 4), (40, 50, 2), (64, 64, 1), (65, 4, 2), (100, 8, 2)]
BADARG, EDTYPE = -1, -2
SHARE = {}          # call -> the largest share of the random-data bound used, printed by every test that raises it


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def raw(p):
    """The float32 values of a placed buffer, bit for bit."""
    return p.backing[p.index.reshape(-1)].reshape(p.index.shape).cpu().numpy()


def sid(shape):
    return 'L{}dh{}H{}'.format(*shape)


def written(p, name):
    bad = []
    if not p.outside_intact():
        bad.append(f'{name}: bytes outside the output were written')
    if p.unwritten():
        bad.append(f'{name}: {p.unwritten()} elements of the output were not written')
    return bad


def untouched(p, name):
    return [] if p.outside_intact() and p.unwritten() == p.index.numel() else [f'{name}: the output was written']


def judge(call, name, kind, got, ref, S, n):
    """The bar of `kind` -> a list of problems; keeps the largest share of the random-data bound per call."""
    if kind == 'exact':
        miss = lr.exact_problems(got, ref)
        return [f'{name}: {miss}/{got.size} elements are not bit-equal to the model'] if miss else []
    share = lr.random_share(got, ref, S, n)
    if share > SHARE.get(call, 0.0):
        SHARE[call] = share
        print(f'[bar] {call}: {100 * share:.1f} % of (n + 4) 2^-24 S at {name}')
    return [f'{name}: {share:.3g} times the bound (n + 4) 2^-24 S'] if share > 1 else []


def run_outer(lib, shape, layout, kind, scale, n_nodes=N):
    L, dh, H = shape
    name = f'outer {sid(shape)} {layout} {kind} scale={scale:.3g}'
    A, B = lr.tiles(kind, shape, n_nodes), lr.tiles(kind, shape, n_nodes, seed=1)
    pa, pb, pm = place(A, layout, F32, 'Q'), place(B, layout, F32, 'K'), place_flat((n_nodes, H, dh, dh), F32)
    rc = lib.ampconv_linear_outer(pa.view, pb.view, n_nodes, L, dh * H, H, scale, pm.ptr, stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}'] + untouched(pm, name)
    ref, S = lr.linear_outer(A, B, np.float32(scale))
    return written(pm, name) + judge('linear_outer', name, kind, raw(pm), ref, S, L)


def run_apply(lib, shape, layout, kind, transpose, scale, n_nodes=N, M=None):
    L, dh, H = shape
    name = f'apply{"^T" if transpose else ""} {sid(shape)} {layout} {kind} scale={scale:.3g}'
    A = lr.tiles(kind, shape, n_nodes)
    M = lr.matrices(kind, shape, n_nodes) if M is None else M
    pa, pm, po = place(A, layout, F32, 'Q'), place_flat(M, F32), place((n_nodes, L, H, dh), layout, F32, 'out0')
    rc = lib.ampconv_linear_apply(pa.view, pm.ptr, transpose, n_nodes, L, dh * H, H, scale, po.view, stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}'] + untouched(po, name)
    ref, S = lr.linear_apply(A, M, transpose, np.float32(scale))
    return written(po, name) + judge('linear_apply', name, kind, raw(po), ref, S, dh)


def three_calls(lib, shape, layout, kind, scale):
    return (run_outer(lib, shape, layout, kind, scale) + run_apply(lib, shape, layout, kind, 0, scale) +
            run_apply(lib, shape, layout, kind, 1, scale))


# ------------------------------------------------------------------------------------------ linear_outer, linear_apply
@pytest.mark.parametrize('kind', ['exact', 'random'])
def test_outer_and_apply_at_every_shape(kind, lib):
    """L * dh and dh * dh below one wavefront, and no multiple of it; the odd head width 7 (dh | 1 = dh: no padding
    column); `scale` honoured: 1 and 1/2 on exact data, 1 / sqrt(dh) on random data."""
    failed = []
    for shape in SHAPES:
        for scale in ((1.0, 0.5) if kind == 'exact' else (float(np.float32(shape[1] ** -0.5)),)):
            failed += three_calls(lib, shape, 'nld', kind, scale)
    assert not failed, failed


@pytest.mark.parametrize('layout', LAYOUTS + ('mixed',))
def test_outer_and_apply_under_every_layout(layout, lib):
    failed = []
    for shape in ((20, 32, 4), (5, 6, 3)):
        failed += three_calls(lib, shape, layout, 'exact', 0.5)
        failed += three_calls(lib, shape, layout, 'random', float(np.float32(shape[1] ** -0.5)))
    assert not failed, failed


@pytest.mark.parametrize('dh,H', [(6, 3), (50, 2)])
def test_outer_and_apply_at_every_token_count(dh, H, lib):
    failed = []
    for L in range(1, 65):
        failed += three_calls(lib, (L, dh, H), 'nld', 'exact', 0.5)
    assert not failed, failed


@pytest.mark.parametrize('shape', [(5, 6, 3), (3, 7, 2), (20, 32, 4)], ids=sid)
def test_apply_tells_a_nearly_symmetric_matrix_from_its_transpose(shape, lib):
    """M = M^T but for ONE element of one (node, head): the two transposes differ in two output columns of one unit."""
    L, dh, H = shape
    M = lr.matrices('exact', shape, N)
    M = M + M.transpose(0, 1, 3, 2)
    M[N // 2, H - 1, 0, dh - 1] += 1
    failed = run_apply(lib, shape, 'nld', 'exact', 0, 0.5, M=M) + run_apply(lib, shape, 'nld', 'exact', 1, 0.5, M=M)
    assert not failed, failed
    a, b = (lr.linear_apply(lr.tiles('exact', shape, N), M, t, 0.5)[0] for t in (0, 1))
    assert 0 < (a != b).sum() <= 2 * L                # the models themselves differ, in columns 0 and dh - 1 of one unit


@pytest.mark.parametrize('call,shape', [('outer', (126, 64, 1)), ('apply', (188, 64, 1))], ids=['outer', 'apply'])
def test_largest_shape_the_64_KiB_of_LDS_allow(call, shape, lib):
    """2 * 126 * 65 * 4 = (188 + 64) * 65 * 4 = 65520 bytes of dynamic LDS: the largest launches the calls make."""
    failed = []
    for kind in ('exact', 'random'):
        if call == 'outer':
            failed += run_outer(lib, shape, 'nld', kind, 0.5, n_nodes=3)
        else:
            failed += run_apply(lib, shape, 'nld', kind, 0, 0.5, n_nodes=3) + run_apply(lib, shape, 'nld', kind, 1, 0.5, n_nodes=3)
    assert not failed, failed


def test_one_token_more_is_refused_and_writes_nothing(lib):
    bad = run_outer(lib, (127, 64, 1), 'nld', 'exact', 1.0, n_nodes=3) + run_apply(lib, (189, 64, 1), 'nld', 'exact', 0, 1.0, n_nodes=3)
    assert len(bad) == 2 and all(b.endswith('returned -1') for b in bad), bad


def test_outer_and_apply_refusals_and_the_empty_call(lib):
    shape = (5, 6, 3)
    L, dh, H = shape
    D = dh * H
    A, M = lr.tiles('exact', shape, N), lr.matrices('exact', shape, N)
    pa, pb, pm_in = place(A, 'nld', F32, 'Q'), place(A, 'nld', F32, 'K'), place_flat(M, F32)
    zero = _lib.View(pa.view.ptr, 0, 0, 0)
    for label, args, want in (('N = 0', (pa.view, pb.view, 0, L, D, H), 0),
                              ('zero-stride A', (zero, pb.view, N, L, D, H), BADARG),
                              ('zero-stride B', (pa.view, zero, N, L, D, H), BADARG),
                              ('D % H != 0', (pa.view, pb.view, N, L, D + 1, H), BADARG)):
        pm = place_flat((N, H, dh, dh), F32)
        assert lib.ampconv_linear_outer(*args, 1.0, pm.ptr, stream()) == want, label
        torch.cuda.synchronize()
        assert not untouched(pm, label)
    assert lib.ampconv_linear_outer(pa.view, pb.view, N, L, D, H, 1.0, None, stream()) == BADARG
    for label, args, want in (('N = 0', (pa.view, pm_in.ptr, 0, 0, L, D, H), 0),
                              ('NULL M', (pa.view, None, 0, N, L, D, H), BADARG),
                              ('zero-stride A', (zero, pm_in.ptr, 0, N, L, D, H), BADARG),
                              ('D % H != 0', (pa.view, pm_in.ptr, 0, N, L, D + 1, H), BADARG)):
        po = place((N, L, H, dh), 'nld', F32, 'out0')
        assert lib.ampconv_linear_apply(*args, 1.0, po.view, stream()) == want, label
        torch.cuda.synchronize()
        assert not untouched(po, label)
    po = place((N, L, H, dh), 'nld', F32, 'out0')
    assert lib.ampconv_linear_apply(pa.view, pm_in.ptr, 0, N, L, D, H, 1.0, _lib.View(po.view.ptr, 0, 0, 0), stream()) == BADARG
    torch.cuda.synchronize()
    assert not untouched(po, 'zero-stride Out')


# ------------------------------------------------------------------------------------------ attn_scores, attn_weights
def shuffled_edges():
    """Graph A's 703 edges -- multi-edges, self-loops, a hub destination and a hub source -- in a seeded random order."""
    g = graph('A')
    order = np.random.default_rng(23).permutation(g.E)
    return g.N, g.src[order], g.dst[order]


def run_edge_call(lib, which, shape, layout, kind, models):
    L, dh, H = shape
    n_nodes, src, dst = shuffled_edges()
    name = f'{which} {sid(shape)} {layout} {kind}'
    Q, K = lr.tiles(kind, shape, n_nodes), lr.tiles(kind, shape, n_nodes, seed=1)
    if (which, shape, kind) not in models:
        models[which, shape, kind] = getattr(lr, which)(Q, K, src, dst)
    ref, S = models[which, shape, kind]
    pq, pk, pw = place(Q, layout, F32, 'Q'), place(K, layout, F32, 'K'), place_flat((len(src), L, L), F32)
    ei = torch.from_numpy(np.stack([src, dst])).cuda()
    rc = getattr(lib, 'ampconv_' + which)(pq.view, pk.view, ei.data_ptr(), len(src), L, dh * H, H, pw.ptr, _lib.AMPCONV_F32,
                                          stream())
    torch.cuda.synchronize()
    if rc != 0:
        return [f'{name}: returned {rc}'] + untouched(pw, name)
    got = raw(pw)
    if which == 'attn_weights':
        share = lr.weights_share(got, ref)
        if share > SHARE.get(which, 0.0):
            SHARE[which] = share
            print(f'[bar] attn_weights: {100 * share:.1f} % of the flat bar / the row-sum bar at {name}')
        return written(pw, name) + ([f'{name}: {share:.3g} times the flat bar or the row-sum bar'] if share > 1 else [])
    return written(pw, name) + judge(which, name, kind, got, ref, S, dh)


@pytest.fixture(scope='module')
def models():
    return {}


@pytest.mark.parametrize('layout', ['nld', 'packed3', 'mixed'])
@pytest.mark.parametrize('which', ['attn_scores', 'attn_weights'])
def test_side_outputs_on_a_shuffled_edge_list(which, layout, lib, models):
    """Original edge order, every shape of the list ((65, 4, 2) and (100, 8, 2): the column loop passes one wavefront),
    random data; attn_scores on exact data too where sqrt(dh) and H are powers of two (bit-equal there)."""
    failed = []
    for shape in EDGE_SHAPES:
        failed += run_edge_call(lib, which, shape, layout, 'random', models)
        if which == 'attn_scores' and shape in ((64, 64, 1), (65, 4, 2)):
            failed += run_edge_call(lib, which, shape, layout, 'exact', models)
    assert not failed, failed


@pytest.mark.parametrize('which', ['attn_scores', 'attn_weights'])
def test_side_outputs_empty_edge_list_and_bf16(which, lib):
    shape = (5, 6, 3)
    L, dh, H = shape
    Q = lr.tiles('random', shape, 8)
    pq, pk = place(Q, 'nld', F32, 'Q'), place(Q, 'nld', F32, 'K')
    ei = torch.zeros(2, 4, dtype=torch.int64, device='cuda:0')
    fn = getattr(lib, 'ampconv_' + which)
    for label, E, dtype, want in (('E = 0', 0, _lib.AMPCONV_F32, 0), ('bf16', 4, _lib.AMPCONV_BF16, EDTYPE)):
        pw = place_flat((4, L, L), F32)
        assert fn(pq.view, pk.view, ei.data_ptr(), E, L, dh * H, H, pw.ptr, dtype, stream()) == want, label
        torch.cuda.synchronize()
        assert not untouched(pw, label)
