"""The pair loss without a GPU: the numpy model of tests/pair_loss_reference.py against torch's autograd in float64,
walk_pairs against a Python loop, the binding's signatures, the package exports and the argument errors that need no
device."""
import os
import re

import numpy as np
import pytest
import torch

import pair_loss_reference as ref
from conftest import ROOT

# two float64 computations of the same formulas over at most 40 x 50 x 24 terms of magnitude <= ~10
TOL = dict(rtol=1e-9, atol=1e-11)


def softplus(x):
    return torch.logaddexp(x, torch.zeros_like(x))             # F.softplus is linear above 20: off by e^-20 there


def torch_composite(z, anchor, positive, negative, weight, kind, scale, neg_weight, exclude_anchor):
    a, p, n = z[anchor], z[positive], z[negative]
    aff = scale * (a * p).sum(1)
    g = scale * a @ n.T
    kept = torch.ones_like(g, dtype=torch.bool)
    if exclude_anchor:
        kept = negative[None, :] != anchor[:, None]
    if kind == 'skipgram':
        neg = torch.logsumexp(g.masked_fill(~kept, -float('inf')), dim=1)
        neg = torch.where(kept.any(1), neg, torch.zeros_like(neg))
        rows = neg - aff
    else:
        neg = (softplus(g) * kept).sum(1)
        rows = softplus(-aff) + neg_weight * neg
    return (weight * rows).sum(), aff, neg


@pytest.mark.parametrize('kind', ['skipgram', 'xent'])
@pytest.mark.parametrize('exclude_anchor', [False, True])
@pytest.mark.parametrize('weighted', [False, True])
def test_numpy_model_matches_torch_autograd_in_float64(kind, exclude_anchor, weighted):
    N, D, B, S = 40, 24, 50, 33
    z, anchor, positive, negative, weight = ref.make_inputs(N, D, B, S, amp=2.0, seed=3)
    negative[:4] = anchor[:4]                                   # excluded pairs exist
    w = weight.astype(np.float64) if weighted else np.ones(B)
    opts = dict(kind=kind, scale=0.7, neg_weight=1.3, exclude_anchor=exclude_anchor)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    loss, aff, neg = torch_composite(zt, *(torch.from_numpy(t) for t in (anchor, positive, negative)),
                                     torch.from_numpy(w), **opts)
    (2.5 * loss).backward()
    got_loss, got_aff, got_neg, _, _ = ref.forward(z, anchor, positive, negative, w if weighted else None, **opts)
    dz = ref.backward(z, anchor, positive, negative, w if weighted else None, g0=2.5, **opts)
    np.testing.assert_allclose(got_loss, loss.item(), **TOL)
    np.testing.assert_allclose(got_aff, aff.detach().numpy(), **TOL)
    np.testing.assert_allclose(got_neg, neg.detach().numpy(), **TOL)
    np.testing.assert_allclose(dz, zt.grad.numpy(), **TOL)


@pytest.mark.parametrize('kind', ['skipgram', 'xent'])
def test_row_whose_only_negative_is_excluded(kind):
    z, _, _, _, _ = ref.make_inputs(6, 5, 1, 1, seed=1)
    anchor, positive, negative = np.array([2, 3]), np.array([4, 1]), np.array([2])     # pair 0: its only negative is its anchor
    loss, aff, neg, pi, c = ref.forward(z, anchor, positive, negative, kind=kind, exclude_anchor=True)
    assert neg[0] == 0.0 and (pi[0] == 0).all() and neg[1] != 0.0
    z64 = z.astype(np.float64)
    g1 = float(z64[3] @ z64[2])
    if kind == 'skipgram':
        want = (0.0 - aff[0]) + (g1 - aff[1])
    else:
        want = ref.softplus(-aff[0]) + ref.softplus(-aff[1]) + ref.softplus(g1)
    np.testing.assert_allclose(loss, want, **TOL)
    dz = ref.backward(z, anchor, positive, negative, kind=kind, exclude_anchor=True)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    torch_composite(zt, *(torch.from_numpy(t) for t in (anchor, positive, negative)), torch.ones(2, dtype=torch.float64),
                    kind, 1.0, 1.0, True)[0].backward()
    np.testing.assert_allclose(dz, zt.grad.numpy(), **TOL)


def test_empty_batch_and_clamped_ids():
    z, _, _, negative, _ = ref.make_inputs(9, 4, 0, 5, seed=2)
    empty = np.zeros(0, dtype=np.int64)
    assert ref.forward(z, empty, empty, negative)[0] == 0.0
    assert (ref.backward(z, empty, empty, negative) == 0).all()
    a, p = np.array([-1, 3]), np.array([9, 2 ** 40])
    np.testing.assert_array_equal(ref.backward(z, a, p, negative), ref.backward(z, [0, 3], [8, 8], negative))


@pytest.mark.parametrize('window,symmetric,relabel', [(1, False, False), (2, False, True), (3, True, True), (7, True, False)])
def test_walk_pairs_against_a_python_loop(window, symmetric, relabel):
    from ampnet_amd import walk_pairs
    rng = np.random.default_rng(window)
    node_idx = np.sort(rng.choice(500, 60, replace=False)).astype(np.int64)
    walks = node_idx[rng.integers(0, 60, (11, 5))]
    walks[3] = walks[3, 0]                                       # a walk that stays put: self pairs are kept
    idx = torch.from_numpy(node_idx) if relabel else None
    a, p = walk_pairs(torch.from_numpy(walks), idx, window=window, symmetric=symmetric)
    want_a, want_p = ref.walk_pairs(walks, node_idx if relabel else None, min(window, 4), symmetric)
    assert a.dtype == p.dtype == torch.int64
    np.testing.assert_array_equal(a.numpy(), want_a)
    np.testing.assert_array_equal(p.numpy(), want_p)
    assert len(want_a) == (2 if symmetric else 1) * 11 * sum(5 - k for k in range(1, min(window, 4) + 1))
    with pytest.raises(ValueError):
        walk_pairs(torch.from_numpy(walks), window=0)


def _c_parameters(name):
    """The parameter declarations of a function of include/ampconv.h."""
    header = open(os.path.join(ROOT, 'include', 'ampconv.h')).read()
    m = re.search(r'^(?:int|size_t) %s\(([^;]*)\);' % name, header, flags=re.M)
    assert m, f'{name} is not declared in include/ampconv.h'
    return [' '.join(p.split()) for p in m.group(1).split(',')]


def test_binding_declares_the_pair_loss_entry_points():
    import ctypes
    from ampnet_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'ampconv.h')).read()
    assert _lib.EXPECTED_ABI == int(re.search(r'#define\s+AMPCONV_VERSION\s+(\d+)', header).group(1))
    assert 'pair loss' in header
    for name in ('ampconv_pair_loss_workspace_bytes', 'ampconv_pair_loss_fwd', 'ampconv_pair_loss_bwd'):
        params = _c_parameters(name)
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(params), (name, len(args), len(params))
        for decl, ctype in zip(params, args):
            if '*' in decl:
                want = ctypes.c_void_p
            else:
                want = {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'float': ctypes.c_float,
                        'size_t': ctypes.c_size_t}[decl.split()[0]]
            assert ctype is want, (name, decl, ctype)
        assert res is (ctypes.c_size_t if name.endswith('bytes') else ctypes.c_int)


def test_package_exports_and_embed():
    import ampnet_amd
    for name in ('pair_loss', 'PairLoss', 'walk_pairs'):
        assert name in ampnet_amd.__all__ and hasattr(ampnet_amd, name), name
    assert callable(ampnet_amd.AMPGCN.embed)
    loss = ampnet_amd.PairLoss(kind='xent', neg_weight=2.0, exclude_anchor=True, reduction='mean')
    assert (loss.kind, loss.neg_weight, loss.exclude_anchor, loss.reduction) == ('xent', 2.0, True, 'mean')
    assert not list(loss.parameters())


def test_argument_errors_without_a_device():
    from ampnet_amd import PairLoss, pair_loss
    z = torch.zeros(10, 8)
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match='GPU'):
        pair_loss(z, ids, ids, ids)                                        # CPU tensors: no eager fallback
    with pytest.raises(ValueError, match='shape'):
        pair_loss(torch.zeros(10, 257), ids, ids, ids)
    with pytest.raises(ValueError, match='at least one negative'):
        pair_loss(z, ids, ids, ids[:0])
    with pytest.raises(ValueError, match='kind'):
        pair_loss(z, ids, ids, ids, kind='hinge')
    with pytest.raises(ValueError, match='kind'):
        PairLoss(kind='hinge')
    with pytest.raises(ValueError, match='reduction'):
        pair_loss(z, ids, ids, ids, reduction='max')
    with pytest.raises(ValueError, match='float32 or bfloat16'):
        pair_loss(z.double(), ids, ids, ids)
    with pytest.raises(ValueError, match='int64'):
        pair_loss(z, ids.int(), ids, ids)
    with pytest.raises(ValueError, match='positives'):
        pair_loss(z, ids, ids[:3], ids)
