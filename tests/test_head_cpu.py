"""CPU checks of the fused classifier head (ampnet_amd/head.py, csrc/head.hip): the numpy model of tests/head_reference.py
agrees with torch's CPU composite and its autograd (the GPU kernels are then held to that model, tests/test_gpu_head.py),
the new entry points are declared and bound, and the package exports the new names."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_reference as ref
from head_reference import make_inputs
from conftest import ROOT, assert_close_scaled

HEADER = os.path.join(ROOT, 'include', 'ampconv.h')
ENTRY_POINTS = ['ampconv_head_workspace_bytes', 'ampconv_head_fwd', 'ampconv_head_bwd', 'ampconv_head_nll_fwd',
                'ampconv_head_nll_bwd']


def torch_composite(pooled, W, b, y, w, mask):
    """The reference's loss and accuracy counts with plain PyTorch ops (labels outside [0, C) have to be masked out)."""
    out = F.log_softmax(F.linear(pooled, W, b), dim=1)
    keep = mask & (y != -100)
    loss = (F.nll_loss(out, y, reduction='none') * w)[keep].sum()
    return out, loss, int(keep.sum()), int((out.argmax(1) == y)[keep].sum())


@pytest.mark.parametrize('shape', [(1, 3, 2), (64, 3, 2), (257, 100, 7), (48, 128, 7), (33, 128, 1), (0, 128, 7)])
def test_reference_model_matches_torch_cpu(shape):
    N, D, C = shape
    pooled, W, b, y, w, masks = make_inputs(N, D, C)
    if N > 8:
        y[3], y[5] = -100, -100                                 # ignored labels
        masks[1, :] = False                                     # an all-false mask
        pooled[7] = 0.0                                         # argmax ties: equal logits in classes of equal bias
        b = b.clone()
        b[:] = b[0]
    for dtype in (torch.float64, torch.float32):                # fp32: the composite the GPU tests also compare with
        p, Wt, bt = (t.to(dtype).clone().requires_grad_(True) for t in (pooled, W, b))
        got = ref.nll_fwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy(), w.numpy(), masks.numpy())
        for m in range(2):
            out, loss, count, correct = torch_composite(p, Wt, bt, y, w.to(dtype), masks[m])
            # loss sums: sums over N rows, scaled like the parameter gradients
            assert_close_scaled(got['loss_sum'][m], loss.item(), f'loss mask {m}', scaled=True)
            assert got['count'][m] == count and got['correct'][m] == correct
            assert_close_scaled(got['logp'], out.detach().numpy(), 'log-probs')
            p.grad = Wt.grad = bt.grad = None
            (3 * loss).backward()
            dp, dW, db = ref.nll_bwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy(), w.numpy(), masks.numpy(), m, 3.0)
            assert_close_scaled(dp, p.grad.numpy(), 'dpooled')
            assert_close_scaled(dW, Wt.grad.numpy(), 'gW')
            assert_close_scaled(db, bt.grad.numpy(), 'gb')
        assert got['bad_labels'] == 0
    if N > 8:
        assert got['loss_sum'][1] == 0.0 and got['count'][1] == 0
        assert int(np.argmax(got['logp'][7])) == 0               # the tie goes to the lowest class


@pytest.mark.parametrize('kind', ['log_softmax', 'sigmoid'])
def test_reference_head_matches_torch_autograd(kind):
    pooled, W, b, *_ = make_inputs(257, 100, 7)
    dout = torch.randn(257, 7, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    p, Wt, bt = (t.double().requires_grad_(True) for t in (pooled, W, b))
    z = F.linear(p, Wt, bt)
    out = F.log_softmax(z, dim=1) if kind == 'log_softmax' else torch.sigmoid(z)
    out.backward(dout)
    got = ref.head_fwd(pooled.numpy(), W.numpy(), b.numpy(), kind)
    assert_close_scaled(got, out.detach().numpy(), 'out')
    dp, dW, db = ref.head_bwd(pooled.numpy(), W.numpy(), dout.numpy(), got, kind)
    assert_close_scaled(dp, p.grad.numpy(), 'dpooled')
    assert_close_scaled(dW, Wt.grad.numpy(), 'gW')
    assert_close_scaled(db, bt.grad.numpy(), 'gb')


def test_reference_bad_labels_are_skipped_and_counted():
    pooled, W, b, y, w, masks = make_inputs(48, 128, 7)
    y2 = y.clone()
    y2[4], y2[9] = 7, -3
    masks[:, 4] = True
    masks[:, 9] = True
    got = ref.nll_fwd(pooled.numpy(), W.numpy(), b.numpy(), y2.numpy(), w.numpy(), masks.numpy())
    out = masks.clone()
    out[:, 4] = False
    out[:, 9] = False
    want = ref.nll_fwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy(), w.numpy(), out.numpy())
    assert got['bad_labels'] == 2 and want['bad_labels'] == 0
    assert got['loss_sum'] == want['loss_sum'] and got['count'] == want['count'] and got['correct'] == want['correct']


def test_entry_points_are_declared_and_bound():
    from ampnet_amd import _lib
    header = open(HEADER).read()
    for name in ENTRY_POINTS:
        assert re.search(r'\b' + name + r'\s*\(', header), f'{name} is not declared in include/ampconv.h'
        assert name in _lib.SIGNATURES, f'{name} is missing from _lib.SIGNATURES'
        declared = re.search(r'\b' + name + r'\s*\(([^;]*)\)\s*;', header).group(1)
        assert len(declared.split(',')) == len(_lib.SIGNATURES[name][1]), name      # one ctypes type per C parameter
    version = int(re.search(r'#define\s+AMPCONV_VERSION\s+(\d+)', header).group(1))
    assert version == _lib.EXPECTED_ABI


def test_package_exports_the_head():
    import ampnet_amd
    from ampnet_amd import AMPGCN
    for name in ('classifier_head', 'saint_nll_loss', 'HeadMetrics'):
        assert hasattr(ampnet_amd, name) and name in ampnet_amd.__all__
    assert 'fused_head' in inspect.signature(AMPGCN.__init__).parameters
    assert inspect.signature(AMPGCN.__init__).parameters['fused_head'].default is False
    assert callable(getattr(AMPGCN, 'nll_loss', None))


def test_fused_head_keeps_the_state_dict_keys_and_refuses_what_it_cannot_run():
    from ampnet_amd import AMPGCN, HeadMetrics, classifier_head, saint_nll_loss
    kw = dict(device='cpu', embedding_dim=8, num_heads=2, num_node_features=11, num_sampled_vectors=3, feat_emb_dim=7,
              val_emb_dim=1)
    torch.manual_seed(0)
    plain = AMPGCN(output_dim=2, **kw)
    torch.manual_seed(0)
    fused = AMPGCN(output_dim=2, fused_head=True, **kw)
    assert list(plain.state_dict().keys()) == list(fused.state_dict().keys())
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in fused.named_modules()]
    assert fused.fused_head and not plain.fused_head and not fused.fused_glue
    with pytest.raises(ValueError, match='output_dim'):
        AMPGCN(output_dim=65, fused_head=True, **kw)
    AMPGCN(output_dim=65, **kw)                                  # the unfused model has no such limit
    x, W, b = torch.randn(4, 8), torch.randn(2, 8), torch.randn(2)
    with pytest.raises(ValueError, match='no CPU fallback'):
        classifier_head(x, W, b)
    with pytest.raises(ValueError, match='no CPU fallback'):
        saint_nll_loss(x, W, b, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError):
        HeadMetrics(5)
    with pytest.raises(ValueError, match='no CPU fallback'):
        HeadMetrics(2, device='cpu')
