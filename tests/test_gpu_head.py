"""The fused classifier head and GraphSAINT-weighted NLL loss (csrc/head.hip behind ampnet_amd/head.py) on the GPU against
the numpy fp64 model of tests/head_reference.py, against torch autograd, against the reference's fixtures, and inside the
whole model.

Shapes (N, D, C): (1, 3, 2) a single row; (64, 3, 2) the XOR model, element-wise path; (257, 100, 7) the class defaults,
ragged rows and a ragged last tile; (48, 128, 7) the Cora fixture; (33, 128, 1) one class: the log-probabilities are
exactly 0; (20011, 256, 64) many workgroups: the cross-workgroup reduction, the class limit and W read from global memory;
(0, 128, 7) empty.  fp32 everywhere, bf16 pooled where D % 8 == 0.  Row passes, class chunks, the home of W and the rows
per tile beyond these shapes are on the ladders of tests/test_gpu_head_kernels.py.
Tolerances: the project's flat atol 1e-5, rtol 1e-4 on log-probabilities and fp32 dpooled; the scaled bar (labels gW, gb)
on dW and db; bf16 dpooled atol = rtol = 2e-2 (tests/test_gpu_glue.py); counts exact."""
import functools
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_reference as ref
from conftest import assert_close_scaled, load_golden, model_files
from head_reference import make_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 2), (64, 3, 2), (257, 100, 7), (48, 128, 7), (33, 128, 1), (20011, 256, 64), (0, 128, 7)]
BIG = (20011, 256, 64)
CASES = [(s, 'f32') for s in SHAPES] + [(s, 'bf16') for s in SHAPES if s[1] % 8 == 0]
CASE_IDS = [f'N{s[0]}_D{s[1]}_C{s[2]}_{d}' for s, d in CASES]
BF16 = dict(atol=2e-2, rtol=2e-2)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _np(t):
    return t.detach().float().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _inputs(shape, dtype):
    """(pooled rounded to the storage dtype, W, b, y with two ignored labels, node weights, two overlapping masks, dout):
    CPU tensors shared by the tests of a case, never modified."""
    N, D, C = shape
    pooled, W, b, y, w, masks = make_inputs(N, D, C)
    if dtype == 'bf16':
        pooled = pooled.to(torch.bfloat16)
    if N > 8:
        y = y.clone()
        y[3], y[5] = -100, -100
    dout = torch.randn(N, C, generator=torch.Generator().manual_seed(7))
    return pooled, W, b, y, w, masks, dout


@functools.lru_cache(maxsize=None)
def _reference(shape, dtype):
    """The fp64 model on the stored values of a case: computed once, shared."""
    pooled, W, b, y, w, masks, dout = _inputs(shape, dtype)
    p, Wn, bn, yn, wn, mn = _np(pooled), W.numpy(), b.numpy(), y.numpy(), w.numpy(), masks.numpy()
    out = {k: ref.head_fwd(p, Wn, bn, k) for k in ('log_softmax', 'sigmoid')}
    return {'out': out, 'bwd': {k: ref.head_bwd(p, Wn, dout.numpy(), out[k], k) for k in out},
            'nll': ref.nll_fwd(p, Wn, bn, yn, wn, mn),
            'nll_bwd': [ref.nll_bwd(p, Wn, bn, yn, wn, mn, m, 1.0) for m in range(2)]}


def _leaves(dev, *tensors):
    return [t.to(dev).requires_grad_(True) for t in tensors]


def _check_grads(got, want, dtype, what):
    dp, dW, db = got
    assert_close_scaled(_np(dp), want[0], f'dpooled {what}', **(BF16 if dtype == 'bf16' else {}))
    assert_close_scaled(_np(dW), want[1], f'gW {what}')
    assert_close_scaled(_np(db), want[2], f'gb {what}')


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_classifier_head_matches_the_reference_model(case, dev):
    from ampnet_amd import classifier_head
    shape, dtype = case
    pooled, W, b, _, _, _, dout = _inputs(shape, dtype)
    want = _reference(shape, dtype)
    for kind in ('log_softmax', 'sigmoid'):
        p, Wt, bt = _leaves(dev, pooled, W, b)
        out = classifier_head(p, Wt, bt, kind)
        assert out.dtype == torch.float32 and out.shape == (shape[0], shape[2])
        out.backward(dout.to(dev))
        assert p.grad.dtype == pooled.dtype
        assert_close_scaled(_np(out), want['out'][kind], f'out {kind}')
        _check_grads((p.grad, Wt.grad, bt.grad), want['bwd'][kind], dtype, kind)
        if shape[2] == 1 and kind == 'log_softmax':
            assert bool((out == 0).all())                         # one class: log-probability exactly 0
        if dtype == 'f32':                                        # torch's own composite on the GPU
            q, Wq, bq = _leaves(dev, pooled, W, b)
            z = F.linear(q, Wq, bq)
            tout = F.log_softmax(z, dim=1) if kind == 'log_softmax' else torch.sigmoid(z)
            tout.backward(dout.to(dev))
            assert_close_scaled(_np(out), _np(tout), f'out {kind} against torch')
            assert_close_scaled(_np(p.grad), _np(q.grad), f'dpooled {kind} against torch')
            assert_close_scaled(_np(Wt.grad), _np(Wq.grad), f'gW {kind} against torch')
            assert_close_scaled(_np(bt.grad), _np(bq.grad), f'gb {kind} against torch')


@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_saint_nll_loss_matches_the_reference_model(case, dev):
    from ampnet_amd import HeadMetrics, saint_nll_loss
    shape, dtype = case
    N = shape[0]
    pooled, W, b, y, w, masks, _ = _inputs(shape, dtype)
    want = _reference(shape, dtype)
    yd, wd, md = y.to(dev), w.to(dev), masks.to(dev)
    grads = []
    for gm in range(2):
        p, Wt, bt = _leaves(dev, pooled, W, b)
        metrics = HeadMetrics(2, dev)
        loss, logp = saint_nll_loss(p, Wt, bt, yd, wd, md, grad_mask=gm, metrics=metrics, return_log_probs=True)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
        loss.backward()
        got = metrics.read()
        # the loss and loss_sum are sums over N rows: scaled like the parameter gradients
        assert_close_scaled(loss.item(), want['nll']['loss_sum'][gm], f'loss of mask {gm}', scaled=True)
        assert_close_scaled(got['loss_sum'], want['nll']['loss_sum'], 'loss_sum', scaled=True)
        assert got['count'] == want['nll']['count'] and got['correct'] == want['nll']['correct']
        assert got['bad_labels'] == 0
        assert_close_scaled(_np(logp), want['nll']['logp'], 'log-probs')
        _check_grads((p.grad, Wt.grad, bt.grad), want['nll_bwd'][gm], dtype, f'mask {gm}')
        unselected = ~(masks[gm] & (y != -100))
        rows = p.grad[unselected.to(dev)]                         # rows outside the gradient mask: bit-zero
        assert bool((rows.view(torch.int16 if dtype == 'bf16' else torch.int32) == 0).all())
        grads.append(p.grad)
    # flipping grad_mask flips where the gradient comes from, wherever the reference model's two gradients differ: with one
    # class softmax - onehot is exactly 0, so both are all-zero there, and a single row has one selection to offer
    if not np.array_equal(want['nll_bwd'][0][0], want['nll_bwd'][1][0]):
        assert not torch.equal(grads[0], grads[1])
    assert shape[2] == 1 or N <= 8 or not torch.equal(grads[0], grads[1])
    # the second mask's metrics are what the first's would be with the masks swapped
    swapped = HeadMetrics(2, dev)
    saint_nll_loss(pooled.to(dev), W.to(dev), b.to(dev), yd, wd, (md[1], md[0]) if N else md.flip(0), metrics=swapped)
    a, s = metrics.read(), swapped.read()
    for key in ('loss_sum', 'count', 'correct'):
        assert a[key] == s[key][::-1], key


def test_node_norm_and_masks_are_optional(dev):
    from ampnet_amd import HeadMetrics, saint_nll_loss
    shape = (257, 100, 7)
    pooled, W, b, y, _, masks, _ = _inputs(shape, 'f32')
    metrics = HeadMetrics(1, dev)
    p, Wt, bt = _leaves(dev, pooled, W, b)
    loss = saint_nll_loss(p, Wt, bt, y.to(dev), metrics=metrics)
    loss.backward()
    want = ref.nll_fwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy())
    assert_close_scaled(loss.item(), want['loss_sum'][0], 'unweighted loss', scaled=True)      # a sum over N rows
    assert metrics.read()['count'] == [shape[0] - 2]             # two labels are -100
    _check_grads((p.grad, Wt.grad, bt.grad), ref.nll_bwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy()), 'f32', 'all nodes')
    single = saint_nll_loss(pooled.to(dev), W.to(dev), b.to(dev), y.to(dev), masks=masks[0].to(dev).to(torch.uint8))
    want1 = ref.nll_fwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy(), None, masks[0].numpy())
    assert_close_scaled(single.item(), want1['loss_sum'][0], 'loss of a [N] uint8 mask', scaled=True)      # a sum over N rows


def test_strided_and_unaligned_pooled_views(dev):
    """A row-strided view (read in place, 16-byte pieces) and a view whose base is 4 bytes off 16-byte alignment (the
    element-wise kernels) give what the contiguous tensor gives."""
    from ampnet_amd import classifier_head, saint_nll_loss
    shape = (48, 128, 7)
    N, D, C = shape
    pooled, W, b, y, w, masks, dout = _inputs(shape, 'f32')
    want = _reference(shape, 'f32')
    wide = torch.zeros(N, D + 32, device=dev)
    strided = wide[:, :D].copy_(pooled.to(dev))
    assert strided.stride(0) == D + 32 and strided.data_ptr() % 16 == 0
    buf = torch.zeros(N * D + 1, device=dev)
    shifted = buf[1:].view(N, D).copy_(pooled.to(dev))
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for view, what in ((strided, 'strided'), (shifted, 'unaligned')):
        p = view.detach().requires_grad_(True)
        Wt, bt = _leaves(dev, W, b)
        out = classifier_head(p, Wt, bt)
        out.backward(dout.to(dev))
        assert_close_scaled(_np(out), want['out']['log_softmax'], f'out {what}')
        _check_grads((p.grad, Wt.grad, bt.grad), want['bwd']['log_softmax'], 'f32', what)
        p = view.detach().requires_grad_(True)
        Wt, bt = _leaves(dev, W, b)
        loss = saint_nll_loss(p, Wt, bt, y.to(dev), w.to(dev), masks.to(dev))
        loss.backward()
        assert_close_scaled(loss.item(), want['nll']['loss_sum'][0], f'loss {what}', scaled=True)      # a sum over N rows
        _check_grads((p.grad, Wt.grad, bt.grad), want['nll_bwd'][0], 'f32', f'loss {what}')


def test_edge_conditions(dev):
    from ampnet_amd import HeadMetrics, saint_nll_loss
    shape = (257, 100, 7)
    N, D, C = shape
    pooled, W, b, y, w, masks, _ = _inputs(shape, 'f32')

    def run(y, masks, scale=1.0, gm=0):
        p, Wt, bt = _leaves(dev, pooled, W, b)
        metrics = HeadMetrics(2, dev)
        loss, logp = saint_nll_loss(p, Wt, bt, y.to(dev), w.to(dev), masks.to(dev), gm, metrics, return_log_probs=True)
        (scale * loss).backward()
        return loss.detach(), logp, (p.grad, Wt.grad, bt.grad), metrics.read()

    # an all-false gradient mask: loss exactly 0, gradients exactly 0, nothing is NaN
    none = torch.stack([torch.zeros(N, dtype=torch.bool), masks[1]])
    loss, logp, grads, got = run(y, none)
    assert loss.item() == 0.0 and got['loss_sum'][0] == 0.0 and got['count'][0] == 0 and got['count'][1] > 0
    for t in grads:
        assert bool((t == 0).all()) and bool(torch.isfinite(t).all())
    assert bool(torch.isfinite(logp).all())

    # -100 is skipped: the two ignored rows count nowhere (the counts are those of the reference model)
    base_loss, base_logp, base_grads, base = run(y, masks)
    want = ref.nll_fwd(pooled.numpy(), W.numpy(), b.numpy(), y.numpy(), w.numpy(), masks.numpy())
    assert base['count'] == want['count'] and base['bad_labels'] == 0
    assert base['count'][0] == int((masks[0] & (y != -100)).sum())

    # a label equal to C and a negative one: skipped and counted; nothing else changes against masking those rows out
    rows = [i for i in range(N) if masks[0][i] and masks[1][i] and y[i] >= 0][:2]
    bad_y = y.clone()
    bad_y[rows[0]], bad_y[rows[1]] = C, -3
    out_masks = masks.clone()
    out_masks[:, rows] = False
    bl, blogp, bgrads, bgot = run(bad_y, masks)
    ml, mlogp, mgrads, mgot = run(y, out_masks)
    assert bgot['bad_labels'] == 2 and mgot['bad_labels'] == 0
    assert torch.equal(bl, ml) and torch.equal(blogp, mlogp)
    for a, c in zip(bgrads, mgrads):
        assert torch.equal(a, c)
    for key in ('loss_sum', 'count', 'correct'):
        assert bgot[key] == mgot[key], key

    # an upstream gradient other than 1 scales the gradients
    _, _, grads3, _ = run(y, masks, scale=3.0)
    for a, c, label in zip(grads3, base_grads, ('dpooled', 'gW', 'gb')):
        assert_close_scaled(_np(a), 3.0 * _np(c).astype(np.float64), f'{label} under 3 * loss')


def test_argmax_ties_go_to_the_lowest_class(dev):
    from ampnet_amd import HeadMetrics, saint_nll_loss
    N, D, C = 16, 8, 5
    pooled = torch.zeros(N, D, device=dev)                       # all logits equal the (equal) biases
    W = torch.randn(C, D, device=dev)
    b = torch.full((C,), 0.25, device=dev)
    y = torch.arange(N, device=dev) % C
    metrics = HeadMetrics(1, dev)
    saint_nll_loss(pooled, W, b, y, metrics=metrics)
    got = metrics.read()
    assert got['count'] == [N] and got['correct'] == [int((y == 0).sum())]


def test_bitwise_reproducible_and_accumulating(dev):
    from ampnet_amd import HeadMetrics, saint_nll_loss
    pooled, W, b, y, w, masks, _ = _inputs(BIG, 'f32')
    yd, wd, md = y.to(dev), w.to(dev), masks.to(dev)

    def run(metrics):
        p, Wt, bt = _leaves(dev, pooled, W, b)
        loss = saint_nll_loss(p, Wt, bt, yd, wd, md, metrics=metrics)
        loss.backward()
        return loss.detach(), p.grad, Wt.grad, bt.grad

    m1, m2 = HeadMetrics(2, dev), HeadMetrics(2, dev)
    first, second = run(m1), run(m2)
    for a, c, label in zip(first, second, ('loss', 'dpooled', 'dW', 'db')):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), label
    assert torch.equal(m1.buffer, m2.buffer)
    once = m1.read()
    run(m1)                                                      # no zero_(): the buffer accumulates
    twice = m1.read()
    assert twice['count'] == [2 * c for c in once['count']] and twice['correct'] == [2 * c for c in once['correct']]
    # loss_sum is a sum over N rows: scaled
    assert_close_scaled(twice['loss_sum'], [2 * v for v in once['loss_sum']], 'loss_sum after two calls', scaled=True)
    assert m1.zero_().read()['count'] == [0, 0]


# ---- the reference's fixtures ----------------------------------------------------------------------------------------
def _cfg_value(v):
    if v in ('True', 'False'):
        return v == 'True'
    if v == 'None':
        return None
    try:
        return int(v)
    except ValueError:
        return float(v)


def _cfg(g):
    return {k: _cfg_value(v) for k, v in zip(g['cfg_keys'].tolist(), g['cfg_vals'].tolist())}


def _load_model(g, dev, **override):
    from ampnet_amd import AMPGCN
    model = AMPGCN(device=dev, **{**_cfg(g), **override}).to(dev)
    model.load_state_dict({k[len('param.'):]: torch.from_numpy(v) for k, v in g.items() if k.startswith('param.')})
    model.train()
    data = types.SimpleNamespace(x=torch.from_numpy(g['x']).to(dev), edge_index=torch.from_numpy(g['edge_index']).to(dev))
    idx = g.get('sampled_node_feat_indices')
    return model, data, None if idx is None else torch.from_numpy(idx).to(dev)


MODEL_IDS = [os.path.basename(p)[:-4] for p in model_files()]


@pytest.mark.parametrize('path', model_files(), ids=MODEL_IDS)
def test_head_matches_reference_fixture(path, dev):
    """relu -> pooling of the fixture's conv2_embedding -> classifier_head with the fixture's final_linear_out, against the
    fixture's logits and parameter gradients (labels and tolerances of test_fused_model_matches_reference_fixture)."""
    from ampnet_amd import classifier_head
    g = load_golden(path)
    cfg = _cfg(g)
    D = cfg['embedding_dim']
    h = F.relu(torch.from_numpy(g['conv2_embedding']).to(dev))
    h = h.reshape(h.shape[0], -1, D)
    pooled = (h.mean(dim=1) if cfg['average_pooling_flag'] else h[:, 0]).contiguous()
    W, b = _leaves(dev, torch.from_numpy(g['param.final_linear_out.weight']), torch.from_numpy(g['param.final_linear_out.bias']))
    logits = classifier_head(pooled, W, b, 'log_softmax' if cfg['softmax_out'] else 'sigmoid')
    (logits * torch.from_numpy(g['dlogits']).to(dev)).sum().backward()
    assert_close_scaled(_np(logits), g['logits'], 'logits')
    assert_close_scaled(_np(W.grad), g['grad.final_linear_out.weight'], 'grad.final_linear_out.weight.grad')
    assert_close_scaled(_np(b.grad), g['grad.final_linear_out.bias'], 'grad.final_linear_out.bias.grad')


@pytest.mark.parametrize('path', model_files(), ids=MODEL_IDS)
def test_fused_head_model_matches_reference_fixture(path, dev):
    g = load_golden(path)
    model, data, idx = _load_model(g, dev, fused_head=True)
    assert model.fused_head
    logits = model(data, feature_indices=idx)
    (logits * torch.from_numpy(g['dlogits']).to(dev)).sum().backward()
    assert_close_scaled(_np(logits), g['logits'], 'logits')
    assert_close_scaled(_np(model.conv1_embedding), g['conv1_embedding'], 'conv1_embedding')
    assert_close_scaled(_np(model.conv2_embedding), g['conv2_embedding'], 'conv2_embedding')
    for name, p in model.named_parameters():
        key = 'grad.' + name
        if key in g:
            assert_close_scaled(_np(p.grad), g[key], key + '.grad')
        else:
            assert p.grad is None, name


@pytest.mark.parametrize('fused_glue', [False, True], ids=['plain_glue', 'fused_glue'])
def test_model_nll_loss_matches_the_unfused_twin(fused_glue, dev):
    """model.nll_loss(...) against the reference's loss formula on model(data) of a fused_head=False twin with the same
    state dict and feature indices: the loss and every parameter gradient."""
    from ampnet_amd import HeadMetrics
    g = load_golden([p for p in model_files() if p.endswith('model_cora.npz')][0])
    fused, data, idx = _load_model(g, dev, fused_head=True, fused_glue=fused_glue)
    twin, _, _ = _load_model(g, dev, fused_glue=fused_glue)
    assert list(fused.state_dict().keys()) == list(twin.state_dict().keys())
    N = data.x.size(0)
    gen = torch.Generator().manual_seed(3)
    data.y = torch.randint(0, 7, (N,), generator=gen).to(dev)
    data.node_norm = (torch.rand(N, generator=gen) * 2 + 0.1).to(dev)
    train = (torch.rand(N, generator=gen) < 0.6).to(dev)
    test = ~train
    metrics = HeadMetrics(2, dev)
    loss = fused.nll_loss(data, masks=(train, test), metrics=metrics, feature_indices=idx)
    loss.backward()
    out = twin(data, feature_indices=idx)
    want = (F.nll_loss(out, data.y, reduction='none') * data.node_norm)[train].sum()
    want.backward()
    assert_close_scaled(loss.item(), want.item(), 'loss', scaled=True)             # a sum over N rows
    assert_close_scaled(_np(fused.conv2_embedding), _np(twin.conv2_embedding), 'conv2_embedding')
    assert torch.equal(fused.sampled_node_feat_indices, twin.sampled_node_feat_indices)
    got = metrics.read()
    assert got['count'] == [int(train.sum()), int(test.sum())]
    assert got['correct'] == [int((out.argmax(1) == data.y)[train].sum()), int((out.argmax(1) == data.y)[test].sum())]
    test_loss = (F.nll_loss(out, data.y, reduction='none') * data.node_norm)[test].sum()
    assert_close_scaled(got['loss_sum'][1], test_loss.item(), 'test-mask loss_sum', scaled=True)      # a sum over N rows
    for (name, p), (_, q) in zip(fused.named_parameters(), twin.named_parameters()):
        if q.grad is None:
            assert p.grad is None, name
        else:
            assert_close_scaled(_np(p.grad), _np(q.grad), f'{name}.grad')


def test_no_device_synchronisation(dev):
    from ampnet_amd import HeadMetrics, saint_nll_loss
    pooled, W, b, y, w, masks, _ = _inputs((257, 100, 7), 'f32')
    p, Wt, bt = _leaves(dev, pooled, W, b)
    yd, wd, m0, m1 = y.to(dev), w.to(dev), masks[0].to(dev), masks[1].to(dev)
    metrics = HeadMetrics(2, dev)
    saint_nll_loss(p, Wt, bt, yd, wd, (m0, m1), metrics=metrics).backward()      # warm up: library load, allocator
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        loss = saint_nll_loss(p, Wt, bt, yd, wd, (m0, m1), metrics=metrics)
        (3 * loss).backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert metrics.read()['count'][0] == 2 * int((masks[0] & (y != -100)).sum())


def test_bad_arguments_raise(dev):
    from ampnet_amd import HeadMetrics, _lib, classifier_head, saint_nll_loss
    N, D = 16, 8
    pooled, y = torch.randn(N, D, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
    W, b = torch.randn(7, D, device=dev), torch.randn(7, device=dev)
    mask = torch.ones(N, dtype=torch.bool, device=dev)
    with pytest.raises(ValueError, match='64'):
        classifier_head(pooled, torch.randn(65, D, device=dev), torch.randn(65, device=dev))
    with pytest.raises(ValueError, match='float32'):
        classifier_head(pooled, W.bfloat16(), b)
    with pytest.raises(ValueError, match='no CPU fallback'):
        saint_nll_loss(pooled.cpu(), W, b, y)
    with pytest.raises(ValueError, match='N = 16'):
        saint_nll_loss(pooled, W, b, y, masks=mask[:-1])
    with pytest.raises(ValueError, match='1 to 4'):
        saint_nll_loss(pooled, W, b, y, masks=(mask,) * 5)
    with pytest.raises(ValueError, match='grad_mask'):
        saint_nll_loss(pooled, W, b, y, masks=(mask, mask), grad_mask=2)
    with pytest.raises(ValueError, match='metrics'):
        saint_nll_loss(pooled, W, b, y, masks=(mask, mask), metrics=HeadMetrics(1, dev))
    with pytest.raises(ValueError, match='output'):
        classifier_head(pooled, W, b, 'softmax')
    # the library itself: error codes, nothing launched
    lib = _lib.load()
    out, scratch = torch.empty(N, 65, device=dev), torch.zeros(13, dtype=torch.int64, device=dev)
    loss = torch.zeros((), device=dev)
    args = (pooled.data_ptr(), N, D, D, W.data_ptr(), b.data_ptr())
    assert lib.ampconv_head_fwd(*args, 65, 0, out.data_ptr(), 0, None) == -1                       # C > 64
    assert lib.ampconv_head_fwd(*args, 0, 0, out.data_ptr(), 0, None) == -1                        # C < 1
    assert lib.ampconv_head_fwd(*args, 7, 2, out.data_ptr(), 0, None) == -1                        # kind
    assert lib.ampconv_head_fwd(*args, 7, 0, out.data_ptr(), 7, None) == -2                        # dtype
    assert lib.ampconv_head_fwd(pooled.data_ptr(), -1, D, D, W.data_ptr(), b.data_ptr(), 7, 0, out.data_ptr(), 0, None) == -1
    nll = (7, y.data_ptr(), None, None)
    tail = (None, None, scratch.data_ptr(), loss.data_ptr(), 0, None)
    assert lib.ampconv_head_nll_fwd(*args, *nll, 5, 0, *tail) == -1                                # M > 4
    assert lib.ampconv_head_nll_fwd(*args, *nll, 2, 2, *tail) == -1                                # grad_mask >= M
    assert lib.ampconv_head_nll_fwd(None, 0, D, D, W.data_ptr(), b.data_ptr(), *nll, 1, 0, *tail) == 0          # N = 0
    dW, db = torch.empty_like(W), torch.empty_like(b)
    assert lib.ampconv_head_bwd(pooled.data_ptr(), N, D, D, W.data_ptr(), 7, 0, out.data_ptr(), out.data_ptr(), None,
                                dW.data_ptr(), db.data_ptr(), scratch.data_ptr(), 8, 0, None) == -3                 # workspace
    torch.cuda.synchronize()
    assert loss.item() == 0.0
