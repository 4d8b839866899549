"""The fused pair loss on the GPU (csrc/pair_loss.hip) against the fp64 model of tests/pair_loss_reference.py: through the
public function, and through ctypes for the row terms and the refusals."""
import types

import numpy as np
import pytest
import torch

import pair_loss_reference as ref
from conftest import assert_close_scaled

pytestmark = pytest.mark.gpu

KINDS = ('skipgram', 'xent')
BF16_TOL = dict(atol=2e-2, rtol=2e-2)                 # the bf16 bar of tests/test_gpu_glue.py


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _stored(z, dtype):
    """(the tensor as stored, its values in fp64): the model runs on the stored values."""
    t = torch.from_numpy(z).to(dtype)
    return t, t.double().numpy()


def _c_forward(zt, anchor, positive, negative, weight, kind, scale=1.0, neg_weight=1.0, exclude=False, ldz=None,
               null_anchor=False, ws_bytes=None):
    """ampconv_pair_loss_fwd through ctypes, every output pre-filled with 7: (return code, aff, neg_term, loss, oob)."""
    from ampnet_amd import _lib
    lib = _lib.load()
    N, D = zt.shape
    B, S = anchor.numel(), negative.numel()
    dev = zt.device
    aff = torch.full((B,), 7.0, device=dev)
    neg = torch.full((B,), 7.0, device=dev)
    loss = torch.full((), 7.0, device=dev)
    oob = torch.full((1,), 7, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.ampconv_pair_loss_workspace_bytes(B, S, min(D, 256))), 256), dtype=torch.uint8, device=dev)
    rc = lib.ampconv_pair_loss_fwd(zt.data_ptr(), N, D, zt.stride(0) if ldz is None else ldz,
                                   None if null_anchor else anchor.data_ptr(),
                                   positive.data_ptr(), B, negative.data_ptr(), S, _lib.ptr(weight), ref_kind(kind), scale,
                                   neg_weight, int(exclude), aff.data_ptr(), neg.data_ptr(), loss.data_ptr(), oob.data_ptr(),
                                   ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, _lib.DTYPES[zt.dtype],
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, aff.cpu().numpy(), neg.cpu().numpy(), float(loss), int(oob)


def ref_kind(kind):
    return {'skipgram': 0, 'xent': 1}[kind]


def _check(dev, N, D, B, S, dtype, kind, amp=1.0, scaled_rows=False, seed=0, **opts):
    """One case: row terms through ctypes, loss and dz through the public function, all against the fp64 model."""
    from ampnet_amd import pair_loss
    z, anchor, positive, negative, weight = ref.make_inputs(N, D, B, S, amp=amp, seed=seed)
    zt, z64 = _stored(z, dtype)
    zt = zt.to(dev).requires_grad_(True)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    want_loss, want_aff, want_neg, _, _ = ref.forward(z64, anchor, positive, negative, weight, kind, **opts)
    want_dz = ref.backward(z64, anchor, positive, negative, weight, kind, **opts)
    tag = f'{kind} {str(dtype)[6:]} N{N} D{D} B{B} S{S}'

    loss = pair_loss(zt, a, p, n, kind=kind, weight=w, **opts)
    loss.backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and zt.grad.dtype == dtype and zt.grad.shape == zt.shape
    dz = zt.grad.double().cpu().numpy()
    assert np.isfinite(dz).all() and np.isfinite(loss.item())
    assert_close_scaled(loss.item(), want_loss, f'{tag}: loss', scaled=True)          # a sum over the B pairs
    if B > 0:
        rc, aff, neg, c_loss, oob = _c_forward(zt.detach(), a, p, n, w, kind, opts.get('scale', 1.0),
                                               opts.get('neg_weight', 1.0), opts.get('exclude_anchor', False))
        assert rc == 0 and oob == 0 and c_loss == loss.item()
        assert np.isfinite(aff).all() and np.isfinite(neg).all()
        # bf16 storage holds the same flat bar: the products of the stored values are exact in fp32
        assert_close_scaled(aff, want_aff, f'{tag}: aff', scaled=scaled_rows)
        assert_close_scaled(neg, want_neg, f'{tag}: neg_term', scaled=scaled_rows)
    if dtype == torch.float32:
        assert_close_scaled(dz, want_dz, f'{tag}: dz', scaled=scaled_rows)
    else:
        assert not scaled_rows
        assert_close_scaled(dz, want_dz, f'{tag}: dz', scaled=False, **BF16_TOL)


LADDER = ([(300, 100, B, 33) for B in (1, 15, 16, 17, 33, 257)] +
          [(300, 100, 33, S) for S in (1, 15, 16, 17, 31, 33, 300)] +
          [(300, D, 33, 33) for D in (1, 3, 4, 31, 32, 33, 100, 128, 256)])
COMBINED = [(300, 100, 17, 5000),        # the split-S merge
            (300, 100, 4000, 20),        # the GraphSAGE shape
            (600, 128, 1000, 500),
            (300, 100, 0, 33)]           # B = 0


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', LADDER + COMBINED, ids=lambda s: 'N%d_D%d_B%d_S%d' % s)
def test_against_the_fp64_model(dev, shape, kind):
    N, D, B, S = shape
    _check(dev, N, D, B, S, torch.float32, kind)
    if D % 8 == 0:
        _check(dev, N, D, B, S, torch.bfloat16, kind)


@pytest.mark.parametrize('kind', KINDS)
def test_large_logits(dev, kind):
    # amp = 4: logits to +-250.  A fp32 torch composite of the same inputs exceeds the flat bar itself by 1.1-2.3x here
    # (rounding of a logit of magnitude 250 is 1.5e-5 already) and uses 0.13 of the scaled one: row terms and dz are held
    # to scaled=True in this case only.  Everything has to be finite.
    _check(dev, 300, 100, 257, 33, torch.float32, kind, amp=4.0, scaled_rows=True)


@pytest.mark.parametrize('kind', KINDS)
def test_options(dev, kind):
    from ampnet_amd import PairLoss
    _check(dev, 300, 100, 33, 40, torch.float32, kind, seed=4, scale=0.5, neg_weight=0.7)
    z, anchor, positive, negative, _ = ref.make_inputs(200, 24, 50, 30, seed=5)
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    a, p, n = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative))
    loss = PairLoss(kind=kind, scale=2.0, reduction='mean')(zt, a, p, n)              # no weights, the mean over B
    loss.backward()
    want = ref.forward(z, anchor, positive, negative, None, kind, scale=2.0)[0] / 50
    want_dz = ref.backward(z, anchor, positive, negative, None, kind, scale=2.0, g0=1 / 50)
    assert_close_scaled(loss.item(), want, f'{kind}: mean loss', scaled=True)
    assert_close_scaled(zt.grad.cpu().numpy(), want_dz, f'{kind}: dz of the mean', scaled=False)


@pytest.mark.parametrize('kind', KINDS)
def test_duplicates_and_shared_roles(dev, kind):
    from ampnet_amd import pair_loss
    N, D, B, S = 300, 100, 40, 23
    z, _, _, _, weight = ref.make_inputs(N, D, B, S, seed=6)
    nodes = np.array([7, 100, 101, 250, 299])
    rng = np.random.default_rng(6)
    anchor, positive, negative = (nodes[rng.integers(0, 5, k)] for k in (B, B, S))
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    loss = pair_loss(zt, a, p, n, kind=kind, weight=w)
    loss.backward()
    dz = zt.grad.cpu().numpy()
    assert_close_scaled(dz, ref.backward(z, anchor, positive, negative, weight, kind), f'{kind}: dz, 5 shared nodes',
                        scaled=False)
    untouched = np.setdiff1d(np.arange(N), nodes)
    assert (dz[untouched].view(np.uint32) == 0).all()                          # exactly +0
    # ... also where dz starts as NaN: the library call itself, on a pre-filled buffer
    from ampnet_amd import _lib
    lib = _lib.load()
    rc, aff, neg, _, _ = _c_forward(zt.detach(), a, p, n, w, kind)
    aff_t, neg_t = torch.from_numpy(aff).to(dev), torch.from_numpy(neg).to(dev)
    ids = torch.cat((a, p, n))
    ids, order = torch.sort(ids, stable=True)
    slot_idx = order.int()
    slot_ptr = torch.searchsorted(ids, torch.arange(N + 1, device=dev)).int()
    out = torch.full((N, D), float('nan'), device=dev)
    g0 = torch.ones((), device=dev)
    ws = torch.empty(int(lib.ampconv_pair_loss_workspace_bytes(B, S, D)), dtype=torch.uint8, device=dev)
    rc = lib.ampconv_pair_loss_bwd(zt.data_ptr(), N, D, D, a.data_ptr(), p.data_ptr(), B, n.data_ptr(), S, w.data_ptr(),
                                   ref_kind(kind), 1.0, 1.0, 0, aff_t.data_ptr(), neg_t.data_ptr(), g0.data_ptr(),
                                   slot_ptr.data_ptr(), slot_idx.data_ptr(), out.data_ptr(), D, ws.data_ptr(), ws.numel(),
                                   0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(out, zt.grad)
    assert (out.cpu().numpy()[untouched].view(np.uint32) == 0).all()


@pytest.mark.parametrize('kind', KINDS)
def test_excluded_anchors(dev, kind):
    from ampnet_amd import pair_loss
    N, D, B = 150, 32, 70
    z, anchor, positive, _, weight = ref.make_inputs(N, D, B, 1, seed=7)
    negative = np.arange(N, dtype=np.int64)                                    # every node of the batch is a negative
    for dtype in (torch.float32, torch.bfloat16):
        zt, z64 = _stored(z, dtype)
        zt = zt.to(dev).requires_grad_(True)
        a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
        loss = pair_loss(zt, a, p, n, kind=kind, weight=w, exclude_anchor=True)
        loss.backward()
        want = ref.forward(z64, anchor, positive, negative, weight, kind, exclude_anchor=True)
        assert_close_scaled(loss.item(), want[0], f'{kind} {dtype}: loss, anchors excluded', scaled=True)
        rc, aff, neg, _, _ = _c_forward(zt.detach(), a, p, n, w, kind, exclude=True)
        assert rc == 0
        assert_close_scaled(neg, want[2], f'{kind} {dtype}: neg_term, anchors excluded', scaled=False)
        included = ref.forward(z64, anchor, positive, negative, weight, kind)[2]
        assert (np.abs(included - want[2]) > 1e-3).any()                        # the exclusion is visible at this bar
        tol = {} if dtype == torch.float32 else BF16_TOL
        assert_close_scaled(zt.grad.double().cpu().numpy(),
                            ref.backward(z64, anchor, positive, negative, weight, kind, exclude_anchor=True),
                            f'{kind} {dtype}: dz, anchors excluded', scaled=False, **tol)
    # a pair whose only negative is its anchor: a negative term of 0
    a1, p1, n1 = (torch.tensor(v, device=dev) for v in ([2, 3], [4, 1], [2]))
    zt = torch.from_numpy(z).to(dev)
    rc, aff, neg, loss, _ = _c_forward(zt, a1, p1, n1, None, kind, exclude=True)
    want = ref.forward(z, [2, 3], [4, 1], [2], None, kind, exclude_anchor=True)
    assert rc == 0 and neg[0] == 0.0
    assert_close_scaled(neg, want[2], f'{kind}: neg_term, a row without a kept negative', scaled=False)
    assert_close_scaled(loss, want[0], f'{kind}: loss, a row without a kept negative', scaled=True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_strided_z_inside_nan_margins(dev, dtype):
    from ampnet_amd import pair_loss
    N, D, B, S = 90, 40, 33, 21
    z, anchor, positive, negative, weight = ref.make_inputs(N, D, B, S, seed=8)
    zs, z64 = _stored(z, dtype)
    for ld, off in ((D + 8, 4), (D + 3, 1)):                                   # aligned rows, and rows no vector load fits
        big = torch.full((N + 2, ld), float('nan'), dtype=dtype, device=dev)
        view = big[1:N + 1, off:off + D]
        view.copy_(zs)
        view.requires_grad_(True)
        a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
        loss = pair_loss(view, a, p, n, weight=w)
        g, = torch.autograd.grad(loss, view)
        assert_close_scaled(loss.item(), ref.forward(z64, anchor, positive, negative, weight)[0], f'{dtype} ld {ld}: loss',
                            scaled=True)
        tol = {} if dtype == torch.float32 else BF16_TOL
        assert_close_scaled(g.double().cpu().numpy(), ref.backward(z64, anchor, positive, negative, weight),
                            f'{dtype} ld {ld}: dz', scaled=False, **tol)


def test_out_of_range_ids(dev):
    from ampnet_amd import pair_loss
    N, D, B, S = 120, 24, 40, 19
    z, anchor, positive, negative, weight = ref.make_inputs(N, D, B, S, seed=9)
    anchor[3], positive[11], negative[5] = -1, N, 2 ** 40
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    for kind in KINDS:
        zt.grad = None
        loss = pair_loss(zt, a, p, n, kind=kind, weight=w)
        loss.backward()
        ca, cp, cn = (ref.clamp_ids(t, N) for t in (anchor, positive, negative))
        assert_close_scaled(loss.item(), ref.forward(z, ca, cp, cn, weight, kind)[0], f'{kind}: loss, clamped ids', scaled=True)
        assert_close_scaled(zt.grad.cpu().numpy(), ref.backward(z, ca, cp, cn, weight, kind), f'{kind}: dz, clamped ids',
                            scaled=False)
        assert _c_forward(zt.detach(), a, p, n, w, kind)[4] != 0
        with pytest.raises(ValueError, match='outside'):
            pair_loss(zt, a, p, n, kind=kind, weight=w, check_indices=True)
    good = torch.from_numpy(ref.clamp_ids(anchor, N)).to(dev)
    pair_loss(zt, good, good, good, check_indices=True)                        # in range: no error


def test_reproducible_and_upstream_gradient(dev):
    from ampnet_amd import pair_loss
    z, anchor, positive, negative, weight = ref.make_inputs(300, 100, 700, 900, seed=10)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    for kind in KINDS:
        runs = []
        for _ in range(2):
            zt = torch.from_numpy(z).to(dev).requires_grad_(True)
            loss = pair_loss(zt, a, p, n, kind=kind, weight=w)
            loss.backward()
            runs.append((loss.detach(), zt.grad))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # bitwise
    # (3 loss).backward() = 3 x the gradient: g0 enters every role gradient as one more factor, so the two differ by a few
    # roundings per term -- the flat fp32 bar, at a ladder shape where dz itself sits at a few per cent of it
    z, anchor, positive, negative, weight = ref.make_inputs(300, 100, 33, 33, seed=13)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    for kind in KINDS:
        grads = []
        for mul in (1.0, 3.0):
            zt = torch.from_numpy(z).to(dev).requires_grad_(True)
            (mul * pair_loss(zt, a, p, n, kind=kind, weight=w)).backward()
            grads.append(zt.grad.double().cpu().numpy())
        assert_close_scaled(grads[1], 3 * grads[0], f'{kind}: dz for the upstream gradient 3', scaled=False)
        assert_close_scaled(grads[1], ref.backward(z, anchor, positive, negative, weight, kind, g0=3.0),
                            f'{kind}: dz for the upstream gradient 3, fp64 model', scaled=False)


def test_refusals_write_nothing(dev):
    N, D, B, S = 50, 16, 8, 6
    z, anchor, positive, negative, weight = ref.make_inputs(N, D, B, S, seed=11)
    zt = torch.from_numpy(z).to(dev)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    wide = torch.zeros(N, 257, device=dev)
    cases = {'D = 257': (wide, a, p, n, {}), 'S = 0 with B > 0': (zt, a, p, n[:0], {}),
             'NULL anchors': (zt, a, p, n, {'null_anchor': True}), 'ldz < D': (zt, a, p, n, {'ldz': D - 1}),
             'short workspace': (zt, a, p, n, {'ws_bytes': 8})}
    for name, (zz, aa, pp, nn, kw) in cases.items():
        rc, aff, neg, loss, oob = _c_forward(zz, aa, pp, nn, w, 'skipgram', **kw)
        assert rc == (-3 if name == 'short workspace' else -1), name            # AMPCONV_E_WORKSPACE, AMPCONV_E_BADARG
        assert loss == 7.0 and oob == 7 and (aff == 7).all() and (neg == 7).all(), name


def test_memory_stays_far_below_one_logit_table(dev):
    """A condition, not a measurement: one [B, S] fp32 table is 67 MB; the role gradients and the workspace of the design
    are about 5 MB, and a forward plus backward may allocate less than a quarter of the table above its inputs."""
    from ampnet_amd import pair_loss
    N, D, B, S = 4096, 100, 4096, 4096
    z, anchor, positive, negative, weight = ref.make_inputs(N, D, B, S, seed=12)
    zt = torch.from_numpy(z).to(dev).requires_grad_(True)
    a, p, n, w = (torch.from_numpy(t).to(dev) for t in (anchor, positive, negative, weight))
    pair_loss(zt, a, p, n, weight=w).backward()                                # the library is loaded, the caches are warm
    zt.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    pair_loss(zt, a, p, n, weight=w).backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    print(f'[mem] peak rise {rise / 1e6:.2f} MB, bound {B * S * 4 / 4 / 1e6:.2f} MB')
    assert rise < B * S * 4 / 4


def test_end_to_end_training_lowers_the_loss(dev):
    from ampnet_amd import AMPGCN, FusedAdam, pair_loss, walk_pairs
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    N = 64
    cluster = torch.arange(N) // 32
    x = torch.randn(N, 6, generator=g) + 2.0 * cluster[:, None]
    src = torch.randint(0, 32, (400,), generator=g) + 32 * (torch.arange(400) % 2)
    dst = torch.randint(0, 32, (400,), generator=g) + 32 * (torch.arange(400) % 2)     # edges stay inside a cluster
    data = types.SimpleNamespace(x=x.to(dev), edge_index=torch.stack((src, dst)).to(dev))
    walks = torch.randint(0, 32, (48, 4), generator=g) + 32 * (torch.arange(48) % 2)[:, None]   # fixed walks, one cluster each
    anchors, positives = walk_pairs(walks.to(dev), window=2, symmetric=True)
    negatives = torch.arange(N, device=dev)
    model = AMPGCN(device=dev, embedding_dim=8, num_heads=2, num_node_features=6, num_sampled_vectors=4, feat_emb_dim=7,
                   output_dim=3, dropout_rate=0.0, dropout_adj_rate=0.0, seed=2).to(dev)
    model.train()
    opt = FusedAdam(model.parameters(), lr=1e-2)
    losses = []
    for step in range(20):
        model.zero_grad(set_to_none=True)
        z = model.embed(data, model.sampled_node_feat_indices)                 # the first step's feature sample, kept
        assert z.shape == (N, 8)
        loss = pair_loss(z, anchors, positives, negatives, exclude_anchor=True, reduction='mean')
        loss.backward()
        if step == 0:
            for name, prm in model.named_parameters():
                if name.startswith('final_linear_out.'):
                    assert prm.grad is None, name                               # the classifier head is behind the embedding
                else:
                    assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
        opt.step()
        losses.append(loss.item())
    print('[e2e] loss', ' '.join(f'{v:.4f}' for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
