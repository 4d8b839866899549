"""The GCN baseline on the GPU (csrc/gcn.hip, ampnet_amd/gcn.py, GCNConv, GCN) against the fp64 model of
tests/gcn_reference.py.  All inputs are CPU-seeded; references are computed once per case and shared.

Tolerances: the project's flat bar (atol 1e-5, rtol 1e-4) on per-row outputs (out, dh, h, log-probabilities, the loss);
parameter gradients (sums over the nodes) on the magnitude-scaled bar of conftest.assert_close_scaled.  With h, g ~ N(0, 1)
a plain fp32 index_add_ restatement sits at <= 4.6e-6 on the ladder graph (hub of 2500, C = 64): the flat bar has room.
What these shapes do not reach (C > 16 in the input kernels, more than 64 rows per chunk of the weight gradient, the
column sum past 32768 rows, parts and long rows beyond one launch) is on the ladders of tests/test_gpu_gcn_kernels.py.
"""
import functools
import importlib.util
import math
import os
import types

import numpy as np
import pytest
import torch

import gcn_reference as R
from conftest import ROOT, assert_close_scaled

from ampnet_amd import (GCN, EdgeCSR, FusedAdam, GCNConv, GraphSAINTRandomWalkSampler, HeadMetrics, _lib, gcn_aggregate,
                        gcn_norm)
from ampnet_amd.gcn import LONG_SEGMENT, gcn_input_linear, zscore_stats
from ampnet_amd.graph import _stream

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LADDER_N = 400
VARIANTS = {'plain': dict(bias=True, improved=False, loops=True), 'nobias': dict(bias=False, improved=False, loops=True),
            'improved': dict(bias=True, improved=True, loops=True), 'noloops': dict(bias=True, improved=False, loops=False)}


@functools.lru_cache(maxsize=None)
def ladder(flip=False):
    """N = 400.  Segment lengths (in-degrees) 0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, LONG_SEGMENT - 1,
    LONG_SEGMENT, LONG_SEGMENT + 1 and 2500 on nodes 0..16; about 5 % of the entries are self-loops; node 388 has three
    copies of its loop, node 389's only edge is its loop; 20 duplicated edges; nodes 390..399 are isolated.
    flip: the transposed graph, i.e. the same ladder on the source side."""
    rng = np.random.default_rng(7)
    lengths = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, LONG_SEGMENT - 1, LONG_SEGMENT, LONG_SEGMENT + 1, 2500]
    lengths += list(rng.integers(0, 9, 388 - len(lengths)))                       # nodes 17..387
    src, dst = [], []
    for d, n in enumerate(lengths):
        s = rng.integers(0, 388, n)
        s[rng.random(n) < 0.05] = d                                               # self-loops inside the segment
        src.append(s)
        dst.append(np.full(n, d))
    src, dst = np.concatenate(src), np.concatenate(dst)
    pick = rng.choice(np.nonzero((dst > 16) & (src != dst))[0], 20, replace=False)  # duplicates outside the ladder rows
    src, dst = np.concatenate([src, src[pick], [388, 388, 388, 5, 388, 389]]), \
        np.concatenate([dst, dst[pick], [388, 388, 388, 388, 20, 389]])
    perm = rng.permutation(src.shape[0])
    ei = np.stack([src[perm], dst[perm]]).astype(np.int64)
    indeg = np.bincount(ei[1], minlength=LADDER_N)
    assert list(indeg[:17]) == lengths[:17] and (indeg[390:] == 0).all() and not np.isin(ei[0], np.arange(390, 400)).any()
    loops = (ei[0] == ei[1]).mean()
    assert 0.03 < loops < 0.08, loops
    return ei[::-1].copy() if flip else ei


@functools.lru_cache(maxsize=None)
def operands(C, seed=0):
    g = torch.Generator().manual_seed(100 + C + seed)
    return (torch.randn(LADDER_N, C, generator=g), torch.randn(LADDER_N, C, generator=g), torch.randn(C, generator=g))


@functools.lru_cache(maxsize=None)
def aggregate_reference(flip, C, variant):
    v = VARIANTS[variant]
    h, g, b = (t.numpy() for t in operands(C))
    out = R.aggregate(h, ladder(flip), b if v['bias'] else None, v['improved'], v['loops'])
    dh, db = R.aggregate_backward(g, ladder(flip), v['improved'], v['loops'])
    return out, dh, db


def run_aggregate(flip, C, variant):
    v = VARIANTS[variant]
    h, g, b = (t.to(DEV) for t in operands(C))
    h.requires_grad_(True)
    bias = b.clone().requires_grad_(True) if v['bias'] else None
    ei = torch.from_numpy(ladder(flip)).to(DEV)
    out = gcn_aggregate(h, ei, bias, v['improved'], v['loops'])
    out.backward(g)
    return out.detach(), h.grad, None if bias is None else bias.grad


CASES = [(flip, C, 'plain') for flip in (False, True) for C in (1, 2, 3, 4, 7, 16, 17, 64, 100)] + \
        [(flip, C, var) for flip in (False, True) for C in (7, 16) for var in ('nobias', 'improved', 'noloops')]


@pytest.mark.parametrize('flip, C, variant', CASES, ids=lambda v: str(v))
def test_aggregate_against_fp64(flip, C, variant):
    out, dh, db = run_aggregate(flip, C, variant)
    want_out, want_dh, want_db = aggregate_reference(flip, C, variant)
    tag = f'{"flipped " if flip else ""}ladder C={C} {variant}'
    assert_close_scaled(out.cpu().numpy(), want_out, f'{tag}: out')
    assert_close_scaled(dh.cpu().numpy(), want_dh, f'{tag}: dh')
    if db is not None:
        assert_close_scaled(db.cpu().numpy(), want_db, f'{tag}: gb')
    if variant == 'noloops':                                                  # dinv = 0: the row is exactly the bias
        b = operands(C)[2].to(DEV)
        ei = ladder(flip)
        empty = np.setdiff1d(np.arange(LADDER_N), ei[1])
        assert empty.size >= 10 and torch.equal(out[torch.from_numpy(empty).to(DEV)], b.expand(empty.size, C))


def test_gcn_norm_counts_and_cache():
    for flip in (False, True):
        ei = torch.from_numpy(ladder(flip)).to(DEV)
        csr = EdgeCSR(ei, LADDER_N)
        for improved, loops in ((False, True), (True, True), (False, False)):
            dinv = gcn_norm(csr, None, improved, loops)
            want = R.gcn_norm(ladder(flip), LADDER_N, improved, loops)[3]
            np.testing.assert_allclose(dinv.cpu().numpy(), want, rtol=2e-7, atol=0)
            assert gcn_norm(csr, LADDER_N, improved, loops) is dinv            # one launch per (improved, add_self_loops)
        assert len(csr._gcn_dinv) == 3


def _abi_aggregate(lib, h, ld_h, C, ptr, idx, dinv, loops, fill, bias, out, ld_out, N, E, ws):
    _lib.check(lib.ampconv_gcn_aggregate(h.data_ptr(), ld_h, C, ptr.data_ptr(), idx.data_ptr(), dinv.data_ptr(), int(loops),
                                         fill, None if bias is None else bias.data_ptr(), out.data_ptr(), ld_out, N, E,
                                         None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(), _stream()),
               'ampconv_gcn_aggregate')


@pytest.mark.parametrize('C', (1, 7, 16, 17))
@pytest.mark.parametrize('side', ('dst', 'src'))
def test_aggregate_through_the_c_abi_on_views(C, side):
    """ld_h = C + 3 behind a base offset of 4 bytes (the 4-byte-load path; C = 1, 17 make ld a multiple of 4, so it is
    the offset alone that rules the 16-byte path out there); out into a wider buffer whose padding stays untouched."""
    lib = _lib.load()
    N, ei = LADDER_N, ladder(False)
    csr = EdgeCSR(torch.from_numpy(ei).to(DEV), N)
    dinv = gcn_norm(csr, None, False, True)
    ptr, idx = (csr.rowptr, csr.col) if side == 'dst' else (csr.cscptr, csr.crow)
    h, g, b = (t.to(DEV) for t in operands(C))
    src = g if side == 'src' else h
    ld_h, ld_out = C + 3, C + 5
    buf = torch.full((N * ld_h + 1,), float('nan'), device=DEV)
    view = buf[1:].view(N, ld_h)
    view[:, :C] = src
    assert view.data_ptr() % 16 == 4
    sentinel = -12345.0
    out = torch.full((N, ld_out), sentinel, device=DEV)
    nws = lib.ampconv_gcn_aggregate_workspace_bytes(N, csr.num_edges, C)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    bias = b if side == 'dst' else None
    _abi_aggregate(lib, view, ld_h, C, ptr, idx, dinv, True, 1.0, bias, out, ld_out, N, csr.num_edges, ws)
    want = aggregate_reference(False, C, 'plain')[0 if side == 'dst' else 1]
    assert_close_scaled(out[:, :C].cpu().numpy(), want, f'C ABI {side} C={C} ld_h={ld_h}: out')
    assert torch.equal(out[:, C:], torch.full((N, ld_out - C), sentinel, device=DEV))
    # the 16-byte path on padded contiguous rows and the walk of every segment by its lane group (no workspace)
    pad = (C + 3) // 4 * 4
    hp = torch.zeros(N, pad, device=DEV)
    hp[:, :C] = src
    out16 = torch.full((N, pad), sentinel, device=DEV)
    _abi_aggregate(lib, hp, pad, C, ptr, idx, dinv, True, 1.0, bias, out16, pad, N, csr.num_edges, ws)
    assert torch.equal(out16[:, :C], out[:, :C])                              # same bits on both load widths
    assert torch.equal(out16[:, C:], torch.full((N, pad - C), sentinel, device=DEV))
    walked = torch.full((N, pad), sentinel, device=DEV)
    _abi_aggregate(lib, hp, pad, C, ptr, idx, dinv, True, 1.0, bias, walked, pad, N, csr.num_edges, None)
    assert_close_scaled(walked[:, :C].cpu().numpy(), want, f'C ABI {side} C={C} no workspace: out')


def test_c_abi_refuses_bad_arguments():
    lib = _lib.load()
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    bad = lib.ampconv_gcn_aggregate(t.data_ptr(), 3, 4, i.data_ptr(), i.data_ptr(), t.data_ptr(), 1, 1.0, None,
                                    t.data_ptr(), 4, 2, 0, None, 0, _stream())
    assert bad == -1                                                          # ld_h < C
    short = torch.empty(16, dtype=torch.uint8, device=DEV)
    assert lib.ampconv_gcn_aggregate(t.data_ptr(), 4, 4, i.data_ptr(), i.data_ptr(), t.data_ptr(), 1, 1.0, None,
                                     t.data_ptr(), 4, 2, 1000, short.data_ptr(), 16, _stream()) == -3
    assert lib.ampconv_gcn_aggregate_workspace_bytes(10, LONG_SEGMENT - 1, 16) == 0
    assert lib.ampconv_gcn_input_fwd(t.data_ptr(), 2, 2, None, None, t.data_ptr(), t.data_ptr(), 2, 2, t.data_ptr(), 2,
                                     short.data_ptr(), 16, _stream()) == -1   # a table without mean / inv_std


@pytest.mark.parametrize('loops', (True, False))
def test_empty_and_degenerate_graphs(loops):
    g = torch.Generator().manual_seed(3)
    for N, ei in ((1, torch.zeros(2, 0, dtype=torch.int64)), (5, torch.zeros(2, 0, dtype=torch.int64)),
                  (5, torch.tensor([[0, 1, 1, 4, 4, 4], [0, 1, 1, 4, 4, 4]]))):
        h, b = torch.randn(N, 3, generator=g), torch.randn(3, generator=g)
        hd = h.to(DEV).requires_grad_(True)
        out = gcn_aggregate(hd, ei.to(DEV), b.to(DEV), False, loops)
        out.backward(torch.ones_like(out))
        want = R.aggregate(h.numpy(), ei.numpy(), b.numpy(), False, loops)
        assert_close_scaled(out.detach().cpu().numpy(), want, f'N={N} E={ei.size(1)} loops={loops}: out')
        want_dh = R.aggregate_backward(np.ones((N, 3)), ei.numpy(), False, loops)[0]
        assert_close_scaled(hd.grad.cpu().numpy(), want_dh, f'N={N} E={ei.size(1)} loops={loops}: dh')
        if loops:                                                             # every node keeps exactly its own loop
            assert torch.equal(out.detach(), hd.detach() + b.to(DEV))


# ---- the first layer over the embedded input

INPUT_CASES = [(1, 2, 2, 2), (64, 2, 2, 2), (65, 33, 3, 5), (300, 1433, 99, 16), (257, 1433, 0, 16)]


def sparse_x(N, F, seed):
    """synthetic_cora-like sparse binary features with one constant column (inv_std = 1) and one column present in a
    single node (|z| ~ sqrt(N))."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, F, generator=g) < 0.02).float()
    x[torch.arange(N), torch.randint(0, F, (N,), generator=g)] = 1.0
    x[:, 3 % F] = 1.0
    if F > 8:
        x[:, 7] = 0.0
        x[N // 2, 7] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def input_operands(N, F, De, C):
    g = torch.Generator().manual_seed(N * 7 + F)
    x = sparse_x(N, F, N + F) if F > 8 else torch.randn(N, F, generator=g)
    bound = math.sqrt(6.0 / (F * (De + 1) + C))
    W = (torch.rand(C, F * (De + 1), generator=g) * 2 - 1) * bound
    table = torch.randn(F, De, generator=g) if De else None
    return x, W, table, torch.randn(N, C, generator=g)


@functools.lru_cache(maxsize=None)
def input_reference(N, F, De, C, mode):
    x, W, table, g = (None if t is None else t.numpy() for t in input_operands(N, F, De, C))
    h = R.input_linear(x, W, table, mode)
    dW, dtable = R.input_linear_backward(x, W, table, g, mode)
    return h, dW, dtable


def run_input(N, F, De, C, mode):
    x, W, table, g = (None if t is None else t.to(DEV) for t in input_operands(N, F, De, C))
    W.requires_grad_(True)
    if table is not None:
        table.requires_grad_(True)
    mean, inv_std = (None, None) if mode == 'raw' else zscore_stats(x)
    h = gcn_input_linear(x, W, table, mean, inv_std)
    h.backward(g)
    return h.detach(), W.grad, None if table is None else table.grad


@pytest.mark.parametrize('N, F, De, C, mode', [c + ('embedded',) for c in INPUT_CASES[:4]] +
                         [INPUT_CASES[4] + ('zscore',), INPUT_CASES[4] + ('raw',)])
def test_input_kernels_against_the_materialised_fp64_model(N, F, De, C, mode):
    h, dW, dtable = run_input(N, F, De, C, mode)
    want_h, want_dW, want_dtable = input_reference(N, F, De, C, mode)
    tag = f'input {mode} N={N} F={F} De={De} C={C}'
    assert h.stride(0) % 4 == 0 or N == 1                                     # rows padded for the 16-byte path
    assert_close_scaled(h.cpu().numpy(), want_h, f'{tag}: h')
    assert_close_scaled(dW.cpu().numpy(), want_dW, f'{tag}: gW')
    if De:                                  # a parameter gradient, a sum over all nodes: the scaled bar, as for gW
        assert_close_scaled(dtable.cpu().numpy(), want_dtable, f'{tag}: g_table', scaled=True)


def test_bitwise_run_to_run():
    runs = [run_aggregate(False, 16, 'plain') + run_aggregate(True, 100, 'plain') + run_input(65, 33, 3, 5, 'embedded')
            + run_input(300, 1433, 99, 16, 'embedded')[1:] for _ in range(3)]
    for other in runs[1:]:
        for name, a, b in zip(('out', 'dh', 'db', 'out100', 'dh100', 'db100', 'h', 'dW', 'dtable', 'dW wide', 'dtable wide'),
                              runs[0], other):
            assert torch.equal(a, b), name


# ---- the model

CONFIGS = {'xor': dict(N=64, E=256, F=2, De=2, hidden=2, C=2), 'cora': dict(N=300, E=2400, F=1433, De=99, hidden=16, C=7)}


@functools.lru_cache(maxsize=None)
def model_data(name):
    c = CONFIGS[name]
    g = torch.Generator().manual_seed(len(name) + c['N'])
    x = sparse_x(c['N'], c['F'], 5) if c['F'] > 8 else torch.randn(c['N'], c['F'], generator=g)
    return types.SimpleNamespace(
        x=x, edge_index=torch.randint(0, c['N'], (2, c['E']), generator=g), y=torch.randint(0, c['C'], (c['N'],), generator=g),
        node_norm=torch.rand(c['N'], generator=g) + 0.5, train_mask=torch.rand(c['N'], generator=g) < 0.7)


def on_device(d):
    return types.SimpleNamespace(**{k: v.to(DEV) for k, v in vars(d).items()})


def make_model(name, mode, **kw):
    c = CONFIGS[name]
    torch.manual_seed(11)
    m = GCN(DEV, num_node_features=c['F'], hidden_dim=c['hidden'], num_sampled_vectors=c['F'], output_dim=c['C'],
            feat_emb_dim=c['De'], input=mode, **{'dropout_rate': 0.0, 'dropout_adj_rate': 0.0, **kw}).to(DEV)
    with torch.no_grad():
        m.conv1.bias.normal_(0, 0.1)
        m.conv2.bias.normal_(0, 0.1)
    return m


@functools.lru_cache(maxsize=None)
def model_reference(name, mode):
    d = model_data(name)
    P = {k: v.detach().cpu().numpy() for k, v in make_model(name, mode).state_dict().items()}
    return R.model(d.x.numpy(), d.edge_index.numpy(), P, mode, d.y.numpy(), d.node_norm.numpy(), d.train_mask.numpy())


def saint_loss(out, d):
    return (torch.nn.functional.nll_loss(out, d.y, reduction='none') * d.node_norm)[d.train_mask].sum()


@pytest.mark.parametrize('training', (False, True), ids=('eval', 'train'))
@pytest.mark.parametrize('mode', ('embedded', 'zscore', 'raw'))
@pytest.mark.parametrize('name', ('xor', 'cora'))
def test_model_against_fp64(name, mode, training):
    ref, d, m = model_reference(name, mode), on_device(model_data(name)), make_model(name, mode)
    m.train(training)
    out = m(d)
    loss = saint_loss(out, d)
    loss.backward()
    tag = f'{name} {mode} {"train" if training else "eval"}'
    assert_close_scaled(out.detach().cpu().numpy(), ref['logp'], f'{tag}: log-probabilities')
    assert_close_scaled(loss.item(), ref['loss'], f'{tag}: loss')
    for k, p in m.named_parameters():
        if ref['grads'][k] is None:
            assert p.grad is None, k                                           # the table is unused outside 'embedded'
        else:
            assert_close_scaled(p.grad.cpu().numpy(), ref['grads'][k], f'{tag}: {k}.grad')


def test_memory_of_the_embedded_model_stays_far_below_the_materialised_input():
    c = CONFIGS['cora']
    d, m = on_device(model_data('cora')), make_model('cora', 'embedded')
    saint_loss(m(d), d).backward()                                             # warm: library, graph cache, allocator
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    saint_loss(m(d), d).backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    materialised = c['N'] * c['F'] * (c['De'] + 1) * 4
    print(f'[mem] peak growth {growth / 1e6:.1f} MB, materialised input {materialised / 1e6:.1f} MB')
    assert growth < materialised / 2


@pytest.mark.parametrize('name', ('xor', 'cora'))
def test_fused_head_and_nll_loss_agree_with_the_unfused_path(name):
    d = on_device(model_data(name))
    plain, fused = make_model(name, 'embedded'), make_model(name, 'embedded', fused_head=True)
    out = plain(d)
    loss = saint_loss(out, d)
    loss.backward()
    out_f = fused(d)
    assert_close_scaled(out_f.detach().cpu().numpy(), out.detach().cpu().numpy(), f'{name}: fused head log-probabilities')
    metrics = HeadMetrics(2, DEV)
    test_mask = ~d.train_mask
    loss_f = fused.nll_loss(d, masks=(d.train_mask, test_mask), metrics=metrics)
    loss_f.backward()
    assert_close_scaled(loss_f.item(), loss.item(), f'{name}: fused loss')
    for (k, p), (_, q) in zip(plain.named_parameters(), fused.named_parameters()):
        assert_close_scaled(q.grad.cpu().numpy(), p.grad.cpu().numpy(), f'{name}: fused {k}.grad')
    got = metrics.read()
    correct = out.argmax(1) == d.y
    assert got['count'] == [int(d.train_mask.sum()), int(test_mask.sum())]
    assert got['correct'] == [int(correct[d.train_mask].sum()), int(correct[test_mask].sum())]
    assert got['bad_labels'] == 0
    assert abs(got["loss_sum"][0] - loss.item()) <= 1e-5 + 1e-4 * abs(loss.item())


def test_fused_glue_dropout_is_seeded_and_keeps_its_share():
    d = on_device(model_data('cora'))
    a, b = (make_model('cora', 'embedded', fused_glue=True, dropout_rate=0.3, seed=5) for _ in range(2))
    out_a, out_b = a.train()(d), b.train()(d)
    assert torch.equal(out_a, out_b)                                           # same seed, same call count
    assert not torch.equal(a(d), out_a)                                        # the next call draws another mask
    c = make_model('cora', 'embedded', fused_glue=True, dropout_rate=0.3, seed=5)
    with torch.no_grad():
        dropped = c.train()._hidden(d)[0]
        full = c.eval()._hidden(d)[0]
    live = full > 0
    n = int(live.sum())
    kept = int((dropped[live] != 0).sum()) / n
    sigma = math.sqrt(0.7 * 0.3 / n)
    print(f'[dropout] kept {kept:.4f} of {n} live activations, sigma {sigma:.4f}')
    assert abs(kept - 0.7) <= 4 * sigma
    assert torch.equal(dropped[~live], torch.zeros_like(dropped[~live]))
    np.testing.assert_allclose(dropped[live & (dropped != 0)].cpu().numpy(), (full[live & (dropped != 0)] / 0.7).cpu().numpy(),
                               rtol=1e-4)


def _example():
    spec = importlib.util.spec_from_file_location('train_graphsaint_gcn', os.path.join(ROOT, 'examples', 'train_graphsaint.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_thirty_fused_adam_steps_reduce_the_loss():
    ex = _example()
    data = ex.synthetic_cora(torch.device(DEV))
    loader = GraphSAINTRandomWalkSampler(data, batch_size=8, walk_length=150, num_steps=1, sample_coverage=5, seed=1)
    batch = next(iter(loader))
    torch.manual_seed(2)
    m = GCN(DEV, num_node_features=1433, hidden_dim=16, num_sampled_vectors=1433, output_dim=7, dropout_rate=0.0,
            dropout_adj_rate=0.0, fused_head=True).to(DEV)
    opt = FusedAdam(m.parameters(), lr=0.005, weight_decay=1e-4)
    losses = []
    for _ in range(30):
        m.train()
        loss = m.nll_loss(batch, masks=batch.train_mask)
        loss.backward()
        opt.step(set_to_none=True)
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().tolist()
    print(f'[train] loss {losses[0]:.4f} -> {losses[-1]:.4f}')
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def test_example_trains_the_baseline():
    history, acc = _example().main(['--model', 'gcn', '--epochs', '1', '--steps', '2'])
    assert len(history) == 1 and all(math.isfinite(v) for v in history[0]) and 0.0 <= acc <= 1.0


def test_gcnconv_layer_matches_its_definition():
    torch.manual_seed(4)
    conv = GCNConv(9, 7, improved=True).to(DEV)
    with torch.no_grad():
        conv.bias.normal_()
    g = torch.Generator().manual_seed(9)
    x, ei = torch.randn(LADDER_N, 9, generator=g), torch.from_numpy(ladder(False))
    out = conv(x.to(DEV), ei.to(DEV))
    want = R.aggregate(x.numpy().astype(np.float64) @ conv.lin.weight.detach().cpu().numpy().astype(np.float64).T, ei.numpy(),
                       conv.bias.detach().cpu().numpy(), improved=True)
    assert_close_scaled(out.detach().cpu().numpy(), want, 'GCNConv(9, 7, improved): out')
    with pytest.raises(ValueError, match='float32'):
        conv(x.to(DEV).half(), ei.to(DEV))
    with pytest.raises(ValueError, match='int64'):
        conv(x.to(DEV), ei.to(DEV).int())
