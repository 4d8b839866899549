"""CPU checks of the attention heatmap (ampnet_amd/heatmap.py): the numpy restatement of the accumulation rule that the
GPU tests use as their oracle is pinned to the fixtures written by the reference's calculate_attn_heatmap
(tools/make_golden_heatmap.py), and the accumulator's host logic -- merge, result, guards, all_reduce -- runs on CPU
tensors.  No kernel runs here."""
import glob
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN_DIR, load_golden

HEATMAP_FIXTURES = sorted(glob.glob(os.path.join(GOLDEN_DIR, 'heatmap', 'heatmap_*.npz')))


def heat_restatement(W, tok, edge_index, src_features, dst_features, edge_sel=None):
    """sum, cnt, heat [rows, cols] (float64, int64, float64).  For every selected edge e = (s -> d), destination token i
    and source token j with r = pos_src[tok[s, j]] >= 0 and c = pos_dst[tok[d, i]] >= 0: sum[r, c] += W[e, i, j],
    cnt[r, c] += 1; heat = sum / cnt, 0 where cnt == 0.  W [E, L, L] belongs to the columns of edge_index."""
    W = np.asarray(W, dtype=np.float64)
    tok, edge_index = np.asarray(tok), np.asarray(edge_index)
    src_features, dst_features = np.asarray(src_features), np.asarray(dst_features)
    F = int(max(tok.max(initial=0), src_features.max(), dst_features.max())) + 1
    pos_src, pos_dst = np.full(F, -1), np.full(F, -1)
    pos_src[src_features] = np.arange(len(src_features))
    pos_dst[dst_features] = np.arange(len(dst_features))
    sel = np.ones(edge_index.shape[1], dtype=bool) if edge_sel is None else np.asarray(edge_sel, dtype=bool)
    r = pos_src[tok[edge_index[0, sel]]][:, None, :]                  # [e, 1, j]
    c = pos_dst[tok[edge_index[1, sel]]][:, :, None]                  # [e, i, 1]
    r, c = np.broadcast_arrays(r, c)
    ok = (r >= 0) & (c >= 0)
    rows, cols = len(src_features), len(dst_features)
    flat = (r * cols + c)[ok]
    s = np.bincount(flat, weights=W[sel][ok], minlength=rows * cols).reshape(rows, cols)
    n = np.bincount(flat, minlength=rows * cols).reshape(rows, cols).astype(np.int64)
    return s, n, np.divide(s, n, out=np.zeros_like(s), where=n != 0)


def load_heatmap_fixture(path):
    f = load_golden(path)
    g = load_golden(os.path.join(GOLDEN_DIR, str(f['base']) + '.npz'))
    return f, g


def class_selection(f, edge_index):
    cls = f['node_class']
    return f['edge_mask'] & (cls[edge_index[0]] == f['src_class']) & (cls[edge_index[1]] == f['dst_class'])


def test_fixtures_cover_both_kinds():
    assert len(HEATMAP_FIXTURES) >= 4
    kinds = set()
    for p in HEATMAP_FIXTURES:
        f, _ = load_heatmap_fixture(p)
        kinds.add(bool(f['edge_mask'].all()))
        for t in (f['heat_class'], f['heat_all']):
            assert (t != 0).mean() >= 1 / 3
    assert kinds == {True, False}                       # weights for all edges, and for a subset used as the mask


@pytest.mark.parametrize('path', HEATMAP_FIXTURES, ids=[os.path.basename(p)[:-4] for p in HEATMAP_FIXTURES])
def test_restatement_reproduces_the_reference_tables(path):
    f, g = load_heatmap_fixture(path)
    ei = g['edge_index']
    W = np.zeros((ei.shape[1],) + g['attn_output_weights'].shape[1:])
    W[g['w_edges']] = g['attn_output_weights']
    _, _, heat = heat_restatement(W, f['token_features'], ei, f['src_features'], f['dst_features'],
                                  class_selection(f, ei))
    assert heat.shape == f['heat_class'].shape
    assert np.abs(heat - f['heat_class']).max() <= 1e-12
    _, _, heat = heat_restatement(W, f['token_features'], ei, f['all_features'], f['all_features'], f['edge_mask'])
    assert np.abs(heat - f['heat_all']).max() <= 1e-12


def _filled(seed, src=(3, 5, 9), dst=(1, 2)):
    from ampnet_amd import AttentionHeatmap
    h = AttentionHeatmap(list(src), list(dst))
    g = torch.Generator().manual_seed(seed)
    h.cnt = torch.randint(0, 5, h.shape, generator=g)
    h.sum = torch.randint(0, 1 << 28, h.shape, generator=g) * h.cnt
    h.triples = int(h.cnt.sum())
    h.num_heads = 4
    return h


def test_merge_is_exact_and_commutative():
    a, b = _filled(1), _filled(2)
    ab = _filled(1).merge(b)
    ba = _filled(2).merge(a)
    assert torch.equal(ab.sum, ba.sum) and torch.equal(ab.cnt, ba.cnt)
    assert torch.equal(ab.sum, a.sum + b.sum) and torch.equal(ab.cnt, a.cnt + b.cnt)
    assert ab.triples == ba.triples == a.triples + b.triples
    assert ab.sum.dtype == torch.int64 and ab.device.type == 'cpu'


def test_result_divides_by_scale_and_count():
    from ampnet_amd import AttentionHeatmap
    from ampnet_amd import heatmap
    h = AttentionHeatmap([7, 2], [4, 0, 9])
    assert h.shape == (2, 3) and h.shift == heatmap.SHIFT == 28
    assert 2.0 ** -(h.shift + 1) <= 1e-7                           # per-term error bound of the fixed point
    h.sum = torch.tensor([[3 << 27, 0, 1 << 28], [0, 5, 0]])
    h.cnt = torch.tensor([[3, 0, 1], [0, 2, 0]])
    r = h.result()
    assert r.dtype == torch.float64
    want = torch.tensor([[0.5, 0.0, 1.0], [0.0, 2.5 / 2 ** 28, 0.0]], dtype=torch.float64)
    assert torch.equal(r, want)
    assert torch.equal(h.counts(), h.cnt) and h.counts() is not h.cnt
    assert (r[h.cnt == 0] == 0).all()
    same = AttentionHeatmap([7, 2])                                # dst_features=None: the same list
    assert same.shape == (2, 2) and torch.equal(same.dst_features, same.src_features)
    full = AttentionHeatmap(num_features=5)
    assert full.shape == (5, 5) and full.src_features.tolist() == [0, 1, 2, 3, 4]


def test_bad_feature_lists_raise():
    from ampnet_amd import AttentionHeatmap
    with pytest.raises(ValueError, match='more than once'):
        AttentionHeatmap([1, 2, 1])
    with pytest.raises(ValueError, match='more than once'):
        AttentionHeatmap([1, 2], [3, 3])
    with pytest.raises(ValueError):
        AttentionHeatmap()
    with pytest.raises(ValueError):
        AttentionHeatmap([1, 9], num_features=5)


def test_overflow_guard_raises_instead_of_wrapping():
    from ampnet_amd import heatmap
    assert heatmap.MAX_TRIPLES * (1 << heatmap.SHIFT) < 2 ** 63 <= (heatmap.MAX_TRIPLES + 2) * (1 << heatmap.SHIFT)
    a, b = _filled(1), _filled(2)
    before = a.sum.clone()
    a.triples = heatmap.MAX_TRIPLES - b.triples + 1
    with pytest.raises(ValueError, match='overflow'):
        a.merge(b)
    assert torch.equal(a.sum, before)                              # refused, not applied
    a.triples = heatmap.MAX_TRIPLES - b.triples
    a.merge(b)
    assert a.triples == heatmap.MAX_TRIPLES


def test_merge_shape_mismatch_raises():
    a = _filled(1)
    with pytest.raises(ValueError):
        a.merge(_filled(2, src=(3, 5)))
    with pytest.raises(ValueError):
        a.merge(_filled(2, src=(3, 5, 8)))                         # same shape, other features
    with pytest.raises(TypeError):
        a.merge(a.sum)


def test_update_refuses_softmax_free_layers():
    from ampnet_amd import AMPConv, AttentionHeatmap
    layer = AMPConv(8, 2, softmax=False)
    with pytest.raises(NotImplementedError):
        AttentionHeatmap([0, 1]).update(layer, torch.zeros(3, 2, dtype=torch.int64))


def test_top_features_counts_presence():
    from ampnet_amd import top_features
    x = torch.tensor([[1., 0, 1, 0], [1, 0, 0, 0], [1, 1, 1, 0], [0, 1, 0, 1]])
    y = torch.tensor([0, 0, 0, 1])
    assert top_features(x, y, 0, k=2).tolist() == [0, 2]
    assert top_features(x, y, 1, k=30).numel() == 4


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    h = _filled(10 + rank)
    h.all_reduce()
    torch.save({'sum': h.sum, 'cnt': h.cnt, 'triples': h.triples}, os.path.join(out_dir, f'h{rank}.pt'))
    dist.destroy_process_group()


def test_all_reduce_world2_equals_merge(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want = _filled(10).merge(_filled(11))
    for rank in range(world):
        got = torch.load(os.path.join(tmp_path, f'h{rank}.pt'))
        assert torch.equal(got['sum'], want.sum) and torch.equal(got['cnt'], want.cnt)
        assert got['triples'] == want.triples
