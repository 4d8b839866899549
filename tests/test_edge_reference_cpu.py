"""Pins tests/edge_reference.py -- the per-pass fp64 model the GPU tests of the edge C ABI compare against -- at fp64
round-off, two independent ways: against the whole-layer oracle with identity projections, and against torch autograd on
a per-edge loop.  No GPU."""
import numpy as np
import pytest
import torch

import edge_reference as er
from oracle.ampconv_numpy import AMPConvOracle

RTOL = 1e-12


def graph():
    """12 nodes, 40 edges: nodes 9..11 receive nothing (empty rows), node 10 sends nothing either, self-loops on 0 and
    3, the edge 1 -> 2 three times."""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 10, 34)
    dst = rng.integers(0, 9, 34)
    src[src == 10] = 11
    src = np.concatenate([src, [0, 3, 1, 1, 1, 11]])
    dst = np.concatenate([dst, [0, 3, 2, 2, 2, 4]])
    assert 10 not in src and dst.max() < 9
    return src, dst, 12


def close(got, want, name, scale=None):
    scale = np.abs(want).max() if scale is None else scale
    err = np.abs(got - want).max()
    print(f'{name}: max err {err:.3e} at max |want| {scale:.3e}')
    assert err <= RTOL * scale, name


@pytest.mark.parametrize('L,H,dh', [(3, 2, 4), (5, 1, 3)])
def test_against_the_layer_oracle_with_identity_projections(L, H, dh):
    """in_proj = three stacked identities, out_proj = identity, no biases: Q = K = V = x, y is Obar, dObar is dy on the
    rows with in-edges, and dx = dQ + dK + dV, dWin = [dQ^T x; dK^T x; dV^T x], dbin = their column sums."""
    src, dst, N = graph()
    D = H * dh
    rng = np.random.default_rng(1)
    x = rng.standard_normal((N, L, D))
    dy = rng.standard_normal((N, L, D))
    eye = np.eye(D)
    o = AMPConvOracle(np.concatenate([eye, eye, eye]), np.zeros(3 * D), eye, np.zeros(D), H)
    y, _ = o.forward(x.reshape(N, L * D), np.stack([src, dst]), need_weights=False)
    dx, dWin, dbin, _, _ = o.backward(dy.reshape(N, L * D))
    rowptr, col = er.csr_of(src, dst, N)
    X = x.reshape(N, L, H, dh)
    O = er.fwd(X, X, X, rowptr, col)
    close(O.reshape(N, L * D), y, 'Obar')
    assert not O[9:].any()                                        # rows without in-edges: exactly 0
    dQ, dK, dV = (t.reshape(N, L, D) for t in er.bwd(X, X, X, dy.reshape(N, L, H, dh), rowptr, col))
    close((dQ + dK + dV).reshape(N, L * D), dx, 'dQ + dK + dV')
    for i, (g, name) in enumerate(((dQ, 'dQ'), (dK, 'dK'), (dV, 'dV'))):
        close(np.tensordot(g, x, axes=([0, 1], [0, 1])), dWin[i * D:(i + 1) * D], f'{name}^T x')
        # (a cancelling sum -- dK's columns sum to exactly 0, softmax gradients having zero row sums -- is held to
        # round-off relative to its TERMS)
        close(g.sum(axis=(0, 1)), dbin[i * D:(i + 1) * D], f'colsum {name}', scale=np.abs(g).max())


def _torch_edges(Q, K, V, rowptr, col, qidx=None):
    R, (_, L, H, dh) = len(rowptr) - 1, Q.shape
    rows, lse = [], []
    for r in range(R):
        d = r if qidx is None else int(qidx[r])
        acc = torch.zeros(L, H, dh, dtype=torch.float64)
        for p in range(rowptr[r], rowptr[r + 1]):
            s = int(col[p])
            S = torch.einsum('ihc,jhc->hij', Q[d], K[s]) / dh ** 0.5
            lse.append(torch.logsumexp(S, dim=-1) / np.log(2.0))
            acc = acc + torch.einsum('hij,jhc->ihc', torch.softmax(S, dim=-1), V[s])
        rows.append(acc / max(1, rowptr[r + 1] - rowptr[r]))
    return torch.stack(rows), (torch.stack(lse) if lse else None)


@pytest.mark.parametrize('L,H,dh', [(4, 2, 6), (7, 3, 5)])
def test_against_torch_autograd_with_independent_operands(L, H, dh):
    src, dst, N = graph()
    rowptr, col = er.csr_of(src, dst, N)
    g = torch.Generator().manual_seed(3)
    Q, K, V, dO = (torch.randn(N, L, H, dh, dtype=torch.float64, generator=g) for _ in range(4))
    for t in (Q, K, V):
        t.requires_grad_(True)
    O, lse = _torch_edges(Q, K, V, rowptr, col)
    O.backward(dO)
    q, k, v, do = (t.detach().numpy() for t in (Q, K, V, dO))
    close(er.fwd(q, k, v, rowptr, col), O.detach().numpy(), 'O')
    for got, want, name in zip(er.bwd(q, k, v, do, rowptr, col), (Q.grad, K.grad, V.grad), ('dQ', 'dK', 'dV')):
        close(got, want.numpy(), name)
    # statistics: the normaliser against torch.logsumexp; delta_i = sum_j P_ij dP_ij = sum_c g_ic o_ic with o = P V the
    # edge's own output (the identity the kernels' hand-off rests on)
    lse2, delta = er.stats(q, k, v, do, rowptr, col)
    close(lse2, lse.detach().numpy(), 'log2-sum-exp')
    for d in range(N):
        for p in range(rowptr[d], rowptr[d + 1]):
            one = np.array([0, 1])
            o_e = er.fwd(q[[d]], k[[int(col[p])]], v[[int(col[p])]], one, np.array([0]))[0]
            want = (do[d] / (rowptr[d + 1] - rowptr[d]) * o_e).sum(axis=-1).T             # [H, L]
            assert np.abs(delta[p] - want).max() <= RTOL * max(1.0, np.abs(want).max())


def test_forward_with_a_query_index():
    """qidx: row r takes its queries from node qidx[r]; the row count follows rowptr, not N."""
    rng = np.random.default_rng(9)
    N, L, H, dh, R = 6, 3, 2, 4, 9
    deg = rng.integers(0, 4, R)
    deg[2] = 0
    rowptr = np.concatenate([[0], np.cumsum(deg)])
    col = rng.integers(0, N, rowptr[-1])
    qidx = rng.integers(0, N, R)
    assert (qidx != np.arange(R)).any()
    g = torch.Generator().manual_seed(4)
    Q, K, V = (torch.randn(N, L, H, dh, dtype=torch.float64, generator=g) for _ in range(3))
    want, _ = _torch_edges(Q, K, V, rowptr, col, qidx)
    got = er.fwd(Q.numpy(), K.numpy(), V.numpy(), rowptr, col, qidx)
    close(got, want.numpy(), 'O with qidx')
    assert got.shape == (R, L, H, dh) and not got[2].any()


def test_layout_helper_places_without_overlap_and_with_the_alignment_it_names():
    """tests/edge_layouts.py on host buffers: every layout maps the logical elements to distinct positions inside the
    backing buffer with a margin of at least one node's extent on both sides; an input holds NaN and an output the
    sentinel (itself a NaN) everywhere else; the alignment class is the one the layout's name promises."""
    import edge_layouts as el
    N, L, H, dh = 5, 3, 2, 8
    x = np.random.default_rng(0).standard_normal((N, L, H, dh)).astype(np.float32)
    for dtype, esize in ((torch.float32, 4), (torch.bfloat16, 2)):
        for layout in el.LAYOUTS + ('padrow',):
            if layout == 'pad4' and esize == 2:
                continue
            backing, view, index = el.place(x, layout, dtype, 'K', device='cpu')
            flat = index.reshape(-1)
            ns = view.node_stride
            assert len(set(flat.tolist())) == x.size, layout
            assert flat.min() >= ns and flat.max() < backing.numel() - ns, layout
            assert (view.ptr - backing.data_ptr()) // esize == int(index[0, 0, 0, 0]), layout
            assert int(index[1, 2, 1, 3]) - int(index[0, 0, 0, 0]) == ns + 2 * view.row_stride + view.head_stride + 3
            want = torch.from_numpy(x).to(dtype).double().numpy()
            assert np.array_equal(el.read(backing, index), want), layout
            outside = torch.ones(backing.numel(), dtype=torch.bool)
            outside[flat] = False
            assert torch.isnan(backing[outside]).all() and outside.sum() >= 2 * ns
            out = el.place((N, L, H, dh), layout, dtype, 'out0', device='cpu')
            assert torch.isnan(out.backing).all() and out.outside_intact() and out.unwritten() == x.size
            out.backing[out.index[2].reshape(-1)] = 0.0
            assert out.outside_intact(slice(2, 3)) and not out.outside_intact(slice(0, 2))
            assert out.unwritten() == x.size - L * H * dh and out.unwritten(slice(2, 3)) == 0
            a = el.alignment_bytes([view], esize)
            assert a == {'pad8': 8, 'pad4': 4}.get(layout, 16), (layout, a)


@pytest.mark.parametrize('chunk,E', [(64, 3926), (128, 7638)])
def test_ladder_graph_holds_the_segment_lengths_it_is_for(chunk, E):
    """tests/edge_runner.py: graph('L', chunk), the graph of tests/test_gpu_edge_ladder.py.  Both degree sequences, the
    edge count, 63 chunks on either side in rows of 2, 3, 4, 5, 9, 13 and 17, self-loops and multi-edges; and
    er.csr_of on it is a STABLE sort by destination."""
    import edge_runner as rn
    c = chunk
    want = list(range(21)) + [c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c - 1, 3 * c, 3 * c + 1,
                              4 * c + 1, 8 * c + 1, 12 * c + 1, 16 * c + 1, 0, 0, 0]
    g = rn.graph('L', chunk)
    assert (g.N, g.n_rows, g.E) == (37, 37, E)
    assert g.indeg.tolist() == want == rn.ladder_degrees(chunk).tolist()
    assert sorted(g.outdeg.tolist()) == sorted(want) and g.outdeg.tolist() != want       # the same multiset, moved
    assert not g.indeg[34:].any() and not g.outdeg[34:].any()                             # three isolated nodes
    for deg in (g.indeg, g.outdeg):
        per_row = rn.chunks_per_row(deg, chunk)
        assert per_row.sum() == rn.LADDER_CHUNKS == 63 and set(per_row.tolist()) == {2, 3, 4, 5, 9, 13, 17}
        assert (deg == chunk).sum() == 1 and len(per_row) == 11                           # exactly `chunk` edges: not cut
    loops = int((g.src == g.dst).sum())
    pairs = np.unique(np.stack([g.src, g.dst]), axis=1).shape[1]
    print(f'chunk {chunk}: {loops} self-loops, {g.E - pairs} repeated edges')
    assert loops >= 100 and pairs < g.E
    # csr_of: the row pointers are the running in-degrees; equal destinations keep the order they came in, also when the
    # edge list arrives shuffled
    assert np.array_equal(g.rowptr, np.concatenate([[0], np.cumsum(want)])) and np.array_equal(g.col, g.src)
    perm = np.random.default_rng(3).permutation(g.E)
    rowptr, col = er.csr_of(g.src[perm], g.dst[perm], g.N)
    assert np.array_equal(rowptr, g.rowptr)
    assert np.array_equal(col, g.src[perm][np.lexsort((np.arange(g.E), g.dst[perm]))])
    for r in (5, 22, 33):                                    # row r holds the sources of its edges in arrival order
        assert np.array_equal(col[rowptr[r]:rowptr[r + 1]], g.src[perm][g.dst[perm] == r])


def test_header_rule_agrees_with_the_family_table():
    """edge_runner.header_rule (the rule of ANY shape, which the token-count sweep uses) gives every listed shape the
    rule the table lists for it."""
    import edge_runner as rn
    for (dtype, shape), rule in rn.TABLE.items():
        assert rn.header_rule(dtype, shape) is rule, (dtype, shape)
    assert rn.header_rule(rn.F32, (4, 32, 4), small=False) is rn._ONE_WAVE
    assert rn.header_rule(rn.F32, (4, 64, 1)) is rn._SMALL_V2 and rn.header_rule(rn.F32, (5, 64, 1)) is rn._PER_UNIT
    assert rn.header_rule(rn.BF16, (20, 96, 1)) is None
