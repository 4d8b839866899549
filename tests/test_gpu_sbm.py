"""The stochastic block model generator on the GPU (csrc/sbm.hip, ampnet_amd/random_graphs.py) against the numpy model of
tests/sbm_reference.py, element for element: edge_index, block and E of every ladder case with every seed and of the
larger case; the two C calls one at a time through ctypes -- ampconv_sbm_count against the model's per-unit counts,
ampconv_sbm_fill, given the model's offsets, into sentinel-filled over-allocated buffers --; refusals; reproducibility;
the XOR link data; one AMPConv forward on a generated graph.

Nothing here is statistical (tests/test_sbm_cpu.py holds the model to its distribution).  A (case, seed) pair is compared
only under the margin condition of sbm_reference (margin >= 1e-9): every pair of the ladder meets it, none is dropped,
and a pair that did not would FAIL here, not be skipped."""
import numpy as np
import pytest
import torch

import sbm_reference as sr
from edge_layouts import place_flat_int
from edge_runner import stream

from ampnet_amd import _lib

pytestmark = pytest.mark.gpu

I64 = torch.int64
BADARG = -1
DEV = 'cuda:0'
SIZE_IDS = ['x'.join(map(str, s)) for s in sr.SIZES]


@pytest.fixture(scope='module')
def lib():
    assert torch.cuda.is_available()
    return _lib.load()


def cases_of(sizes):
    for c in sr.ladder():
        if c[0] == tuple(sizes):
            for seed in sr.SEEDS:
                r = sr.reference(*c, seed)
                assert r.margin >= sr.MARGIN_MIN, (sr.case_id(c), seed, r.margin)
                yield c, seed, r, sr.MATRICES[c[1]](len(sizes))


def differs(got, want, name):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want):
        return []
    where = np.nonzero(np.asarray(got != want).reshape(-1))[0][:6].tolist() if got.shape == want.shape else f'shape {got.shape} vs {want.shape}'
    return [f'{name}: differs from the model at {where}']


# ------------------------------------------------------------------------------------------------------ the public function
@pytest.mark.parametrize('sizes', sr.SIZES, ids=SIZE_IDS)
def test_graph_equals_the_model(sizes, lib):
    from ampnet_amd import stochastic_block_model
    failed = []
    for c, seed, r, P in cases_of(sizes):
        g = stochastic_block_model(list(sizes), P, directed=c[2], selfloops=c[3], seed=seed, device=DEV)
        name = f'{sr.case_id(c)}-seed{seed}'
        assert g.edge_index.dtype == I64 and g.block.dtype == I64 and g.edge_index.is_cuda and g.edge_index.is_contiguous()
        assert g.num_nodes == r.num_nodes
        failed += differs(g.edge_index, r.edge_index, name + ' edge_index') + differs(g.block, r.block, name + ' block')
    assert not failed, failed[:10]


@pytest.mark.parametrize('directed', [True, False], ids=['dir', 'und'])
def test_larger_graph_equals_the_model(directed, lib):
    """sizes [5000] * 4, p_in 2e-3, p_out 2e-4: about 260 k edges, 313 waves per block, chains of ~10 draws."""
    from ampnet_amd import random_partition_graph
    failed = []
    for seed in sr.SEEDS:
        r = sr.big_reference(directed, seed)
        assert r.margin >= sr.MARGIN_MIN, (seed, r.margin)
        g = random_partition_graph(sr.BIG['sizes'], sr.BIG['p_in'], sr.BIG['p_out'], directed=directed, seed=seed, device=DEV)
        failed += differs(g.edge_index, r.edge_index, f'seed {seed} edge_index') + differs(g.block, r.block, f'seed {seed} block')
    assert not failed, failed


# ------------------------------------------------------------------------------------------------- the C calls, one at a time
def tables(P):
    return torch.from_numpy(np.ascontiguousarray(P)).to(DEV), torch.from_numpy(sr.log1p_table(P)).to(DEV)


@pytest.mark.parametrize('sizes', sr.SIZES, ids=SIZE_IDS)
def test_count_and_fill_calls(sizes, lib):
    """count and mcount equal the model's per-unit numbers, everything around them untouched; fill, given the model's
    offsets and a capacity of E + 32, writes exactly the positions [0, E) of row and col -- each inside a larger
    allocation full of the sentinel -- with the model's values, and nothing behind or around them."""
    failed = []
    s = np.asarray(sizes, np.int64)
    K, N = len(sizes), int(s.sum())
    for c, seed, r, P in cases_of(sizes):
        name = f'{sr.case_id(c)}-seed{seed}'
        P_d, lq_d = tables(P)
        head = (s.ctypes.data, K, P_d.data_ptr(), lq_d.data_ptr(), int(c[2]), int(c[3]), seed)
        pc, pm = place_flat_int((N * K,), I64), place_flat_int((N * K,), I64)
        rc = lib.ampconv_sbm_count(*head, pc.ptr, pm.ptr, stream())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        for p, want, what in ((pc, r.count, 'count'), (pm, r.mcount, 'mcount')):
            if not p.outside_intact() or p.unwritten():
                failed.append(f'{name} {what}: written outside, or {p.unwritten()} elements not written')
            failed += differs(p.backing[p.index], want, f'{name} {what}')
        E = r.edge_index.shape[1]
        cap = E + 32
        poff, pmoff = place_flat_int(r.off, I64), place_flat_int(r.moff, I64)
        prow, pcol = place_flat_int((cap,), I64), place_flat_int((cap,), I64)
        rc = lib.ampconv_sbm_fill(*head, poff.ptr, None if c[2] else pmoff.ptr, r.e_upper, prow.ptr, pcol.ptr, cap, stream())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        own = slice(0, E)
        for p, want, what in ((prow, r.edge_index[0], 'row'), (pcol, r.edge_index[1], 'col')):
            if not p.outside_intact(own):
                failed.append(f'{name} {what}: written outside [0, E)')
            if p.unwritten(own):
                failed.append(f'{name} {what}: {p.unwritten(own)} of the E positions not written')
            failed += differs(p.backing[p.index[own]], want, f'{name} {what}')
    assert not failed, failed[:10]


def test_refusals(lib):
    """AMPCONV_E_BADARG, nothing written: a null pointer in every place that needs one, K <= 0, K > 256, a negative size."""
    s = np.asarray([5, 7], np.int64)
    P_d, lq_d = tables(sr.uniform(2, 0.3))
    pc, pm, prow, pcol = (place_flat_int((64,), I64) for _ in range(4))
    poff = place_flat_int(np.zeros(24, np.int64), I64)
    st = stream()

    def count(sizes=s.ctypes.data, K=2, P=P_d.data_ptr(), lq=lq_d.data_ptr(), cnt=pc.ptr, mcnt=pm.ptr):
        return lib.ampconv_sbm_count(sizes, K, P, lq, 0, 0, 0, cnt, mcnt, st)

    def fill(sizes=s.ctypes.data, K=2, P=P_d.data_ptr(), lq=lq_d.data_ptr(), off=poff.ptr, moff=poff.ptr, row=prow.ptr,
             col=pcol.ptr, E=64, base=0):
        return lib.ampconv_sbm_fill(sizes, K, P, lq, 0, 0, 0, off, moff, base, row, col, E, st)
    neg = np.asarray([5, -1], np.int64)
    many = np.ones(257, np.int64)
    got = {'count sizes': count(sizes=None), 'count P': count(P=None), 'count lq': count(lq=None), 'count out': count(cnt=None),
           'count K=0': count(K=0), 'count K=-1': count(K=-1), 'count K=257': count(sizes=many.ctypes.data, K=257),
           'count negative size': count(sizes=neg.ctypes.data),
           'fill sizes': fill(sizes=None), 'fill P': fill(P=None), 'fill lq': fill(lq=None), 'fill off': fill(off=None),
           'fill row': fill(row=None), 'fill col': fill(col=None), 'fill K=0': fill(K=0), 'fill K=257': fill(sizes=many.ctypes.data, K=257),
           'fill negative size': fill(sizes=neg.ctypes.data), 'fill E<0': fill(E=-1), 'fill base<0': fill(base=-1)}
    torch.cuda.synchronize()
    assert all(rc == BADARG for rc in got.values()), got
    assert all(p.outside_intact() and p.unwritten() == 64 for p in (pc, pm, prow, pcol))
    assert count(mcnt=None) == 0 and fill(moff=None, E=0) == 0          # the optional ones
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ reproducibility
def test_two_runs_give_the_same_bits_and_another_seed_other_bits(lib):
    from ampnet_amd import stochastic_block_model
    P = sr.in_out(4, 0.8, 0.05)
    a = stochastic_block_model([64, 65, 63, 1], P, seed=3, device=DEV)
    b = stochastic_block_model([64, 65, 63, 1], P, seed=3, device=DEV)
    c = stochastic_block_model([64, 65, 63, 1], P, seed=4, device=DEV)
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.block, b.block)
    assert a.edge_index.shape != c.edge_index.shape or not torch.equal(a.edge_index, c.edge_index)


def test_no_edge_gives_an_empty_edge_index(lib):
    from ampnet_amd import gnp_random_graph, stochastic_block_model
    for g in (gnp_random_graph(100, 0.0, device=DEV), gnp_random_graph(1, 1.0, device=DEV), gnp_random_graph(0, 0.5, device=DEV),
              stochastic_block_model([0, 0], [[1.0, 1.0], [1.0, 1.0]], device=DEV)):
        assert g.edge_index.dtype == I64 and tuple(g.edge_index.shape) == (2, 0) and g.edge_index.is_cuda
        assert g.block.dtype == I64 and g.block.numel() == g.num_nodes


def test_too_many_edges_raise_before_anything_is_filled(lib, monkeypatch):
    """sizes [70000], p = 1, directed: 4.9e9 edges, counted in closed form; ValueError, and fill is never called."""
    from ampnet_amd import gnp_random_graph

    def no_fill(*a):
        raise AssertionError('ampconv_sbm_fill was called')
    monkeypatch.setattr(lib, 'ampconv_sbm_fill', no_fill)
    with pytest.raises(ValueError, match='2\\^31'):
        gnp_random_graph(70000, 1.0, directed=True, device=DEV)
    with pytest.raises(ValueError, match='2\\^31'):
        gnp_random_graph(70000, 1.0, directed=False, device=DEV)        # 2.45e9 pairs and as many mirrors


# ------------------------------------------------------------------------------------------------------------ XOR link data
def test_xor_link_dataset(lib):
    from ampnet_amd import stochastic_block_model, xor_link_dataset
    from ampnet_amd.random_graphs import xor_link_matrix
    n, std = 400, 0.1
    d = xor_link_dataset(n, noise_std=std, same_class_link_prob=0.7, diff_class_link_prob=0.1, seed=3, device=DEV)
    assert d.num_nodes == n and tuple(d.x.shape) == (n, 2) and d.x.dtype == torch.float32 and d.y.dtype == torch.float32
    assert torch.equal(d.y.cpu(), torch.tensor([0., 1., 1., 0.]).repeat_interleave(n // 4))
    corners = torch.tensor([[0., 0.], [0., 1.], [1., 0.], [1., 1.]])
    means = d.x.cpu().double().reshape(4, n // 4, 2).mean(dim=1)
    # the mean of 100 draws of N(corner, 0.1^2): standard error 0.01 per coordinate; 6 of them (1e-8 over the 8 means)
    assert (means - corners).abs().max() <= 6 * std / (n // 4) ** 0.5, means
    g = stochastic_block_model([n // 4] * 4, xor_link_matrix(0.7, 0.1), directed=True, selfloops=False, seed=3, device=DEV)
    assert torch.equal(d.edge_index, g.edge_index)
    r = sr.block_model([n // 4] * 4, xor_link_matrix(0.7, 0.1), True, False, 3)
    assert r.margin >= sr.MARGIN_MIN and np.array_equal(d.edge_index.cpu().numpy(), r.edge_index)
    again = xor_link_dataset(n, noise_std=std, seed=3, device=DEV)
    assert torch.equal(again.x, d.x) and torch.equal(again.edge_index, d.edge_index)
    assert tuple(xor_link_dataset(8, noise_std=0.0, same_class_link_prob=0.0, diff_class_link_prob=0.0, device=DEV).edge_index.shape) == (2, 0)


# ----------------------------------------------------------------------------------------------------------------- plumbing
def test_ampconv_forward_on_a_generated_graph(lib):
    """AMPConv(8, 2), L = 2: the forward on a generated edge_index is bit-equal to the forward on the same edges after a
    round trip through host memory (the generated tensor is an ordinary contiguous int64 [2, E])."""
    from ampnet_amd import AMPConv, random_partition_graph
    torch.manual_seed(0)
    g = random_partition_graph([40, 30, 30], 0.3, 0.02, seed=1, device=DEV)
    layer = AMPConv(8, 2).to(DEV)
    x = torch.randn(g.num_nodes, 2 * 8, device=DEV)
    with torch.no_grad():
        y0 = layer(x, g.edge_index)
        y1 = layer(x, torch.from_numpy(g.edge_index.cpu().numpy().copy()).to(DEV))
    assert g.edge_index.size(1) > 0 and torch.isfinite(y0).all() and y0.abs().sum() > 0
    assert torch.equal(y0, y1)
