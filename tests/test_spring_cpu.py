"""The models of tests/spring_reference.py held to networkx's recorded values on the CPU, and the host side of
ampnet_amd.spring (the adjacency, the argument checks, the boundary).  The fixtures under tests/golden/spring were
recorded from networkx 3.4.2 (tools/make_golden_spring.py); where networkx is installed the fp64 model is also checked
live on a fresh graph."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import spring_reference as sr
from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'ampconv.h')


@pytest.fixture(scope='module')
def fixtures():
    return {name: sr.load(name) for name in sr.CASES}


def graph_of(f):
    return sr.adjacency_model(f['edge_index'], f['N'], None, f['symmetric'])


# ------------------------------------------------------------------------------------------------ networkx's own loop
def test_fp64_model_equals_the_dense_path_fixtures_exactly(fixtures):
    for name in sr.DENSE_CASES:
        f = fixtures[name]
        A = sr.dense(*graph_of(f), f['N'])
        assert f['pos_50'].dtype == np.float64
        for n in sr.ITERATIONS:
            pos, _ = sr.fr_model(A, f['pos0'], iterations=n)
            assert np.array_equal(pos, f[f'pos_{n}']), (name, n, np.abs(pos - f[f'pos_{n}']).max())
        pos, _ = sr.fr_model(A, f['pos0'])
        assert np.array_equal(sr.rescale_model(pos), f['pos_default']), name


def test_path2_stops_after_43_iterations(fixtures):
    f = fixtures['path2']
    graph = graph_of(f)
    pos, ran = sr.fr_model(sr.dense(*graph, 2), f['pos0'])
    assert ran == 43 and np.array_equal(pos, f['pos_50'])
    assert sr.fr_model(sr.dense(*graph, 2), f['pos0'], threshold=-1.0)[1] == 50      # it is the rule that stops it
    y32, ran32 = sr.fr_model(sr.dense(*graph, 2), f['pos0'], dtype=np.float32)
    assert ran32 == 43 and np.abs(y32 - f['pos_50']).max() < 1e-6
    y, ran_header = sr.layout_model(f['pos0'], *graph)
    assert ran_header == 43 and np.abs(y - f['pos_50']).max() < 1e-6


def test_fp64_model_against_networkx_live():
    nx = pytest.importorskip('networkx')
    seed = int.from_bytes(os.urandom(4), 'little')                    # a fresh graph every run; the seed reproduces it
    rng = np.random.default_rng(seed)
    N = int(rng.integers(20, 120))
    G = nx.gnp_random_graph(N, float(rng.uniform(0.02, 0.3)), seed=int(rng.integers(1 << 30)))
    case = f'seed {seed}: {N} nodes, {G.number_of_edges()} edges'
    print(case)
    pos0 = rng.random((N, 2), dtype=np.float32)
    edges = np.array(list(G.edges()), np.int64).T.reshape(2, -1)
    A = sr.dense(*sr.adjacency_model(edges, N), N)
    assert np.array_equal(A, nx.to_numpy_array(G)), case
    for n in (1, 7, 50):
        want = nx.spring_layout(G, pos={i: pos0[i].astype(np.float64) for i in range(N)}, iterations=n, scale=None, seed=0)
        got, _ = sr.fr_model(A, pos0, iterations=n)
        assert np.array_equal(got, np.stack([want[i] for i in range(N)])), f'{case}, {n} iterations'
    want = nx.spring_layout(G, pos={i: pos0[i].astype(np.float64) for i in range(N)}, scale=2.5, center=(1.0, -3.0), seed=0)
    got = sr.rescale_model(sr.fr_model(A, pos0)[0], 2.5, (1.0, -3.0))
    assert np.array_equal(got, np.stack([want[i] for i in range(N)])), f'{case}, rescaled'


def test_header_model_follows_the_fixtures(fixtures):
    """The header's iteration (float32 positions, fp64 sums) against networkx's values: at 1 and 5 iterations within 4 x
    the float32-arithmetic model's own deviation (floor 1e-6) -- the bar the kernels are held to -- and after the
    default run the layout has pulled the edges together: the quality figure of the GPU tests, on the model first."""
    for name in sr.CASES:
        f = fixtures[name]
        graph = graph_of(f)
        A = sr.dense(*graph, f['N'])
        for n in (1, 5):
            want = f[f'pos_{n}'].astype(np.float64)
            bar = max(4.0 * np.abs(sr.fr_model(A, f['pos0'], iterations=n, dtype=np.float32)[0] - want).max(), 1e-6)
            got, _ = sr.layout_model(f['pos0'], *graph, iterations=n)
            dev = np.abs(got - want).max()
            print(f'{name} n={n}: header model deviates {dev:.3e}, bar {bar:.3e}')
            assert dev <= bar, (name, n)
        if name != 'path2':
            y, _ = sr.layout_model(f['pos0'], *graph)
            start, end = sr.edge_ratio(f['pos0'], f['edge_index']), sr.edge_ratio(sr.rescale_model(y), f['edge_index'])
            theirs = sr.edge_ratio(f['pos_default'], f['edge_index'])
            print(f'{name}: edge / non-edge distance {start:.3f} -> {end:.3f} (networkx {theirs:.3f})')
            assert end < 0.6 * start and theirs < 0.6 * start


# ------------------------------------------------------------------------------------------------------ the adjacency
def test_adjacency_model_and_package_against_the_fixtures_matrices(fixtures):
    spring = importlib.import_module('ampnet_amd.spring')
    for name in sr.CASES:
        f = fixtures[name]
        want = (f['a_indptr'], f['a_indices'], f['a_val'])
        for got in (graph_of(f), [t.numpy() for t in spring.adjacency(torch.as_tensor(f['edge_index']), f['N'], None, f['symmetric'])]):
            assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        assert got[0].dtype == np.int64 and got[1].dtype == np.int64 and got[2].dtype == np.float32
    f = fixtures['xor_digraph_40']
    assert (f['edge_index'][0] == f['edge_index'][1]).sum() == 40                # the self-loops are kept
    sym = sr.adjacency_model(f['edge_index'], 40, None, True)
    assert sym[1].size > f['a_indices'].size and np.array_equal(sr.dense(*sym, 40), sr.dense(*sym, 40).T)


def test_adjacency_duplicates_weights_and_empty_graphs():
    spring = importlib.import_module('ampnet_amd.spring')
    rng = np.random.default_rng(5)
    N, E = 30, 400                                                    # 400 arcs on 900 pairs: many duplicates
    ei = rng.integers(0, N, (2, E))
    w = rng.random(E).astype(np.float32)
    for weight, symmetric in ((None, True), (None, False), (w, False)):
        want = sr.adjacency_model(ei, N, weight, symmetric)
        got = spring.adjacency(torch.as_tensor(ei), N, None if weight is None else torch.as_tensor(weight), symmetric)
        assert all(np.array_equal(g.numpy(), x) for g, x in zip(got, want)), symmetric
        assert all((np.diff(want[1][want[0][i]:want[0][i + 1]]) > 0).all() for i in range(N))
    A = np.zeros((N, N))
    np.add.at(A, (ei[0], ei[1]), w.astype(np.float64))
    assert np.allclose(sr.dense(*want, N), A, rtol=1e-6, atol=0) and want[1].size < E
    empty = spring.adjacency(torch.zeros(2, 0, dtype=torch.int64), 7)
    assert empty[0].tolist() == [0] * 8 and empty[1].numel() == 0 and empty[2].numel() == 0


# ----------------------------------------------------------------------------------------------------------- the start
def test_start_stream_against_its_integer_model():
    import pipeline_reference as pr
    for seed in (0, 1, 2 ** 63 + 12345, -7):
        y = sr.uniform_start_model(50, 3, seed)
        i, c = np.meshgrid(np.arange(50), np.arange(3), indexing='ij')
        raw = pr.draw(seed, i, c)                                     # the sampler's stream, an independent statement of it
        assert np.array_equal(y, ((raw >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(np.float32))
        assert y.dtype == np.float32 and (y >= 0).all() and (y < 1).all()
        assert np.array_equal(y.astype(np.float64) * 2.0 ** 24, np.round(y.astype(np.float64) * 2.0 ** 24))
    a, b = sr.uniform_start_model(4000, 2, 0), sr.uniform_start_model(4000, 2, 1)
    assert not np.array_equal(a, b) and abs(a.mean() - 0.5) < 0.02 and abs(a.var() - 1.0 / 12) < 0.01
    t0, dt = sr.temperature_model(np.array([[0.25, 0.5, 9.0], [0.75, 0.25, -9.0]], np.float32), 9)
    assert t0 == 0.1 * 0.5 and dt == t0 / 10                          # the first two columns only


# ---------------------------------------------------------------------------------------------------------- validation
def test_arguments_are_checked_before_anything_runs():
    from ampnet_amd import spring_layout
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])
    with pytest.raises(ValueError, match='GPU'):
        spring_layout(ei, 5)
    pos = torch.zeros(5, 2)
    for kw in (dict(dim=1), dict(dim=4), dict(dim=2.0), dict(k=0.0), dict(k=-1.0), dict(k='x'), dict(k=float('nan')), dict(iterations=-1),
               dict(iterations=2.5), dict(iterations=True), dict(threshold='x'), dict(threshold=float('nan')), dict(scale='big'),
               dict(scale=float('inf')), dict(center=(0.0,)), dict(center=(0.0, 0.0, 0.0)), dict(center=1.0), dict(center=('a', 'b')),
               dict(seed=1.5), dict(seed='x'), dict(symmetric=1), dict(weight=torch.ones(3)), dict(weight=torch.ones(2), symmetric=False),
               dict(weight=torch.ones(3, dtype=torch.int64), symmetric=False), dict(weight=[1.0, 1.0, 1.0], symmetric=False),
               dict(weight=torch.ones(3, requires_grad=True), symmetric=False), dict(pos=torch.zeros(5, 3)), dict(pos=torch.zeros(4, 2)),
               dict(pos=pos.double()), dict(pos=[[0.0, 0.0]] * 5), dict(pos=torch.zeros(5, 2, requires_grad=True)),
               dict(fixed=torch.tensor([0])), dict(pos=pos, fixed=[0]), dict(pos=pos, fixed=torch.tensor([0.0])),
               dict(pos=pos, fixed=torch.zeros(4, dtype=torch.bool)), dict(pos=pos, fixed=torch.zeros(1, 1, dtype=torch.int64))):
        with pytest.raises(ValueError):
            spring_layout(ei, 5, **kw)
    for bad_ei, n in ((ei.int(), 5), (ei[0], 5), (ei.t(), 5), (ei.tolist(), 5), (ei, -1), (ei, 2.0), (ei, True), (ei, (1 << 24) + 1), (ei, 0)):
        with pytest.raises(ValueError):
            spring_layout(bad_ei, n)
    with pytest.raises(ValueError, match='fixed without positions'):
        spring_layout(ei, 5, fixed=torch.tensor([1]))


# ------------------------------------------------------------------------------------------------------- the boundary
def test_header_constants_and_symbols():
    import __graft_entry__ as ge
    from ampnet_amd import _lib
    ge.build()
    text = open(HEADER).read()
    consts = dict(re.findall(r'#define\s+AMPCONV_SPRING_(\w+)\s+(.+)', text))
    assert sorted(consts) == ['CHUNK', 'MAX_N', 'PART', 'RUN', 'TILE']
    for name, value in consts.items():
        assert eval(value.strip(), {}) == getattr(_lib, 'SPRING_' + name), name
    assert (sr.RUN, sr.PART) == (_lib.SPRING_RUN, _lib.SPRING_PART)
    spring = importlib.import_module('ampnet_amd.spring')
    assert (spring.MAX_N, spring.PART) == (_lib.SPRING_MAX_N, _lib.SPRING_PART)
    code = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = sorted(set(re.findall(r'\b(ampconv_spring_[a-z_0-9]+)\s*\(', code)))
    assert declared == ['ampconv_spring_repulsion', 'ampconv_spring_repulsion_workspace_bytes', 'ampconv_spring_start',
                        'ampconv_spring_step', 'ampconv_spring_step_split', 'ampconv_spring_step_workspace_bytes']
    lib = ctypes.CDLL(os.path.join(ROOT, 'ampnet_amd', 'libampconv.so'))
    for name in declared:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    # the workspace sizes answer without a device: 0 for what the kernels do not take
    lib = _lib.load()
    assert lib.ampconv_spring_repulsion_workspace_bytes(0, 2) == 0 == lib.ampconv_spring_repulsion_workspace_bytes(5, 4)
    assert lib.ampconv_spring_step_workspace_bytes(5, -1, 2) == 0 == lib.ampconv_spring_step_workspace_bytes((1 << 24) + 1, 0, 2)
    assert lib.ampconv_spring_repulsion_workspace_bytes(96000, 2) == 24 * 2 * 96000 * 8
    assert lib.ampconv_spring_step_workspace_bytes(10, 640, 3) >= (10 + 10 + 1) * 3 * 4 + 10 * 8
    import ampnet_amd
    assert ampnet_amd.spring_layout is spring.spring_layout and ampnet_amd.SpringResult is spring.SpringResult
    assert ampnet_amd.SpringLayout is spring.SpringLayout
