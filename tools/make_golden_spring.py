#!/usr/bin/env python3
"""tests/golden/spring/*.npz: small graphs, a seeded start and what networkx's spring_layout returns for them, for
tests/test_spring_cpu.py and tests/test_gpu_spring.py.

TEST INFRASTRUCTURE; runs on the CPU where networkx is installed (written with 3.4.2).  Per fixture:

    num_nodes, symmetric   the node count; whether the graph is undirected (a Graph) or a DiGraph
    edge_index             int32 [2, E]: every edge of the Graph once (either direction), every arc of the DiGraph
    a_indptr, a_indices,   the CSR of the matrix networkx lays out, nx.to_scipy_sparse_array(G, dtype='f'): what
    a_val                  ampnet_amd.spring.adjacency has to produce from edge_index
    pos0                   the start, float32 (uniform [0, 1), so float32 and float64 hold the same values)
    pos_1, pos_5, pos_50   nx.spring_layout(G, pos=pos0, iterations=n, scale=None): three separate runs, dt depends on
                           the iteration count.  float64 on networkx's dense path (N < 500), float32 on its sparse one
    pos_default            nx.spring_layout(G, pos=pos0): 50 iterations, rescaled to scale 1 around the origin

The cases are tests/spring_reference.CASES:

    sbm64            4 blocks of 16, p_in 0.5, p_out 0.02: a clustered layout
    grid8            the 8 x 8 grid
    cycle33          a cycle of odd length
    path2            2 nodes, 1 edge: networkx stops after 43 of 50 iterations
    sbm512           4 blocks of 128, p_in 0.1, p_out 0.005: N >= 500, networkx's sparse path with float32 positions
    xor_digraph_40   the directed 5-nearest-neighbour graph of 40 duplicated-XOR points, the point itself included
                     (self-loops), as the reference's synthetic XOR benchmark builds it

    python tools/make_golden_spring.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def sbm(nx, sizes, p_in, p_out, seed):
    p = [[p_in if a == b else p_out for b in range(len(sizes))] for a in range(len(sizes))]
    G = nx.stochastic_block_model(sizes, p, seed=seed)
    H = nx.Graph()
    H.add_nodes_from(range(sum(sizes)))
    H.add_edges_from(G.edges())
    return H


def xor_digraph(nx, n, neighbors, noise, seed):
    rng = np.random.default_rng(seed)
    x = np.repeat(np.array([[0., 0.], [0., 1.], [1., 0.], [1., 1.]]), n // 4, axis=0)
    x = x + rng.normal(0.0, noise, x.shape)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind='stable')[:, :neighbors + 1]          # the point itself first: a self-loop
    adj = np.zeros((n, n), np.uint8)
    adj[np.arange(n)[:, None], idx] = 1
    return nx.from_numpy_array(adj, create_using=nx.DiGraph)


def main():
    import networkx as nx
    import spring_reference as sr
    os.makedirs(sr.GOLDEN_DIR, exist_ok=True)
    graphs = {
        'sbm64': sbm(nx, [16] * 4, 0.5, 0.02, 1),
        'grid8': nx.convert_node_labels_to_integers(nx.grid_2d_graph(8, 8), ordering='sorted'),
        'cycle33': nx.cycle_graph(33),
        'path2': nx.path_graph(2),
        'sbm512': sbm(nx, [128] * 4, 0.1, 0.005, 2),
        'xor_digraph_40': xor_digraph(nx, 40, 5, 0.1, 3),
    }
    for seed, name in enumerate(sr.CASES):
        G = graphs[name]
        N = G.number_of_nodes()
        assert list(G.nodes()) == list(range(N))
        # path2: a start from which networkx stops after 43 of 50 iterations, found by trying seeds
        pos0 = np.random.default_rng(149 if name == 'path2' else 100 + seed).random((N, 2), dtype=np.float32)
        start = {i: pos0[i].astype(np.float64) for i in range(N)}
        A = nx.to_scipy_sparse_array(G, dtype='f').tocsr()
        A.sort_indices()
        out = dict(num_nodes=np.int64(N), symmetric=np.bool_(not G.is_directed()), edge_index=np.array(list(G.edges()), np.int32).T.reshape(2, -1),
                   a_indptr=A.indptr.astype(np.int32), a_indices=A.indices.astype(np.int32), a_val=A.data.astype(np.float32), pos0=pos0)
        for n in sr.ITERATIONS:
            p = nx.spring_layout(G, pos=dict(start), iterations=n, scale=None, seed=0)
            out[f'pos_{n}'] = np.stack([p[i] for i in range(N)])
        p = nx.spring_layout(G, pos=dict(start), seed=0)
        out['pos_default'] = np.stack([p[i] for i in range(N)])
        path = os.path.join(sr.GOLDEN_DIR, name + '.npz')
        np.savez_compressed(path, **out)
        print(f'{name}: N {N}, {out["edge_index"].shape[1]} edges, positions {out["pos_50"].dtype}, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
