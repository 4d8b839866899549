#!/usr/bin/env python
"""Times ampnet_amd.stochastic_block_model (csrc/sbm.hip) beside two baselines of the same distribution: a PyTorch
implementation on the GPU -- row tiles of `torch.rand(tile, N) < P_row` followed by `nonzero` -- and, at 100 000 nodes,
networkx.stochastic_block_model on the host.

    python tools/bench_sbm.py [--rounds 5] [--skip-networkx]

Workloads: undirected graphs of four equal blocks.  1 M and 100 k nodes with about 10 neighbours per node, 80 % of them
inside the node's block (p_in = 8 / (N / 4), p_out = 2 / (3 N / 4)); 4 000 nodes with (p_in, p_out) = (0.8, 0.05).
Method (that of tools/bench_spring.py): 2 warm-up rounds, the median of the timed rounds by device events around work
that ends in a synchronise, the spread max - min; the fused call and the PyTorch route alternate in one process.  The
whole call includes its one read-back (the total, to allocate).  count and fill are then timed alone through the C ABI
on the call's own offsets; fill_bytes_per_s counts the 16 bytes per edge_index column that fill writes.  The PyTorch
route draws N^2 uniforms: at 1 M nodes it is timed on 8 row tiles and scaled to N / tile of them (`torch_extrapolated`).
One JSON line per workload."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ampnet_amd import _lib, stochastic_block_model                          # noqa: E402
from ampnet_amd.graph import _stream                                           # noqa: E402

TILE = 1024


def in_out(K, p_in, p_out):
    return np.where(np.eye(K, dtype=bool), float(p_in), float(p_out))


def timed(fn, rounds, warmup=2):
    ms = []
    for r in range(warmup + rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if r >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), max(ms) - min(ms)


def torch_tiles(sizes, P, dev, tiles=None):
    """The same distribution with library calls: for a tile of rows, rand < P[block(row)][block(col)], the strict upper
    triangle, nonzero; then the mirrors.  tiles: only the first so many (the 1 M extrapolation)."""
    N = int(sum(sizes))
    block = torch.repeat_interleave(torch.arange(len(sizes), device=dev), torch.tensor(sizes, device=dev))
    Pd = torch.from_numpy(P).float().to(dev)
    cols = torch.arange(N, device=dev)
    out = []
    for n, b in enumerate(range(0, N, TILE)):
        if tiles is not None and n >= tiles:
            break
        rows = cols[b:b + TILE]
        hit = (torch.rand(rows.numel(), N, device=dev) < Pd[block[rows]][:, block]) & (cols[None, :] > rows[:, None])
        r, c = hit.nonzero(as_tuple=True)
        out.append(torch.stack((r + b, c)))
    upper = torch.cat(out, dim=1)
    return torch.cat((upper, upper.flip(0)), dim=1)


def bench(N, p_in, p_out, rounds, networkx_too):
    dev = torch.device('cuda:0')
    K = 4
    sizes = [N // K] * K
    P = in_out(K, p_in, p_out)
    g = [None]

    def fused():
        g[0] = stochastic_block_model(sizes, P, seed=0, device=dev)
    extrapolated = N > 200_000
    tiles = 8 if extrapolated else None
    f_ms, t_ms = [], []
    for r in range(2 + rounds):                                             # the routes alternate
        a, b = timed(fused, 1, warmup=0), timed(lambda: torch_tiles(sizes, P, dev, tiles), 1, warmup=0)
        if r >= 2:
            f_ms.append(a[0])
            t_ms.append(b[0] * ((N / TILE) / tiles if extrapolated else 1.0))
    E = int(g[0].edge_index.size(1))

    # the two kernels alone, on the offsets of that call
    lib = _lib.load()
    s = np.asarray(sizes, np.int64)
    with np.errstate(divide='ignore'):
        lq = np.log1p(-P)
    P_d, lq_d = torch.from_numpy(P).to(dev), torch.from_numpy(lq).to(dev)
    head = (s.ctypes.data, K, P_d.data_ptr(), lq_d.data_ptr(), 0, 0, 0)
    counts = torch.empty(1, N * K, dtype=torch.int64, device=dev)
    c_ms, c_spread = timed(lambda: _lib.check(lib.ampconv_sbm_count(*head, counts.data_ptr(), None, _stream()), 'count'), rounds)
    s_ms, s_spread = timed(lambda: torch.cumsum(counts, dim=1), rounds)
    ends = torch.cumsum(counts, dim=1)
    off = ends - counts
    e_upper = int(ends[0, -1])
    ei = torch.empty(2, E, dtype=torch.int64, device=dev)
    fl_ms, fl_spread = timed(lambda: _lib.check(lib.ampconv_sbm_fill(*head, off.data_ptr(), off.data_ptr(), e_upper, ei[0].data_ptr(),
                                                                      ei[1].data_ptr(), E, _stream()), 'fill'), rounds)
    assert torch.equal(ei, g[0].edge_index)
    cp_ms, cp_spread = timed(lambda: ei.clone(), rounds)                   # the same bytes, read and written coalesced
    out = dict(N=N, K=K, p_in=p_in, p_out=p_out, E=E, call_ms=round(statistics.median(f_ms), 4),
               call_spread_ms=round(max(f_ms) - min(f_ms), 4), edges_per_s=round(E / (statistics.median(f_ms) * 1e-3), 0),
               count_ms=round(c_ms, 4), count_spread_ms=round(c_spread, 4), cumsum_ms=round(s_ms, 4), cumsum_spread_ms=round(s_spread, 4),
               fill_ms=round(fl_ms, 4), fill_spread_ms=round(fl_spread, 4), fill_bytes=16 * E,
               fill_bytes_per_s=round(16 * E / (fl_ms * 1e-3), 0), fill_minus_count_ms=round(fl_ms - c_ms, 4),
               clone_edge_index_ms=round(cp_ms, 4), clone_spread_ms=round(cp_spread, 4),
               torch_ms=round(statistics.median(t_ms), 3), torch_spread_ms=round(max(t_ms) - min(t_ms), 3),
               torch_extrapolated=extrapolated, speedup_over_torch=round(statistics.median(t_ms) / statistics.median(f_ms), 1))
    if networkx_too:
        import networkx as nx
        t0 = time.perf_counter()
        G = nx.stochastic_block_model(sizes, P.tolist(), seed=0)
        out.update(networkx_s=round(time.perf_counter() - t0, 2), networkx_E=2 * G.number_of_edges())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-networkx', action='store_true')
    args = ap.parse_args()
    for N, p_in, p_out in ((1_000_000, 8 / 250_000, 2 / 750_000), (100_000, 8 / 25_000, 2 / 75_000), (4_000, 0.8, 0.05)):
        bench(N, p_in, p_out, args.rounds, networkx_too=N == 100_000 and not args.skip_networkx)


if __name__ == '__main__':
    main()
