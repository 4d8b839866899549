#!/usr/bin/env python
"""Times one iteration of ampnet_amd.spring (ampconv_spring_repulsion + ampconv_spring_step) beside the composite a user
writes in torch -- the same arithmetic, the N x N term in row chunks of 4096 so that it fits --, and, in the same
process, ampconv_tsne_repulsion on the same points: the two N-body kernels side by side.

    python tools/bench_spring.py [N ...] [--rounds 5] [--degree 10] [--dim 2]

Without a size: 10 000 and 96 000 nodes (one GraphSAINT batch), a random graph of average degree 10, uniform positions.
Method (that of tools/bench_tsne.py): the routes alternate in one process, 2 warm-up rounds, the median of the timed
rounds by device events, the spread max - min; a round is 5 iterations of the fused route and 1 of the composite.  The
threshold is negative, so the stopping rule never latches and every iteration does its work.  One JSON line per size."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ampnet_amd                                                              # noqa: E402,F401
S = sys.modules['ampnet_amd.spring']
T = sys.modules['ampnet_amd.tsne']

CHUNK = 4096


def random_graph(N, degree, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, N, (2, N * degree // 2), generator=g)


def composite_step(y, rows, indices, val, k, t):
    N = y.size(0)
    rep = torch.empty(N, y.size(1), dtype=torch.float64, device=y.device)
    for b in range(0, N, CHUNK):
        d = y[b:b + CHUNK, None, :] - y[None, :, :]
        q = 1.0 / (d * d).sum(2).clamp_(min=1e-4)
        rep[b:b + CHUNK] = (q[:, :, None] * d).sum(1)                       # float32 sums: the composite's fastest form
    d = y[rows] - y[indices]
    w = val * (d * d).sum(1).sqrt().clamp_(min=0.01)
    att = torch.zeros_like(rep).index_add_(0, rows, (w[:, None] * d).double())
    disp = k * k * rep - att / k
    length = disp.norm(dim=1)
    length = torch.where(length < 0.01, torch.full_like(length, 0.1), length)
    delta = (disp * (t / length)[:, None]).float()
    done = delta.double().pow(2).sum().sqrt() / N < -1.0                   # computed as the kernels compute it, never true
    return y + delta, done


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def bench(N, degree, dim, rounds):
    ei = random_graph(N, degree).cuda()
    indptr, indices, val = S.adjacency(ei, N)
    y0 = S.uniform_start(N, dim, 0, ei.device)
    k = 1.0 / math.sqrt(N)
    state = None

    def make():
        nonlocal state
        state = S.SpringLayout(y0, indptr, indices, val, k, 1 << 20, threshold=-1.0)
    fused_mem = peak(make)
    iters = 5

    def fused():
        for _ in range(iters):
            state.step()
    rows = torch.arange(N, device=ei.device).repeat_interleave(indptr[1:] - indptr[:-1])
    cs = [y0.clone()]

    def comp():
        cs[0], _ = composite_step(cs[0], rows, indices, val, k, 0.1)
    comp_mem = peak(comp)
    f_ms, c_ms = [], []
    for r in range(2 + rounds):                                             # the routes alternate
        a, b = timed(fused, 1, warmup=0), timed(comp, 1, warmup=0)
        if r >= 2:
            f_ms.append(a[0] / iters)
            c_ms.append(b[0])
    rep_ms, rep_spread = timed(state.repulsion, rounds)
    out = dict(N=N, dim=dim, nnz=int(indices.numel()),
               fused_iteration_ms=round(statistics.median(f_ms), 4), fused_spread_ms=round(max(f_ms) - min(f_ms), 4),
               composite_iteration_ms=round(statistics.median(c_ms), 4), composite_spread_ms=round(max(c_ms) - min(c_ms), 4),
               speedup=round(statistics.median(c_ms) / statistics.median(f_ms), 2),
               spring_repulsion_ms=round(rep_ms, 4), spring_repulsion_spread_ms=round(rep_spread, 4),
               pairs_per_s=round(N * N / (rep_ms * 1e-3), 0), fused_state_bytes=int(fused_mem), composite_peak_bytes=int(comp_mem))
    if dim == 2:                                                            # t-SNE's N-body kernel on the same points, same process
        lib = state.lib
        neg, Z = torch.empty(N, 2, device=ei.device), torch.empty(1, dtype=torch.float64, device=ei.device)
        ws = torch.empty(max(int(lib.ampconv_tsne_repulsion_workspace_bytes(N)), 256), dtype=torch.uint8, device=ei.device)
        t_ms, t_spread = timed(lambda: T._lib.check(lib.ampconv_tsne_repulsion(
            y0.data_ptr(), N, neg.data_ptr(), Z.data_ptr(), ws.data_ptr(), ws.numel(), T._stream()), 'ampconv_tsne_repulsion'), rounds)
        out.update(tsne_repulsion_ms=round(t_ms, 4), tsne_repulsion_spread_ms=round(t_spread, 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('sizes', nargs='*', type=int)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--degree', type=int, default=10)
    ap.add_argument('--dim', type=int, default=2, choices=(2, 3))
    args = ap.parse_args()
    for N in args.sizes or (10_000, 96_000):
        bench(N, args.degree, args.dim, args.rounds)


if __name__ == '__main__':
    main()
