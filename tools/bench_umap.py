#!/usr/bin/env python
"""Measures ampnet_amd.umap: the error of the epoch kernel's two coefficients against fp64, the one-time stages
(neighbours, memberships, fuzzy union) and one epoch of the layout at a few sizes.

    python tools/bench_umap.py [M ...] [--rounds 5] [--dims 2 30] [--coefficients-only]

Coefficients: ampconv_umap_coefficients evaluates the kernel's own attract / repel functions on 2^20 values of d2 spread
log-uniformly over [1e-12, 1e4]; the reference is numpy fp64 at the same float32 (a, b) and the same float32 d2, for the
default curve and for (spread, min_dist) = (1, 0.5) and (2, 0.01); printed: the largest relative error of each.  The
largest over the DEFAULT curve is R_COEFF of tests/umap_reference.py (the epoch test's margin is 4 x it).

Times (method of tools/bench_knn.py): 2 warm-up rounds, the median of the timed rounds by device events, the spread
max - min; a round of the epoch timing is 20 consecutive epochs from epoch n_epochs / 4 on (every epoch fires a
different share of the entries), reported per epoch, with the launches per epoch.  Without a size: 10 000 and 96 000
points, 16 features in 8 Gaussian blobs.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ampnet_amd                                                              # noqa: E402,F401
U = sys.modules['ampnet_amd.umap']


def data(N, D=16, centers=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(centers, D, generator=g) * 4
    return c[torch.randint(0, centers, (N,), generator=g)] + torch.randn(N, D, generator=g)


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


def coefficients():
    lib = U._lib.load()
    n = 1 << 20
    d2 = torch.logspace(-12, 4, n, dtype=torch.float64).float().cuda()
    att, rep = torch.empty_like(d2), torch.empty_like(d2)
    x = d2.cpu().numpy().astype(np.float64)
    for spread, min_dist in ((1.0, 0.1), (1.0, 0.5), (2.0, 0.01)):
        a, b = U.find_ab_params(spread, min_dist)
        U._lib.check(lib.ampconv_umap_coefficients(d2.data_ptr(), n, a, b, 1.0, att.data_ptr(), rep.data_ptr(), U._stream()),
                     'ampconv_umap_coefficients')
        torch.cuda.synchronize()
        a32, b32 = float(np.float32(a)), float(np.float32(b))
        want_att = -2.0 * a32 * b32 * x ** (b32 - 1.0) / (a32 * x ** b32 + 1.0)
        want_rep = 2.0 * b32 / ((0.001 + x) * (a32 * x ** b32 + 1.0))
        ea = np.abs(att.cpu().numpy().astype(np.float64) - want_att) / np.abs(want_att)
        er = np.abs(rep.cpu().numpy().astype(np.float64) - want_rep) / np.abs(want_rep)
        print(json.dumps(dict(coefficients=dict(spread=spread, min_dist=min_dist, a=a, b=b), attract_rel_err=float(ea.max()),
                              attract_at_d2=float(x[ea.argmax()]), repel_rel_err=float(er.max()), repel_at_d2=float(x[er.argmax()]),
                              r=float(max(ea.max(), er.max())))), flush=True)


def bench(M, dims, rounds):
    x = data(M).cuda()
    k = 15

    def stage():
        idx, dist = U.neighbors_with_self(x, k)
        memb, sigma, rho = U.memberships(idx, dist)
        return U.fuzzy_graph(idx, memb)

    idx, dist = U.neighbors_with_self(x, k)
    memb, _, _ = U.memberships(idx, dist)
    nb_ms, _ = timed(lambda: U.neighbors_with_self(x, k), rounds, warmup=1)
    mb_ms, mb_sp = timed(lambda: U.memberships(idx, dist), rounds, warmup=1)
    fz_ms, fz_sp = timed(lambda: U.fuzzy_graph(idx, memb), rounds, warmup=1)
    indptr, indices, val = stage()
    n_epochs = 500 if M <= 10000 else 200
    a, b = U.find_ab_params()
    sched = U.schedule(indptr, indices, val, n_epochs)
    print(json.dumps(dict(M=M, n_neighbors=k, nnz=int(indices.numel()), sampled_nnz=int(sched[1].numel()), n_epochs=n_epochs,
                          longest_row=int((indptr[1:] - indptr[:-1]).max()), neighbours_ms=round(nb_ms, 3),
                          memberships_ms=round(mb_ms, 4), memberships_spread_ms=round(mb_sp, 4), fuzzy_union_ms=round(fz_ms, 3),
                          fuzzy_union_spread_ms=round(fz_sp, 3))), flush=True)
    for dim in dims:
        y0 = U.scaled_start(torch.randn(M, dim, generator=torch.Generator().manual_seed(1)).cuda())
        state = U.Layout(y0, *sched, a, b, n_epochs, 0)
        at = [n_epochs // 4]

        def epochs():
            for _ in range(20):
                state.epoch(at[0] % n_epochs)
                at[0] += 1
        ms, sp = timed(epochs, rounds)
        launches = 1 + int(sched[1].numel() > U.PART)
        print(json.dumps(dict(M=M, dim=dim, epoch_ms=round(ms / 20, 5), epoch_spread_ms=round(sp / 20, 5), launches_per_epoch=launches,
                              entries_per_s=round(int(sched[1].numel()) / (ms / 20 * 1e-3), 0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('sizes', nargs='*', type=int)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dims', nargs='*', type=int, default=[2, 30])
    ap.add_argument('--coefficients-only', action='store_true')
    args = ap.parse_args()
    coefficients()
    if args.coefficients_only:
        return
    for M in args.sizes or (10_000, 96_000):
        bench(M, args.dims, args.rounds)


if __name__ == '__main__':
    main()
