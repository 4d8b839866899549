#!/usr/bin/env python
"""Times one t-SNE iteration of ampnet_amd.tsne (ampconv_tsne_repulsion + ampconv_tsne_step) beside the composite a user
writes in torch -- the same arithmetic, the N x N term in row chunks of 4096 so that it fits --, the one-time affinity
stage (neighbours, perplexity search, joint probabilities), and the peak memory of both routes.

    python tools/bench_tsne.py [N ...] [--rounds 5] [--perplexity 10] [--sklearn N]

Without a size: 10 000 and 96 000 points (one GraphSAINT batch of embeddings), 16 features in 8 Gaussian blobs, the
embedding at scale 10.  Method (that of tools/bench_knn.py): the routes alternate in one process, 2 warm-up rounds, the
median of the timed rounds by device events, the spread max - min; a round is 5 iterations of the fused route and 1 of
the composite.  --sklearn N adds, for context only, scikit-learn's Barnes-Hut TSNE (angle 0.5, its default) on the host
threads at N points, 250 + 50 iterations, reported per iteration.  One JSON line per size."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ampnet_amd                                                              # noqa: E402,F401
T = sys.modules['ampnet_amd.tsne']

CHUNK = 4096


def data(N, D=16, centers=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(centers, D, generator=g) * 4
    return c[torch.randint(0, centers, (N,), generator=g)] + torch.randn(N, D, generator=g)


def composite_step(y, update, gains, indptr, indices, val, rows, exag, mom, lr):
    N = y.size(0)
    neg = torch.empty_like(y)
    Z = torch.zeros((), dtype=torch.float64, device=y.device)
    ar = torch.arange(N, device=y.device)
    for b in range(0, N, CHUNK):
        d = y[b:b + CHUNK, None, :] - y[None, :, :]
        q = 1.0 / (1.0 + (d * d).sum(2))
        q[ar[b:b + CHUNK] - b, ar[b:b + CHUNK]] = 0
        Z += q.sum(dtype=torch.float64)
        neg[b:b + CHUNK] = ((q * q)[:, :, None] * d).sum(1)
    d = y[rows] - y[indices]
    w = (exag * val) / (1.0 + (d * d).sum(1))
    pos = torch.zeros_like(y).index_add_(0, rows, w[:, None] * d)
    grad = 4.0 * (pos - (neg.double() / Z.clamp(min=2.0 ** -52)).float())
    gains = torch.where(update * grad < 0, gains + 0.2, gains * 0.8).clamp_(min=0.01)
    update = mom * update - lr * (grad * gains)
    return y + update, update, gains


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


def bench(N, perplexity, rounds):
    x = data(N).cuda()
    k = min(N - 1, int(3.0 * perplexity + 1))

    def stage():
        idx, d2 = T.nearest(x, k)
        cond, beta = T.affinities(d2, perplexity)
        return T.joint_probabilities(idx, cond)

    aff_ms, aff_spread = timed(stage, max(2, rounds // 2), warmup=1)
    indptr, indices, val = stage()
    y0 = (torch.randn(N, 2, generator=torch.Generator().manual_seed(1)) * 10).cuda()
    lr = max(N / 12.0 / 4.0, 50.0)
    state = None

    def make():
        nonlocal state
        state = T.Descent(y0, indptr, indices, val)
    fused_mem = peak(make)
    iters = 5

    def fused():
        for _ in range(iters):
            state.step(1.0, 0.8, lr, False)
    rows = torch.arange(N, device=x.device).repeat_interleave(indptr[1:] - indptr[:-1])
    cs = [y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)]

    def comp():
        cs[0], cs[1], cs[2] = composite_step(cs[0], cs[1], cs[2], indptr, indices, val, rows, 1.0, 0.8, lr)
    comp_mem = peak(comp)
    f_ms, c_ms = [], []
    for r in range(2 + rounds):                                             # the routes alternate
        a, b = timed(fused, 1, warmup=0), timed(comp, 1, warmup=0)
        if r >= 2:
            f_ms.append(a[0] / iters)
            c_ms.append(b[0])
    rep_ms, _ = timed(lambda: T._lib.check(state.lib.ampconv_tsne_repulsion(
        state.y[0].data_ptr(), N, state.neg.data_ptr(), state.Z.data_ptr(), state.ws_rep.data_ptr(), state.ws_rep.numel(),
        T._stream()), 'ampconv_tsne_repulsion'), rounds)
    out = dict(N=N, perplexity=perplexity, nnz=int(indices.numel()),
               fused_iteration_ms=round(statistics.median(f_ms), 4), fused_spread_ms=round(max(f_ms) - min(f_ms), 4),
               composite_iteration_ms=round(statistics.median(c_ms), 4), composite_spread_ms=round(max(c_ms) - min(c_ms), 4),
               speedup=round(statistics.median(c_ms) / statistics.median(f_ms), 2), repulsion_ms=round(rep_ms, 4),
               pairs_per_s=round(N * (N - 1) / (rep_ms * 1e-3), 0), fused_state_bytes=int(fused_mem), composite_peak_bytes=int(comp_mem),
               affinity_stage_ms=round(aff_ms, 3), affinity_stage_spread_ms=round(aff_spread, 3))
    print(json.dumps(out), flush=True)


def sklearn_context(N, perplexity):
    from sklearn.manifold import TSNE
    X = data(N).numpy()
    t = time.time()
    TSNE(n_components=2, perplexity=perplexity, init='pca', max_iter=300).fit(X)
    dt = time.time() - t
    print(json.dumps(dict(sklearn_N=N, threads=os.environ.get('OMP_NUM_THREADS'), total_s=round(dt, 2),
                          per_iteration_ms_including_affinities=round(dt / 300 * 1e3, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('sizes', nargs='*', type=int)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--perplexity', type=float, default=10.0)
    ap.add_argument('--sklearn', type=int, default=0, metavar='N')
    args = ap.parse_args()
    for N in args.sizes or (10_000, 96_000):
        bench(N, args.perplexity, args.rounds)
    if args.sklearn:
        sklearn_context(args.sklearn, args.perplexity)


if __name__ == '__main__':
    main()
