#!/usr/bin/env python
"""Times the fused nearest-neighbour search (ampnet_amd.knn, all rows against all rows) beside the composite a user writes
without it: torch.topk(x[chunk] @ x.t(), k) over row chunks sized so that one [chunk, N] block is at most 1 GiB.

    python tools/bench_knn.py [N D k] [--metric dot|cosine|l2] [--bf16] [--rounds 7] [--no-composite]

Without a shape: one cfg4 GraphSAINT batch (96 000, 100, 10), cfg4's million nodes (1 000 000, 128, 10) and the example's
evaluation (2 708, 128, 1).  Method (that of tools/bench_pair_loss.py): the two routes alternate in one process, 2 warm-up
rounds, the median of the timed rounds by HIP events; the spread is max - min over a route's rounds and the composite's
is the margin of the comparison; launches and the fused route's per-kernel times from torch.profiler over one round;
peak memory of each route above its inputs; the fused route's FLOP rate counts 2 Q S D.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ampnet_amd import knn                                                     # noqa: E402

DEFAULT_SHAPES = [(96_000, 100, 10), (1_000_000, 128, 10), (2_708, 128, 1)]
BLOCK_BYTES = 1 << 30


def composite(x, k, metric):
    N = x.size(0)
    xf = x.float()
    if metric == 'cosine':
        xf = torch.nn.functional.normalize(xf, dim=1)
    sq = (xf * xf).sum(1) if metric == 'l2' else None
    chunk = max(1, min(N, BLOCK_BYTES // (4 * N)))
    idx, score = [], []
    for r in range(0, N, chunk):
        g = xf[r:r + chunk] @ xf.t()
        if metric == 'l2':
            g = (2.0 * g - sq[r:r + chunk, None] - sq[None, :]).clamp_(max=0.0)          # -d2
        s, i = torch.topk(g, k, dim=1)
        idx.append(i)
        score.append(s)
    return torch.cat(idx), torch.cat(score)


def fused(x, k, metric):
    return knn(x, k, metric=metric)


def timed(route, args):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    route(*args)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end)


def profiled(route, args):
    """(device launches, {kernel name: ms}) of one round."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        route(*args)
        torch.cuda.synchronize()
    events = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = {}
    for e in events:
        name = e.name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0][:48]
        kernels[name] = kernels.get(name, 0.0) + e.device_time_total / 1e3
    return len(events), {n: round(t, 4) for n, t in sorted(kernels.items(), key=lambda kv: -kv[1])}


def peak(route, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    route(*args)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def bench(N, D, k, opts):
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    dtype = torch.bfloat16 if opts.bf16 else torch.float32
    x = torch.randn(N, D, generator=g).to(dtype).to(dev)
    args = (x, k, opts.metric)
    routes = [('fused', fused)] + ([] if opts.no_composite else [('composite', composite)])
    times = {name: [] for name, _ in routes}
    for r in range(2 + opts.rounds):                                           # the routes alternate; 2 warm-up rounds
        for name, route in routes:
            t = timed(route, args)
            if r >= 2:
                times[name].append(t)
    out = {'N': N, 'D': D, 'k': k, 'metric': opts.metric, 'dtype': str(dtype)[6:], 'rounds': opts.rounds}
    for name, route in routes:
        ts = times[name]
        out[name + '_ms'] = round(statistics.median(ts), 4)
        out[name + '_spread_ms'] = round(max(ts) - min(ts), 4)
        out[name + '_launches'], kernels = profiled(route, args)
        if name == 'fused':
            out['fused_kernels_ms'] = kernels
        out[name + '_peak_mb'] = round(peak(route, args), 1)
    out['fused_tflops'] = round(2.0 * N * N * D / (out['fused_ms'] * 1e-3) / 1e12, 2)
    if not opts.no_composite:
        out['speedup'] = round(out['composite_ms'] / out['fused_ms'], 2)
        out['no_slower'] = out['fused_ms'] <= out['composite_ms'] + out['composite_spread_ms']
        if opts.metric == 'dot' and not opts.bf16:                             # the two routes' neighbours, where no tie decides
            fi, ci = fused(*args)[0], composite(*args)[0]
            out['rows_with_equal_idx'] = round(float((fi == ci).all(1).float().mean()), 6)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('shape', nargs='*', type=int, help='N D k')
    ap.add_argument('--metric', default='dot', choices=['dot', 'cosine', 'l2'])
    ap.add_argument('--bf16', action='store_true')
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-composite', action='store_true')
    opts = ap.parse_args()
    if opts.shape and len(opts.shape) != 3:
        ap.error('a shape is three integers: N D k')
    for N, D, k in ([tuple(opts.shape)] if opts.shape else DEFAULT_SHAPES):
        bench(N, D, k, opts)


if __name__ == '__main__':
    main()
