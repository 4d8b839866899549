#!/usr/bin/env python
"""Times the fused pair loss (ampnet_amd.pair_loss, forward + backward) beside the PyTorch composite of the same loss on
the same inputs: index_select, matmul, logsumexp (or softplus), then autograd.

    python tools/bench_pair_loss.py [B S D] [--bf16] [--kind skipgram|xent] [--rounds 7] [--nodes N]

Without a shape: GraphSAGE's 20 negatives (100 000, 20, 100), in-batch negatives (100 000, 16 384, 100) and the whole
cfg4 batch as negatives (100 000, 96 000, 100) -- the last one on the fused route only: the composite's [B, S] tables
(38 GB per copy) do not belong on a shared card.  Method: the two routes alternate, 2 warm-up rounds, the median of the
timed rounds by HIP events; the composite's own run-to-run spread (max - min over its rounds) is printed as the margin
of the comparison; launches counted by torch.profiler over one round; peak memory of each route above its inputs; the
fused route's FLOP rate from 2 B S D x 5 (one product forward, two per backward pass).  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ampnet_amd import pair_loss                                               # noqa: E402

DEFAULT_SHAPES = [(100_000, 20, 100, True), (100_000, 16_384, 100, True), (100_000, 96_000, 100, False)]


def composite(z, a, p, n, w, kind):
    A, P, Nn = z.index_select(0, a).float(), z.index_select(0, p).float(), z.index_select(0, n).float()
    aff = (A * P).sum(1)
    g = A @ Nn.t()
    if kind == 'skipgram':
        rows = torch.logsumexp(g, dim=1) - aff
    else:
        rows = torch.nn.functional.softplus(-aff) + torch.nn.functional.softplus(g).sum(1)
    return (w * rows).sum()


def fused(z, a, p, n, w, kind):
    return pair_loss(z, a, p, n, kind=kind, weight=w)


def one_round(route, z, args):
    z.grad = None
    route(z, *args).backward()


def timed(route, z, args):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    one_round(route, z, args)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end)


def launches(route, z, args):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        one_round(route, z, args)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def peak(route, z, args):
    torch.cuda.synchronize()
    z.grad = None
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    one_round(route, z, args)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def bench(B, S, D, with_composite, opts):
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    N = opts.nodes or max(S, 96_000)
    dtype = torch.bfloat16 if opts.bf16 else torch.float32
    z = (torch.randn(N, D, generator=g) / D ** 0.25).to(dtype).to(dev).requires_grad_(True)
    a, p = (torch.randint(0, N, (B,), generator=g).to(dev) for _ in range(2))
    n = torch.randperm(N, generator=g)[:S].to(dev) if S <= N else torch.randint(0, N, (S,), generator=g).to(dev)
    w = (0.5 + torch.rand(B, generator=g)).to(dev)
    args = (a, p, n, w, opts.kind)
    routes = [('fused', fused)] + ([('composite', composite)] if with_composite else [])
    times = {name: [] for name, _ in routes}
    for r in range(2 + opts.rounds):                                           # the routes alternate; 2 warm-up rounds
        for name, route in routes:
            t = timed(route, z, args)
            if r >= 2:
                times[name].append(t)
    out = {'B': B, 'S': S, 'D': D, 'N': N, 'dtype': str(dtype)[6:], 'kind': opts.kind, 'rounds': opts.rounds}
    for name, route in routes:
        ts = times[name]
        out[name + '_ms'] = round(statistics.median(ts), 4)
        out[name + '_spread_ms'] = round(max(ts) - min(ts), 4)
        out[name + '_launches'] = launches(route, z, args)
        out[name + '_peak_mb'] = round(peak(route, z, args), 1)
    out['fused_tflops'] = round(2.0 * B * S * D * 5 / (out['fused_ms'] * 1e-3) / 1e12, 2)
    if with_composite:
        out['speedup'] = round(out['composite_ms'] / out['fused_ms'], 2)
        out['no_slower'] = out['fused_ms'] <= out['composite_ms'] + out['composite_spread_ms']
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('shape', nargs='*', type=int, help='B S D')
    ap.add_argument('--bf16', action='store_true')
    ap.add_argument('--kind', default='skipgram', choices=['skipgram', 'xent'])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--nodes', type=int, default=0, help='rows of z (default: max(S, 96 000))')
    ap.add_argument('--no-composite', action='store_true')
    opts = ap.parse_args()
    if opts.shape and len(opts.shape) != 3:
        ap.error('a shape is three integers: B S D')
    shapes = [tuple(opts.shape) + (not opts.no_composite,)] if opts.shape else DEFAULT_SHAPES
    for B, S, D, with_composite in shapes:
        bench(B, S, D, with_composite and not opts.no_composite, opts)


if __name__ == '__main__':
    main()
