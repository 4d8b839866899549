#!/usr/bin/env python
"""Times ampnet_amd.pca and its three phases (means + Gram, eigh, projection) beside two yardsticks in the same process:
the composite a user writes in torch -- x - mean, xc^T @ xc in fp32, torch.linalg.eigh, xc @ V -- and torch.pca_lowrank.

    python tools/bench_pca.py [R W k rows|columns] [--bf16] [--rounds 5] [--no-error]

Without a shape: one GraphSAINT batch of embeddings (96 000, 100) and a million of them (1 000 000, 256) as rows, Cora's
features (2 708, 1 433) as columns with the featuriser's 99 components, and the XOR data (400, 10).  Method (that of
tools/bench_knn.py): the routes alternate in one process, 2 warm-up rounds, the median of the timed rounds by device
events, the spread max - min; the phases are timed by events of their own in rounds of their own; peak memory of each
route above its input; the Gram kernel's FLOP rate counts 2 R W^2 / 2 (the upper triangle) and its byte rate the rows
once.  Where the fp64 model fits the host (R W <= 2^25) each route's largest error against it is reported: singular
values relative to S_1, components and scores absolute after the sign rule.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from ampnet_amd import pca                                                     # noqa: E402
import ampnet_amd.pca                                                          # noqa: E402,F401
P = sys.modules['ampnet_amd.pca']

DEFAULT_SHAPES = [(96_000, 100, 16, 'rows'), (1_000_000, 256, 16, 'rows'), (2_708, 1_433, 99, 'columns'), (400, 10, 2, 'rows')]


def fused(x, k, samples):
    r = pca(x, k, samples=samples)
    return r.scores, r.components, r.singular_values


def _flip(comp, scores):
    at = comp.abs().argmax(dim=1, keepdim=True)
    sign = torch.where(comp.gather(1, at) < 0, -1.0, 1.0)
    return comp * sign, scores * sign.t()


def composite(x, k, samples):
    X = x.float() if samples == 'rows' else x.float().t()
    xc = X - X.mean(dim=0, keepdim=True)
    if samples == 'rows':
        lam, vec = torch.linalg.eigh(xc.t() @ xc)
        V = vec.flip(1)[:, :k]
        comp, scores = _flip(V.t(), xc @ V)
    else:                                                                      # the Gram matrix of the samples
        lam, vec = torch.linalg.eigh(xc @ xc.t())
        S = lam.flip(0)[:k].clamp(min=0).sqrt()
        U = vec.flip(1)[:, :k]
        comp, scores = _flip((U.t() @ xc) / S[:, None], U * S)
    return scores, comp, lam.flip(0)[:k].clamp(min=0).sqrt()


def lowrank(x, k, samples):
    X = x.float() if samples == 'rows' else x.float().t()
    U, S, V = torch.pca_lowrank(X, q=k, center=True, niter=2)
    comp, scores = _flip(V.t(), U * S)
    return scores, comp, S


def timed(route, args):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    route(*args)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end)


def peak(route, args):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    route(*args)
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - before) / 1e6


def phases(x, k, samples, rounds):
    """Median ms of the means, the Gram call, eigh and the projection, each between events of its own."""
    rows = samples == 'rows'
    out = {n: [] for n in ('mean', 'gram', 'eigh', 'project')}
    for r in range(2 + rounds):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        mean = P.column_or_row_mean(x, 0 if rows else 1)
        ev[1].record()
        Sm = P.gram(x, col_shift=mean) if rows else P.gram(x, row_shift=mean)
        ev[2].record()
        lam, vec = P.eigh_descending(Sm)
        ev[3].record()
        V = vec[:, :k].float().contiguous()
        P.project(x, V, col_shift=mean) if rows else P.project(x, V, row_shift=mean)
        ev[4].record()
        ev[4].synchronize()
        if r >= 2:
            for i, n in enumerate(out):
                out[n].append(ev[i].elapsed_time(ev[i + 1]))
    return {n: round(statistics.median(t), 4) for n, t in out.items()}


def errors(x, k, samples, results):
    import pca_reference as pr
    ref = pr.pca_model(x.float().cpu().numpy(), k, samples)
    out = {}
    for name, (scores, comp, S) in results.items():
        S = S.double().cpu().numpy()
        out[name] = {'singular_values_rel': float(np.abs(S - ref['singular_values']).max() / ref['singular_values'][0]),
                     'components': float(np.abs(comp.double().cpu().numpy() - ref['components']).max()),
                     'scores': float(np.abs(scores.double().cpu().numpy() - ref['scores']).max())}
    return out


def bench(R, W, k, samples, opts):
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    dtype = torch.bfloat16 if opts.bf16 else torch.float32
    # a decaying spectrum plus a mean: random factors, so the leading directions are separated
    r = min(R, W, 32)
    x = (torch.randn(R, r, generator=g) * (0.8 ** torch.arange(r))) @ torch.randn(r, W, generator=g) / r ** 0.5
    x = (x + 0.05 * torch.randn(R, W, generator=g) + torch.randn(W, generator=g)).to(dtype).to(dev)
    args = (x, k, samples)
    routes = [('fused', fused), ('composite', composite), ('lowrank', lowrank)]
    times = {name: [] for name, _ in routes}
    for rnd in range(2 + opts.rounds):
        for name, route in routes:
            t = timed(route, args)
            if rnd >= 2:
                times[name].append(t)
    out = {'R': R, 'W': W, 'k': k, 'samples': samples, 'dtype': str(dtype)[6:], 'rounds': opts.rounds,
           'eigh_on_device': bool(P.EIGH_DEVICE), 'gram_splits': int(P._lib.load().ampconv_pca_gram_splits(R, W))}
    for name, route in routes:
        ts = times[name]
        out[name + '_ms'] = round(statistics.median(ts), 4)
        out[name + '_spread_ms'] = round(max(ts) - min(ts), 4)
        out[name + '_peak_mb'] = round(peak(route, args), 1)
    out['phases_ms'] = phases(x, k, samples, opts.rounds)
    gram_s = out['phases_ms']['gram'] * 1e-3
    out['gram_tflops'] = round(R * W * (W + 1.0) / gram_s / 1e12, 3)
    out['gram_gbytes_per_s'] = round(R * W * x.element_size() / gram_s / 1e9, 1)
    out['speedup_vs_composite'] = round(out['composite_ms'] / out['fused_ms'], 2)
    if not opts.no_error and R * W <= 1 << 25:
        out['max_error'] = errors(x, k, samples, {name: route(*args) for name, route in routes})
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('shape', nargs='*', help='R W k rows|columns')
    ap.add_argument('--bf16', action='store_true')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-error', action='store_true')
    opts = ap.parse_args()
    if opts.shape and len(opts.shape) != 4:
        ap.error('a shape is R W k rows|columns')
    shapes = [(int(opts.shape[0]), int(opts.shape[1]), int(opts.shape[2]), opts.shape[3])] if opts.shape else DEFAULT_SHAPES
    for R, W, k, samples in shapes:
        bench(R, W, k, samples, opts)


if __name__ == '__main__':
    main()
