"""Developer benchmark: the per-token LayerNorm sites of ampnet_amd/norm.py (AMPGCN(layer_norm=True)) beside the
composite they replace, F.layer_norm on [N, L, D] followed by the fused glue pass.

    python tools/bench_norm.py [N L D] [--bf16] [--p P] [--rounds R]

Two sites, forward and backward timed separately with HIP events, both routes in one process on the same random
tensors, alternating (2 warm-up rounds, the median of the rest):
    site     norm_act_dropout(x, D, w, b, p, 'relu')            | act_dropout(F.layer_norm(x3, (D,), w, b), p, 'relu')
    readout  norm_act_dropout_pool(x, D, w, b, p, 'relu')       | act_dropout_pool(F.layer_norm(x3, (D,), w, b), D, p, 'relu')
Bytes the ALGORITHM needs, T = N L D itemsize (statistics, weight, bias and the pooled [N, D] are left out: < 1 %):
    fused:      site forward 2 T (read x, write y), backward 3 T (read x and dy, write dx);
                readout forward 1 T, backward 2 T (read x, write dx)
    composite:  layer_norm forward 2 T, backward 3 T; act_dropout forward 2 T, backward 3 T (dy, the saved output, dx);
                act_dropout_pool forward 1 T, backward 2 T.  site 4 T + 6 T, readout 3 T + 5 T
Each direction's share of the 8 TB/s HBM peak is its own byte count over its own time.  Prints a markdown table and one
JSON line.  Needs a GPU (no fallback).
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ampnet_amd import act_dropout, act_dropout_pool, norm_act_dropout, norm_act_dropout_pool  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s, MI355X


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def sites(N, L, D, p, itemsize):
    """name -> (composite route, fused route, output shape, composite (fwd, bwd) bytes, fused (fwd, bwd) bytes)"""
    T = N * L * D * itemsize

    def layer_norm(x, w, b):
        return F.layer_norm(x.view(N, L, D), (D,), w, b).view(N, L * D)
    return {
        'site': (lambda x, w, b: act_dropout(layer_norm(x, w, b), p, 'relu'),
                 lambda x, w, b: norm_act_dropout(x, D, w, b, p=p, activation='relu'), (N, L * D), (4 * T, 6 * T), (2 * T, 3 * T)),
        'readout': (lambda x, w, b: act_dropout_pool(layer_norm(x, w, b), D, p, 'relu', 'mean'),
                    lambda x, w, b: norm_act_dropout_pool(x, D, w, b, p=p, activation='relu', pooling='mean'), (N, D),
                    (3 * T, 5 * T), (T, 2 * T)),
    }


def one_call(fn, x, w, b, dy):
    """(forward ms, backward ms) of one call"""
    x.grad = w.grad = b.grad = None
    torch.cuda.synchronize()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    out = fn(x, w, b)
    e[1].record()
    out.backward(dy)
    e[2].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])


def main():
    flags = ('--p', '--rounds')
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] not in flags]
    N, L, D = (int(a) for a in args) if len(args) == 3 else (100000, 40, 100)
    p, rounds = opt('--p', 0.1, float), opt('--rounds', 10)
    dtype = torch.bfloat16 if '--bf16' in sys.argv else torch.float32
    if not torch.cuda.is_available():
        raise SystemExit('bench_norm.py needs a GPU')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    x = torch.randn(N, L * D, device=dev).to(dtype).requires_grad_(True)
    w = (1 + 0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    b = (0.1 * torch.randn(D, device=dev)).requires_grad_(True)
    wc, bc = (w, b) if dtype == torch.float32 else (w.detach().to(dtype).requires_grad_(True),      # F.layer_norm wants one dtype
                                                    b.detach().to(dtype).requires_grad_(True))
    result = {'shape': [N, L, D], 'dtype': str(dtype).split('.')[-1], 'p': p, 'rounds': rounds, 'sites': {}}
    for name, (comp_fn, fused_fn, out_shape, comp_bytes, fused_bytes) in sites(N, L, D, p, x.element_size()).items():
        dy = torch.randn(out_shape, device=dev).to(dtype)
        ms = {'composite': ([], []), 'fused': ([], [])}
        for r in range(rounds + 2):                               # alternating; the first two rounds are warm-up
            for route, fn, params in (('composite', comp_fn, (wc, bc)), ('fused', fused_fn, (w, b))):
                t = one_call(fn, x, *params, dy)
                if r >= 2:
                    ms[route][0].append(t[0])
                    ms[route][1].append(t[1])
        row = {}
        for route, nbytes in (('composite', comp_bytes), ('fused', fused_bytes)):
            for d, direction in enumerate(('fwd', 'bwd')):
                med = statistics.median(ms[route][d])
                row[f'{route}_{direction}'] = {'ms_median': med, 'ms_min': min(ms[route][d]), 'ms_max': max(ms[route][d]),
                                               'bytes': nbytes[d], 'hbm_share': nbytes[d] / (med * 1e-3) / HBM_PEAK}
        for direction in ('fwd', 'bwd'):
            row[f'fused_over_composite_{direction}'] = (row[f'fused_{direction}']['ms_median'] /
                                                        row[f'composite_{direction}']['ms_median'])
        result['sites'][name] = row
        del dy
    print(f'shape {N} x {L} x {D}, {result["dtype"]}, p = {p}, median of {rounds} rounds (min .. max)')
    print('| call | composite ms | fused ms | fused / composite | composite share of 8 TB/s | fused share of 8 TB/s | fused GB/s |')
    print('|---|---|---|---|---|---|---|')
    for name, row in result['sites'].items():
        for direction in ('fwd', 'bwd'):
            c, f = row[f'composite_{direction}'], row[f'fused_{direction}']
            print(f'| {name} {direction} | {c["ms_median"]:.3f} ({c["ms_min"]:.3f} .. {c["ms_max"]:.3f}) | {f["ms_median"]:.3f} '
                  f'({f["ms_min"]:.3f} .. {f["ms_max"]:.3f}) | {row[f"fused_over_composite_{direction}"]:.3f} | '
                  f'{c["hbm_share"]:.3f} | {f["hbm_share"]:.3f} | {f["bytes"] / (f["ms_median"] * 1e-3) / 1e9:.0f} |')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
