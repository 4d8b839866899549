"""Developer benchmark: the glue around the AMPConv layers as separate PyTorch ops (what AMPGCN.forward runs by default)
beside the fused HIP passes of ampnet_amd/glue.py (AMPGCN(fused_glue=True)).

    python tools/bench_glue.py [N L D] [--bf16] [--p P] [--rounds R]

Three sites, each forward + backward on the same random [N, L * D] tensors, both routes in one process, alternating:
    drop1     F.dropout(x, p)                                  | act_dropout(x, p, 'identity')
    relu_drop F.dropout(F.relu(x), p)                          | act_dropout(x, p, 'relu')
    readout   F.dropout(F.relu(x), p).reshape(N, L, D).mean(1) | act_dropout_pool(x, D, p, 'relu', 'mean')
Per site and route: the median over the rounds of the HIP-event time of one forward + backward (2 warm-up rounds),
torch.cuda.max_memory_allocated above what is resident before the call (x, dy), and the share of the 8 TB/s HBM peak
reached on the route's own byte count T = N L D itemsize:
    fused: drop1 4 T (forward read + write, backward read + write), relu_drop 5 T (backward also reads the saved output),
           readout 3 T (forward reads x, backward reads x and writes dx)
    torch: dropout = read + write + 1-byte mask (forward), read + mask + write (backward); relu = read + write (forward),
           2 reads + write (backward); mean = read (forward), write (backward)
Prints a markdown table and one JSON line.  Needs a GPU (no fallback).
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ampnet_amd import act_dropout, act_dropout_pool  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s, MI355X


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def sites(N, L, D, p, itemsize):
    """name -> (torch route, fused route, output shape, torch bytes, fused bytes); bytes for forward + backward."""
    T = N * L * D * itemsize
    M = N * L * D                                              # the bool mask nn.Dropout saves
    drop = (2 * T + M) + (2 * T + M)
    relu = 2 * T + 3 * T
    return {
        'drop1': (lambda x: F.dropout(x, p, True), lambda x: act_dropout(x, p, 'identity'), (N, L * D), drop, 4 * T),
        'relu_drop': (lambda x: F.dropout(F.relu(x), p, True), lambda x: act_dropout(x, p, 'relu'), (N, L * D),
                      relu + drop, 5 * T),
        'readout': (lambda x: F.dropout(F.relu(x), p, True).reshape(N, L, D).mean(dim=1),
                    lambda x: act_dropout_pool(x, D, p, 'relu', 'mean'), (N, D), relu + drop + 2 * T, 3 * T),
    }


def one_call(fn, x, dy):
    """(milliseconds, peak bytes above the resident tensors) of one forward + backward."""
    x.grad = None
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(x).backward(dy)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), torch.cuda.max_memory_allocated() - base


def main():
    flags = ('--p', '--rounds')
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] not in flags]
    N, L, D = (int(a) for a in args) if len(args) == 3 else (100000, 40, 100)
    p, rounds = opt('--p', 0.1, float), opt('--rounds', 10)
    dtype = torch.bfloat16 if '--bf16' in sys.argv else torch.float32
    if not torch.cuda.is_available():
        raise SystemExit('bench_glue.py needs a GPU')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    x = torch.randn(N, L * D, device=dev).to(dtype).requires_grad_(True)
    result = {'shape': [N, L, D], 'dtype': str(dtype).split('.')[-1], 'p': p, 'rounds': rounds, 'sites': {}}
    total = {'torch': 0.0, 'fused': 0.0}
    for name, (torch_fn, fused_fn, out_shape, torch_bytes, fused_bytes) in sites(N, L, D, p, x.element_size()).items():
        dy = torch.randn(out_shape, device=dev).to(dtype)
        ms = {'torch': [], 'fused': []}
        peak = {'torch': 0, 'fused': 0}
        for r in range(rounds + 2):                               # alternating; the first two rounds are warm-up
            for route, fn in (('torch', torch_fn), ('fused', fused_fn)):
                t, m = one_call(fn, x, dy)
                if r >= 2:
                    ms[route].append(t)
                    peak[route] = max(peak[route], m)
        row = {}
        for route, nbytes in (('torch', torch_bytes), ('fused', fused_bytes)):
            med = statistics.median(ms[route])
            total[route] += med
            row[route] = {'ms_median': med, 'ms_min': min(ms[route]), 'ms_max': max(ms[route]), 'bytes': nbytes,
                          'hbm_share': nbytes / (med * 1e-3) / HBM_PEAK, 'peak_bytes': peak[route]}
        row['fused_over_torch'] = row['fused']['ms_median'] / row['torch']['ms_median']
        result['sites'][name] = row
        del dy
    result['total_ms'] = total
    result['fused_over_torch'] = total['fused'] / total['torch']
    print(f'shape {N} x {L} x {D}, {result["dtype"]}, p = {p}, median of {rounds} rounds (min .. max), forward + backward')
    print('| site | torch ms | fused ms | fused / torch | torch share of 8 TB/s | fused share of 8 TB/s | torch peak GB | fused peak GB |')
    print('|---|---|---|---|---|---|---|---|')
    for name, row in result['sites'].items():
        t, f = row['torch'], row['fused']
        print(f'| {name} | {t["ms_median"]:.3f} ({t["ms_min"]:.3f} .. {t["ms_max"]:.3f}) | {f["ms_median"]:.3f} '
              f'({f["ms_min"]:.3f} .. {f["ms_max"]:.3f}) | {row["fused_over_torch"]:.3f} | {t["hbm_share"]:.3f} | '
              f'{f["hbm_share"]:.3f} | {t["peak_bytes"] / 1e9:.2f} | {f["peak_bytes"] / 1e9:.2f} |')
    print(f'| total | {total["torch"]:.3f} | {total["fused"]:.3f} | {result["fused_over_torch"]:.3f} | | | | |')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
