"""Developer benchmark: the reference's loss tail as PyTorch ops beside the fused head + loss of ampnet_amd/head.py.

    python tools/bench_head.py [N D C] [--bf16] [--rounds R]

Both routes start from the same pooled [N, D], W [C, D], b, labels, node_norm and two masks and run forward + backward:
    torch: out = log_softmax(linear(pooled, W, b)); per mask (F.nll_loss(out, y, reduction='none') * node_norm)[mask].sum()
           and (out.argmax(1) == y)[mask].float().mean(); backward of the first mask's loss; loss.item() and float(acc)
           as examples/train_graphsaint.py and the reference's loop do (the boolean indexing synchronises on its own)
    fused: saint_nll_loss(pooled, W, b, y, node_norm, (mask0, mask1), metrics=m).backward(); nothing is read back
Without arguments: (1200, 128, 7) a Cora-sized GraphSAINT batch, (96000, 256, 7), (1000000, 256, 7).
Per shape and route: the median over the rounds of the HIP-event time of one step (2 warm-up rounds, routes alternating),
the kernel launches of one step counted by torch.profiler, and for the fused route the rate at which it moves its own
byte count (pooled read once forward; read again and dpooled written backward: 3 N D itemsize) as a share of the 8 TB/s peak.
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

from ampnet_amd import HeadMetrics, saint_nll_loss  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s, MI355X
SHAPES = [(1200, 128, 7), (96000, 256, 7), (1000000, 256, 7)]


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def make_routes(N, D, C, dtype, dev):
    g = torch.Generator(device='cpu').manual_seed(0)
    pooled = torch.randn(N, D, generator=g).to(dev).to(dtype).requires_grad_(True)
    W = ((torch.rand(C, D, generator=g) * 2 - 1) / D ** 0.5).to(dev).requires_grad_(True)
    b = ((torch.rand(C, generator=g) * 2 - 1) / D ** 0.5).to(dev).requires_grad_(True)
    y = torch.randint(0, C, (N,), generator=g).to(dev)
    norm = (torch.rand(N, generator=g) * 3 + 0.1).to(dev)
    train = (torch.rand(N, generator=g) < 0.5).to(dev)
    test = ~train
    metrics = HeadMetrics(2, dev)
    leaves = (pooled, W, b)

    def torch_step():
        out = F.log_softmax(F.linear(pooled.float() if dtype != torch.float32 else pooled, W, b), dim=1)
        loss = (F.nll_loss(out, y, reduction='none') * norm)[train].sum()
        loss.backward()
        test_loss = (F.nll_loss(out, y, reduction='none') * norm)[test].sum()
        hit = out.argmax(1) == y
        return loss.item(), float(hit[train].float().mean()), test_loss.item(), float(hit[test].float().mean())

    def fused_step():
        saint_nll_loss(pooled, W, b, y, norm, (train, test), metrics=metrics).backward()

    return leaves, torch_step, fused_step


def timed(step, leaves):
    for t in leaves:
        t.grad = None
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def launches(step):
    """Kernel launches of one step (memsets and copies not counted), or None where the profiler sees no device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
                and not e.name.lower().startswith(('memcpy', 'memset')))
        return n or None
    except Exception:                                               # the count is a side measurement
        return None


def bench(N, D, C, dtype, rounds, dev):
    leaves, torch_step, fused_step = make_routes(N, D, C, dtype, dev)
    ms = {'torch': [], 'fused': []}
    for r in range(rounds + 2):                                     # alternating; the first two rounds are warm-up
        for route, step in (('torch', torch_step), ('fused', fused_step)):
            t = timed(step, leaves)
            if r >= 2:
                ms[route].append(t)
    row = {'shape': [N, D, C]}
    for route, step in (('torch', torch_step), ('fused', fused_step)):
        row[route] = {'ms_median': statistics.median(ms[route]), 'ms_min': min(ms[route]), 'ms_max': max(ms[route]),
                      'launches': launches(step)}
    nbytes = 3 * N * D * leaves[0].element_size()
    row['fused']['bytes'] = nbytes
    row['fused']['hbm_share'] = nbytes / (row['fused']['ms_median'] * 1e-3) / HBM_PEAK
    row['fused_over_torch'] = row['fused']['ms_median'] / row['torch']['ms_median']
    return row


def main():
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] != '--rounds']
    shapes = [tuple(int(a) for a in args)] if len(args) == 3 else SHAPES
    rounds = opt('--rounds', 20)
    dtype = torch.bfloat16 if '--bf16' in sys.argv else torch.float32
    if not torch.cuda.is_available():
        raise SystemExit('bench_head.py needs a GPU')
    dev = torch.device('cuda:0')
    result = {'dtype': str(dtype).split('.')[-1], 'rounds': rounds, 'device': torch.cuda.get_device_name(0), 'rows': []}
    for N, D, C in shapes:
        result['rows'].append(bench(N, D, C, dtype, rounds, dev))
        torch.cuda.empty_cache()
    print(f'{result["device"]}, pooled {result["dtype"]}, median of {rounds} rounds (min .. max), forward + backward, two masks')
    print('| N, D, C | torch ms | fused ms | fused / torch | torch launches | fused launches | fused share of 8 TB/s |')
    print('|---|---|---|---|---|---|---|')
    for row in result['rows']:
        t, f = row['torch'], row['fused']
        print(f'| {", ".join(map(str, row["shape"]))} | {t["ms_median"]:.3f} ({t["ms_min"]:.3f} .. {t["ms_max"]:.3f}) | '
              f'{f["ms_median"]:.3f} ({f["ms_min"]:.3f} .. {f["ms_max"]:.3f}) | {row["fused_over_torch"]:.3f} | '
              f'{t["launches"] or "not measured"} | {f["launches"] or "not measured"} | {f["hbm_share"]:.3f} |')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
