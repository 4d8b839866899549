"""Developer benchmark: one optimizer step over AMPGCN's actual parameter set, ampnet_amd.FusedAdam beside torch.optim.Adam.

    python tools/bench_optim.py [--steps S] [--no-train] [--only VARIANT] [--bf16]

Parameter sets: AMPGCN at 128 / 4 / 20 (experiments/cora_benchmark_graphsaint.py) and at the class defaults 100 / 2 / 40,
each with and without layer_norm; every parameter gets a random gradient once.  Variants, all with lr=0.1,
weight_decay=1e-4 and the zeroing of the gradients that belongs to a training step:
    fused            FusedAdam.step(set_to_none=True) (the gradients are re-attached outside the timed region)
    fused+clip       the same with max_grad_norm=1.0: the norm's two launches and the device-side coefficient
    torch foreach    torch.optim.Adam (its default multi-tensor path): zero_grad() + step()
    torch fused      torch.optim.Adam(fused=True): zero_grad() + step()
Per set and variant: the median over S steps (default 300, after 20 warm-up steps, variants alternating) of the HIP-event
time of one step, and the kernel launches of one step counted by torch.profiler.  --only runs one variant for S steps
and nothing else (for a kernel trace of exactly that variant).  --bf16: the class-default set only, as
AMPGCN(storage_dtype=torch.bfloat16) holds it -- conv parameters and their gradients in bf16, the rest fp32 --, FusedAdam's
mixed-precision step (fp32 masters) with and without clipping; the torch variants are left out (torch.optim.Adam on bf16
parameters is a different, lossy computation).  Unless --no-train: the per-batch time that
examples/train_graphsaint.py --fused-head prints for its last epoch, with and without --fused-adam, each in a child
process.  Prints a markdown table and one JSON line.  Needs a GPU (no fallback).
"""
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ampnet_amd import AMPGCN, FusedAdam  # noqa: E402

SETS = [('128/4/20', dict(embedding_dim=128, num_heads=4, num_sampled_vectors=20, feat_emb_dim=127), False),
        ('128/4/20 +LN', dict(embedding_dim=128, num_heads=4, num_sampled_vectors=20, feat_emb_dim=127), True),
        ('100/2/40', dict(), False),
        ('100/2/40 +LN', dict(), True)]
VARIANTS = ['fused', 'fused+clip', 'torch foreach', 'torch fused']
LR, WD = 0.1, 1e-4


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def make_variant(name, shapes, dev, dtypes=None):
    """(prepare, step): prepare() attaches the gradients (not timed), step() is what a training step runs."""
    g = torch.Generator().manual_seed(0)
    dtypes = dtypes or [torch.float32] * len(shapes)
    params = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev, dt)) for s, dt in zip(shapes, dtypes)]
    grads = [(torch.randn(s, generator=g) * 0.01).to(dev, dt) for s, dt in zip(shapes, dtypes)]

    def prepare():
        for p, gr in zip(params, grads):
            p.grad = gr

    if name.startswith('fused'):
        o = FusedAdam(params, lr=LR, weight_decay=WD, max_grad_norm=1.0 if name == 'fused+clip' else None)
        return prepare, lambda: o.step(set_to_none=True)
    o = torch.optim.Adam(params, lr=LR, weight_decay=WD, fused=(name == 'torch fused') or None)

    def step():
        o.step()
        o.zero_grad()                                              # set_to_none: no launch, as in the training loop
    return prepare, step


def timed(prepare, step):
    prepare()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def launches(prepare, step):
    """Kernel launches of one step (memsets and copies not counted), or None where the profiler sees no device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        prepare()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')
                and not e.name.lower().startswith(('memcpy', 'memset')))
        return n or None
    except Exception:                                               # the count is a side measurement
        return None


def parameter_shapes(cfg, layer_norm, storage_dtype=torch.float32):
    model = AMPGCN(device='cpu', dropout_rate=0.0, dropout_adj_rate=0.0, layer_norm=layer_norm, storage_dtype=storage_dtype,
                   **cfg)
    return [tuple(p.shape) for p in model.parameters()], [p.dtype for p in model.parameters()]


def bench(label, cfg, layer_norm, steps, dev, variants=VARIANTS, storage_dtype=torch.float32):
    shapes, dtypes = parameter_shapes(cfg, layer_norm, storage_dtype)
    routes = {v: make_variant(v, shapes, dev, dtypes) for v in variants}
    ms = {v: [] for v in variants}
    for r in range(steps + 20):                                     # alternating; the first 20 rounds are warm-up
        for v in variants:
            t = timed(*routes[v])
            if r >= 20:
                ms[v].append(t)
    row = {'set': label, 'tensors': len(shapes), 'elements': sum(int(torch.Size(s).numel()) for s in shapes)}
    for v in variants:
        row[v] = {'ms_median': statistics.median(ms[v]), 'ms_min': min(ms[v]), 'ms_max': max(ms[v]),
                  'launches': launches(*routes[v])}
    return row


def train_ms(extra):
    """ms per sampled batch of the example's last epoch (child process)."""
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_graphsaint.py'), '--epochs', '4', '--fused-head'] + extra
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    lines = [l for l in out.splitlines() if l.startswith('epoch ') or l.startswith('full-graph')]
    return float(re.findall(r'= ([0-9.]+) ms per sampled batch', out)[-1]), lines


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim.py needs a GPU')
    dev = torch.device('cuda:0')
    steps = opt('--steps', 300)
    only = opt('--only', None, str)
    if only is not None:                                            # one variant, nothing else: for a kernel trace
        label, cfg, ln = SETS[2]
        shapes, dtypes = parameter_shapes(cfg, ln, torch.bfloat16 if '--bf16' in sys.argv else torch.float32)
        prepare, step = make_variant(only, shapes, dev, dtypes)
        for _ in range(steps):
            prepare()
            step()
        torch.cuda.synchronize()
        print(f'{only}: {steps} steps over the {label} set')
        return
    if '--bf16' in sys.argv:                                        # the class-default set, fp32 and bf16 storage side by side
        label, cfg, ln = SETS[2]
        variants = VARIANTS[:2]
        rows = [bench(label + ' fp32', cfg, ln, steps, dev, variants),
                bench(label + ' bf16 storage', cfg, ln, steps, dev, variants, torch.bfloat16)]
        print(f'{torch.cuda.get_device_name(0)}, one optimizer step, median of {steps} steps in ms (min .. max) / kernel launches')
        for row in rows:
            for v in variants:
                print(f'| {row["set"]} | {v} | {row[v]["ms_median"]:.4f} ({row[v]["ms_min"]:.4f} .. {row[v]["ms_max"]:.4f}) / '
                      f'{row[v]["launches"] or "not measured"} |')
        if '--no-train' not in sys.argv:
            for extra in (['--fused-adam'], ['--fused-adam', '--bf16'], ['--fused-adam', '--class-defaults'],
                          ['--fused-adam', '--class-defaults', '--bf16']):
                ms, lines = train_ms(extra)
                rows.append({'train': extra, 'ms_per_batch_last_epoch': ms, 'log': lines})
                print(f'examples/train_graphsaint.py --epochs 4 --fused-head {" ".join(extra)}: {ms:.2f} ms per sampled batch')
        print(json.dumps({'steps': steps, 'device': torch.cuda.get_device_name(0), 'rows': rows}))
        return
    result = {'steps': steps, 'device': torch.cuda.get_device_name(0), 'rows': [bench(*s, steps, dev) for s in SETS]}
    print(f'{result["device"]}, one optimizer step, median of {steps} steps in ms (min .. max) / kernel launches')
    print('| parameter set | tensors | elements | ' + ' | '.join(VARIANTS) + ' |')
    print('|---|---|---|' + '---|' * len(VARIANTS))
    for row in result['rows']:
        cells = [f'{row[v]["ms_median"]:.4f} ({row[v]["ms_min"]:.4f} .. {row[v]["ms_max"]:.4f}) / '
                 f'{row[v]["launches"] or "not measured"}' for v in VARIANTS]
        print(f'| {row["set"]} | {row["tensors"]} | {row["elements"]} | ' + ' | '.join(cells) + ' |')
    if '--no-train' not in sys.argv:
        result['train'] = {}
        for name, extra in (('torch.optim.Adam', []), ('--fused-adam', ['--fused-adam'])):
            ms, lines = train_ms(extra)
            result['train'][name] = {'ms_per_batch_last_epoch': ms, 'log': lines}
            print(f'examples/train_graphsaint.py --epochs 4 --fused-head {" ".join(extra)}: {ms:.2f} ms per sampled batch '
                  f'(last epoch)')
            for l in lines:
                print('    ' + l)
    print(json.dumps(result))


if __name__ == '__main__':
    main()
