"""Developer benchmark: tensor statistics on the device (ampnet_amd.tensor_stats, csrc/stats.hip) beside what a user would
write today.

    python tools/bench_stats.py [--rows N] [--reps R] [--no-train] [--large-only] [--trace]

(a) The parameter gradients of the examples/train_graphsaint.py model (AMPGCN 128 / 4 / 20): one gradient_stats() with its
    30-bin histogram and median.
(b) One large activation tensor, [N, 20 * 128] with N = 100 000 (cfg3, ~1 GB in fp32), N(0,1) and ReLU of it (more than
    half of all elements in one bin), fp32 and bf16: each pass alone through the C ABI -- moments, the histogram over the
    tensor's own range (50 bins), the median -- and tensor_stats(x, bins=50, median=True) as a whole.
Baselines, in the same run:
    (i)  torch on the device: isfinite().all(), min, max, mean, std, abs().mean(), torch.histc, torch.median on the same
         tensor(s);
    (ii) the reference's way (amp_gcn.py:278-405): .cpu().numpy() and numpy for the same numbers, at (a) and at the
         activation of a 1 000-node batch only.
Times are HIP-event times (host clock around a synchronise for (ii)), medians over R repetitions (default 10) after 3
warm-up calls, variants alternating.  A pass is also given as achieved read bandwidth: the bytes of the tensor times the
number of times the pass reads it (1, 1, and 3 digit passes for fp32 / 2 for bf16), over its time, beside the 8 TB/s peak.
Unless --no-train: the per-batch time examples/train_graphsaint.py prints for its last epoch with and without
--diagnostics 4, each in a child process.  --trace: nothing is timed; one gradient_stats().read() and one
tensor_stats(large fp32, bins=50, median=True).read(), for a kernel trace that counts the launches of a call.
Prints a markdown table and one JSON line.  Needs a GPU (no fallback).
"""
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ampnet_amd import AMPGCN, _lib, tensor_stats  # noqa: E402
from ampnet_amd.graph import _stream  # noqa: E402

PEAK_TBS = 8.0


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def event_ms(fns, reps, warmup=3):
    """{name: median HIP-event milliseconds of fn()}; the variants alternate."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in times.items()}


def host_ms(f, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return statistics.median(out)


def torch_composition(x, bins):
    """What a user would write today, on the device; the results stay there."""
    return (torch.isfinite(x).all(), x.min(), x.max(), x.mean(), x.std(), x.abs().mean(),
            torch.histc(x.float() if x.dtype != torch.float32 else x, bins=bins), torch.median(x))


def numpy_way(x, bins):
    """The reference's way: the tensor to the host, numpy on it."""
    a = x.detach().float().view(-1).cpu().numpy()
    return (np.isfinite(a).all(), np.histogram(a, bins=bins), a.mean(), np.median(a), a.std(ddof=1), np.abs(a).mean(),
            np.abs(a).max())


class Passes:
    """The three C entry points on one tensor, each callable alone (the records of the moments pass stay valid)."""

    def __init__(self, x, bins=50):
        self.lib = _lib.load()
        self.x, self.bins = x, bins
        code = _lib.AMPCONV_BF16 if x.dtype == torch.bfloat16 else _lib.AMPCONV_F32
        self.table = (_lib.StatsTensor * 1)((x.data_ptr(), x.numel(), code))
        dev = x.device
        self.records = torch.zeros(_lib.STATS_RECORD_BYTES, dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(bins + 2, dtype=torch.int64, device=dev)
        self.out = torch.zeros(1, dtype=torch.float32, device=dev)
        self.ws = torch.empty(self.lib.ampconv_stats_workspace_bytes(self.table, 1), dtype=torch.uint8, device=dev)
        self.q = (ctypes.c_double * 1)(0.5)

    def moments(self):
        _lib.check(self.lib.ampconv_stats_moments(self.table, 1, self.records.data_ptr(), self.ws.data_ptr(),
                                                  self.ws.numel(), _stream()), 'moments')

    def histogram(self):
        _lib.check(self.lib.ampconv_stats_histogram(self.table, 1, self.bins, None, self.records.data_ptr(),
                                                    self.counts.data_ptr(), _stream()), 'histogram')

    def median(self):
        _lib.check(self.lib.ampconv_stats_select(self.table, 1, self.q, 1, self.records.data_ptr(), self.out.data_ptr(),
                                                 self.ws.data_ptr(), self.ws.numel(), _stream()), 'select')


def example_model(dev):
    torch.manual_seed(1)
    model = AMPGCN(device=dev, embedding_dim=128, num_heads=4, num_node_features=1433, num_sampled_vectors=20, output_dim=7,
                   softmax_out=True, feat_emb_dim=127, val_emb_dim=1, dropout_rate=0.0, dropout_adj_rate=0.0).to(dev)
    g = torch.Generator().manual_seed(2)
    for p in model.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * 0.01).to(dev)
    return model


def bench_gradients(dev, reps, rows):
    model = example_model(dev)
    grads = [p.grad for n, p in model.named_parameters() if 'weight' in n]
    fns = {'gradient_stats()': lambda: model.gradient_stats(),
           'torch on the device': lambda: [torch_composition(g, 30) for g in grads]}
    ms = event_ms(fns, reps)
    ms['gradient_stats().read()'] = host_ms(lambda: model.gradient_stats().read(), reps)
    ms['.cpu().numpy() + numpy'] = host_ms(lambda: [numpy_way(g, 30) for g in grads], reps)
    elements = sum(g.numel() for g in grads)
    rows.append(f'| (a) {len(grads)} weight gradients, {elements} elements | ' + ' | '.join(f'{k}: {v:.3f} ms' for k, v in ms.items()) + ' |')
    return {'tensors': len(grads), 'elements': elements, 'ms': ms}


def bench_large(dev, n_rows, reps, rows):
    out = {}
    base = torch.randn(n_rows, 20 * 128, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    for content in ('normal', 'relu'):
        x32 = base if content == 'normal' else torch.relu(base)
        for dtype in (torch.float32, torch.bfloat16):
            x = x32 if dtype == torch.float32 else x32.to(dtype)
            p = Passes(x)
            p.moments()
            fns = {'moments': p.moments, 'histogram': p.histogram, 'median': p.median,
                   'all three': lambda: tensor_stats(x, bins=50, median=True),
                   'torch moments': lambda: (torch.isfinite(x).all(), x.min(), x.max(), x.mean(), x.std(), x.abs().mean()),
                   'torch histc': lambda: torch.histc(x if x.dtype == torch.float32 else x.float(), bins=50), 'torch median': lambda: torch.median(x)}
            ms = event_ms(fns, reps)
            gb = x.numel() * x.element_size() / 1e9
            reads = {'moments': 1, 'histogram': 1, 'median': 3 if dtype == torch.float32 else 2}
            reads['all three'] = sum(reads.values())
            tbs = {k: reads[k] * gb / ms[k] for k in reads}             # GB / ms = TB / s
            name = f'{content} {"fp32" if dtype == torch.float32 else "bf16"}'
            out[name] = {'GB': gb, 'ms': ms, 'TB_per_s': tbs}
            torch_all = ms['torch moments'] + ms['torch histc'] + ms['torch median']
            rows.append(f'| (b) {name} [{n_rows}, 2560], {gb:.2f} GB | '
                        + ' | '.join(f'{k}: {ms[k]:.3f} ms = {tbs[k]:.2f} TB/s ({100 * tbs[k] / PEAK_TBS:.0f} %)' for k in reads)
                        + f' | torch: moments {ms["torch moments"]:.3f}, histc {ms["torch histc"]:.3f}, median '
                          f'{ms["torch median"]:.3f}, together {torch_all:.3f} ms = {torch_all / ms["all three"]:.1f} x |')
            del p, x
        del x32
    return out


def bench_batch_activation(dev, reps, rows):
    """The activation of a 1 000-node batch: the size at which the reference's host path is tolerable."""
    x = torch.randn(1000, 20 * 128, device=dev, generator=torch.Generator(device=dev).manual_seed(4))
    ms = event_ms({'tensor_stats': lambda: tensor_stats(x, bins=50, median=True),
                   'torch on the device': lambda: torch_composition(x, 50)}, reps)
    ms['tensor_stats().read()'] = host_ms(lambda: tensor_stats(x, bins=50, median=True).read(), reps)
    ms['.cpu().numpy() + numpy'] = host_ms(lambda: numpy_way(x, 50), reps)
    rows.append('| one [1000, 2560] fp32 activation | ' + ' | '.join(f'{k}: {v:.3f} ms' for k, v in ms.items()) + ' |')
    return ms


def train_ms(extra):
    cmd = [sys.executable, os.path.join(ROOT, 'examples', 'train_graphsaint.py'), '--epochs', '3'] + extra
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(' '.join(cmd) + '\n' + r.stdout)
    return float(re.findall(r'= ([0-9.]+) ms per sampled batch', r.stdout)[-1])


def main():
    assert torch.cuda.is_available(), 'tools/bench_stats.py needs a GPU'
    dev = torch.device('cuda:0')
    n_rows, reps = opt('--rows', 100_000), opt('--reps', 10)
    if '--trace' in sys.argv:
        model = example_model(dev)
        x = torch.randn(n_rows, 20 * 128, device=dev)
        torch.cuda.synchronize()
        model.gradient_stats().read()
        tensor_stats(x, bins=50, median=True).read()
        return
    rows, result = [], {'lib': _lib.LIB_PATH, 'rows': n_rows, 'reps': reps}
    if '--large-only' not in sys.argv:
        result['gradients'] = bench_gradients(dev, reps, rows)
        result['batch_activation'] = bench_batch_activation(dev, reps, rows)
    result['large'] = bench_large(dev, n_rows, reps, rows)
    if '--no-train' not in sys.argv and '--large-only' not in sys.argv:
        result['train_ms_per_batch'] = {'plain': train_ms([]), '--diagnostics 4': train_ms(['--diagnostics', '4'])}
        rows.append(f'| examples/train_graphsaint.py, last epoch, per batch | plain: {result["train_ms_per_batch"]["plain"]:.2f} ms | '
                    f'--diagnostics 4: {result["train_ms_per_batch"]["--diagnostics 4"]:.2f} ms |')
    print('\n'.join(rows))
    print(json.dumps(result))


if __name__ == '__main__':
    main()
