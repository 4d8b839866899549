"""Developer benchmark: masked feature modelling as PyTorch ops beside the fused kernels of ampnet_amd/masked.py.

    python tools/bench_masked.py [--nodes N] [--rounds R]

Shapes: the class-default token shape L = 40, D = 100 and cfg3's L = 20, D = 128, N = 100 000 nodes (F = 1433 feature
columns); mask rates 0.15 and 0.75; fp32 and bf16 tokens.  Three phases, each timed on its own, both routes from the same
inputs in the same process:
    build     fused: build_masked_tokens (tokens, mask and target in one kernel, the mask drawn inside)
              torch: the library's plain token build, then mask = rand(N, L) < rate, tokens.view(T, D)[mask] = mask_token
                     (index_put over the token tensor) and target = (x.gather(1, idx) - mean[idx]) * inv_std[idx]
    loss fwd  fused: masked_value_loss(h, masked, target, W, b)
              torch: ((h[masked].float() @ W.T + b - target[masked]) ** 2).mean()     (boolean index: nonzero + gather)
    loss bwd  the backward of each, gradients to h, W and b
Per phase and route: the median over the rounds of the HIP-event time (2 warm-up rounds, routes alternating, every round
ends in a device synchronise).  The byte model, from shapes alone (T = N L, r = the measured masked share, s = the token
item size): build  T D s + T (1 + 4 + 4)   [tokens written; mask and target written, idx read; table rows and x come from
cache];  loss fwd  r T D s + T (1 + 4) + r T 4   [masked rows read; mask read, resid written; target of the masked];
loss bwd  r T D s + T D s + T (1 + 4)   [masked rows read, dh written whole; mask and resid read].  `share` is that byte
count over the fused time as a share of the 8 TB/s peak.  Prints a markdown table and one JSON line.  Needs a GPU."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ampnet_amd import FeatureTokens, build_masked_tokens, masked_value_loss  # noqa: E402
from ampnet_amd.module.feature_tokens import _BuildTokens  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s, MI355X
SHAPES = [(40, 100), (20, 128)]
RATES = (0.15, 0.75)
FDIM = 1433


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def bench(N, L, D, rate, dtype, rounds, dev):
    g = torch.Generator(device='cpu').manual_seed(0)
    gd = torch.Generator(device=dev).manual_seed(0)
    ft = FeatureTokens(FDIM, D - 1, L, seed=1, token_dtype=dtype).to(dev)
    table = ft.feature_embedding_table.weight.detach()
    x = torch.randn(N, FDIM, generator=gd, device=dev)
    idx = torch.randint(0, FDIM, (N, L), generator=gd, device=dev, dtype=torch.int32)
    idx64 = idx.long()
    mean, inv_std = ft.zscore_stats(x)
    mask_token = (0.02 * torch.randn(1, D, generator=g)).to(dev)
    W = ((torch.rand(1, D, generator=g) * 2 - 1) / D ** 0.5).to(dev).requires_grad_(True)
    b = ((torch.rand(1, generator=g) * 2 - 1) / D ** 0.5).to(dev).requires_grad_(True)
    h = torch.randn(N, L * D, generator=gd, device=dev).to(dtype).requires_grad_(True)
    T, s = N * L, h.element_size()
    state = {}

    def fused_build():
        with torch.no_grad():
            return build_masked_tokens(table, mask_token, x, mean, inv_std, idx, seed=7, rate=rate, dtype=dtype)

    def torch_build():
        with torch.no_grad():
            tokens = _BuildTokens.apply(table, x, mean, inv_std, idx, dtype)
            masked = torch.rand(N, L, device=dev) < rate
            tokens.view(T, D)[masked.view(-1)] = mask_token.to(dtype)
            target = (x.gather(1, idx64) - mean[idx64]) * inv_std[idx64]
            return tokens, masked, target

    _, masked, target = fused_build()
    masked = masked.view(torch.bool)

    def fused_fwd():
        state['fused'] = masked_value_loss(h, masked, target, W, b)

    def torch_fwd():
        rows = h.view(N, L, D)[masked]
        state['torch'] = ((rows.float() @ W.T + b - target[masked][:, None]) ** 2).mean()

    def backward(route):
        def run():
            for t in (h, W, b):
                t.grad = None
            state[route].backward()
        return run

    ms = {k: [] for k in ('build torch', 'build fused', 'fwd torch', 'fwd fused', 'bwd torch', 'bwd fused')}
    for r in range(rounds + 2):                                     # alternating; the first two rounds are warm-up
        for route, build, fwd in (('torch', torch_build, torch_fwd), ('fused', fused_build, fused_fwd)):
            times = (timed(build)[0], timed(fwd)[0], timed(backward(route))[0])
            if r >= 2:
                for phase, t in zip(('build', 'fwd', 'bwd'), times):
                    ms[f'{phase} {route}'].append(t)
    share = float(masked.float().mean())
    close = abs(float(state['fused']) - float(state['torch'])) <= 1e-3 * max(1.0, abs(float(state['torch'])))
    nbytes = {'build': T * D * s + 9 * T, 'fwd': share * T * D * s + 5 * T + 4 * share * T,
              'bwd': share * T * D * s + T * D * s + 5 * T}
    row = {'shape': [N, L, D], 'rate': rate, 'dtype': str(dtype).split('.')[-1], 'masked_share': share, 'losses_agree': close}
    for phase in ('build', 'fwd', 'bwd'):
        t, f = ms[f'{phase} torch'], ms[f'{phase} fused']
        row[phase] = {'torch_ms': statistics.median(t), 'torch_min': min(t), 'torch_max': max(t),
                      'fused_ms': statistics.median(f), 'fused_min': min(f), 'fused_max': max(f), 'bytes': int(nbytes[phase]),
                      'hbm_share': nbytes[phase] / (statistics.median(f) * 1e-3) / HBM_PEAK}
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_masked.py needs a GPU')
    N, rounds = opt('--nodes', 100000), opt('--rounds', 10)
    dev = torch.device('cuda:0')
    result = {'rounds': rounds, 'device': torch.cuda.get_device_name(0), 'rows': []}
    for L, D in SHAPES:
        for dtype in (torch.float32, torch.bfloat16):
            for rate in RATES:
                result['rows'].append(bench(N, L, D, rate, dtype, rounds, dev))
                torch.cuda.empty_cache()
    print(f'{result["device"]}, median of {rounds} rounds (min .. max) in ms, torch composite | fused, and the fused share of 8 TB/s')
    print('| N, L, D | dtype | rate | build torch | build fused | share | loss fwd torch | loss fwd fused | share | '
          'loss bwd torch | loss bwd fused | share |')
    print('|---|---|---|---|---|---|---|---|---|---|---|---|')
    for row in result['rows']:
        cells = []
        for phase in ('build', 'fwd', 'bwd'):
            p = row[phase]
            cells += [f'{p["torch_ms"]:.3f} ({p["torch_min"]:.3f} .. {p["torch_max"]:.3f})',
                      f'{p["fused_ms"]:.3f} ({p["fused_min"]:.3f} .. {p["fused_max"]:.3f})', f'{p["hbm_share"]:.3f}']
        print(f'| {", ".join(map(str, row["shape"]))} | {row["dtype"]} | {row["rate"]} | ' + ' | '.join(cells) + ' |')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
