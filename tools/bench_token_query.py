"""Developer benchmark: AMPConv.forward_token (the last layer computed for the read-out token only) beside the full layer
and a slice, and one AMPGCN training step with and without readout_token_only.

    python tools/bench_token_query.py [--rounds R] [--nodes N] [--edges E] [--skip-model]

In ONE process, per shape, three series alternate round by round:
    full_a   y = layer(x, ei).view(N, L, D)[:, 0];   y.backward(dy)
    token    y = layer.forward_token(x, ei, 0);       y.backward(dy)
    full_b   full_a again -- the two medians of the SAME code give the run-to-run spread a difference has to exceed
Shapes: the AMPGCN class-default layer (L = 40, D = 100, H = 2) in fp32 and bf16, BASELINE config 3's layer (L = 20,
D = 128, H = 4, fp32), on N = 100 000 nodes / E = 1 000 000 random edges; then one AMPGCN(average_pooling_flag=False)
training step (zero_grad, nll_loss, backward, Adam step) at the class defaults, flag off / on / off.
Times are HIP-event times of one forward + backward after 2 warm-up rounds; medians over the rounds (min .. max).
Before any time is printed, y and x.grad of both paths on the timed inputs are compared at the bars of
tests/test_gpu_token_layer.py (fp32: atol 1e-5 + rtol 1e-4 |want|; bf16: 2e-2 of the tensor's scale); a miss ends the run.
Per shape the tool also prints the ALGORITHMIC bytes of the three one-query-token edge passes, computed from the shapes
(token_pass_bytes below), and that byte count over the token call's WHOLE forward + backward time as a share of the 8 TB/s
HBM peak -- the call also runs the projections, so this is a lower bound of the passes' own rate, not a kernel time.
Needs a GPU: there is no CPU fallback.  Prints a markdown table and one JSON line."""
import json
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s, MI355X


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def token_pass_bytes(N, E, n_src, L, D, itemsize):
    """Bytes the three one-query-token passes have to move, from shapes alone: per in-edge the source's K and V tiles
    (forward, destination pass); per row its q / dObar rows in and its O / dQ row out; per source with out-edges its own
    K and V tiles once, per out-edge the destination's q and dObar rows, per node its dK and dV tiles out; the graph's
    index arrays once per pass (int32 pointers and indices, fp32 1 / in-degree)."""
    tile, row = L * D * itemsize, D * itemsize
    fwd = E * 2 * tile + N * 2 * row + 4 * (E + N + 1)
    dst = E * 2 * tile + N * 3 * row + 4 * (E + N + 1)
    src = n_src * 2 * tile + N * 2 * tile + E * 2 * row + 4 * (2 * E + N + 1)
    return {'fwd': fwd, 'dst': dst, 'src': src, 'total': fwd + dst + src}


def full_pass_bytes(N, E, L, D, itemsize):
    """The same count for the full layer's three passes (every query token): two L x D tiles per edge in each pass, the
    source pass reads the destination's Q and dObar tiles instead of rows."""
    tile = L * D * itemsize
    return 3 * E * 2 * tile + N * (2 + 3 + 4) * tile + 4 * (4 * E + 3 * (N + 1))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def held(got, want, bf16, what):
    """max error / tolerance of one tensor at the tests' bars; raises above 1."""
    got, want = got.double(), want.double()
    if bf16:
        tol = 2e-2 * max(1.0, float(want.abs().max())) + 2e-2 * want.abs()
    else:
        tol = 1e-5 + 1e-4 * want.abs()
    used = float(((got - want).abs() / tol).max())
    if not used <= 1.0:
        raise SystemExit(f'bench_token_query: {what} of the token path is outside the bar ({100 * used:.0f} % of it): no time printed')
    return used


def summary(ms):
    return {'ms_median': statistics.median(ms), 'ms_min': min(ms), 'ms_max': max(ms)}


def bench_layer(name, N, ei, L, D, H, dtype, rounds, dev):
    from ampnet_amd import AMPConv
    from ampnet_amd.conv import functional as F_
    bf16 = dtype == torch.bfloat16
    torch.manual_seed(1)
    layer = AMPConv(D, H).to(dev).to(dtype)
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(N, L * D, device=dev, generator=g).to(dtype).requires_grad_(True)
    dy = torch.randn(N, D, device=dev, generator=g).to(dtype)
    assert F_.token_supported(L, D, H, dtype), 'the fast path has to be what is timed'

    def full():
        x.grad = None
        y = layer(x, ei).view(N, L, D)[:, 0]
        y.backward(dy)
        return y

    def token():
        x.grad = None
        y = layer.forward_token(x, ei, 0)
        y.backward(dy)
        return y

    y_full = full().detach().clone()
    dx_full = x.grad.clone()
    y_tok = token().detach().clone()
    check = {'y': held(y_tok, y_full, bf16, f'{name}: y'), 'x.grad': held(x.grad, dx_full, bf16, f'{name}: x.grad')}
    del y_full, dx_full, y_tok
    ms = {'full_a': [], 'token': [], 'full_b': []}
    for r in range(rounds + 2):                                       # alternating; the first two rounds are warm-up
        for series, fn in (('full_a', full), ('token', token), ('full_b', full)):
            t, _ = timed(fn)
            if r >= 2:
                ms[series].append(t)
    row = {k: summary(v) for k, v in ms.items()}
    E = ei.size(1)
    n_src = int(torch.unique(ei[0]).numel())
    nbytes = token_pass_bytes(N, E, n_src, L, D, x.element_size())
    row.update(shape=[N, E, L, D, H], dtype=str(dtype).split('.')[-1], bar_used=check, token_pass_bytes=nbytes,
               full_pass_bytes=full_pass_bytes(N, E, L, D, x.element_size()),
               token_bytes_over_call_time_share_of_hbm_peak=nbytes['total'] / (row['token']['ms_median'] * 1e-3) / HBM_PEAK,
               spread_ms=abs(row['full_a']['ms_median'] - row['full_b']['ms_median']),
               gain_ms=min(row['full_a']['ms_median'], row['full_b']['ms_median']) - row['token']['ms_median'])
    row['faster_by_more_than_spread'] = row['gain_ms'] > row['spread_ms']
    return row


def bench_model(N, ei, rounds, dev, feats=256, classes=7):
    from ampnet_amd import AMPGCN
    g = torch.Generator(device=dev).manual_seed(3)
    x = (torch.rand(N, feats, device=dev, generator=g) < 0.2).float()
    x[torch.arange(N, device=dev), torch.randint(0, feats, (N,), device=dev, generator=g)] = 1.0
    data = types.SimpleNamespace(x=x, edge_index=ei, y=torch.randint(0, classes, (N,), device=dev, generator=g))
    steps = {}
    for series, flag in (('plain_a', False), ('token', True), ('plain_b', False)):
        torch.manual_seed(4)
        model = AMPGCN(device=dev, num_node_features=feats, output_dim=classes, average_pooling_flag=False,
                       readout_token_only=flag).to(dev).train()
        optim = torch.optim.Adam(model.parameters(), lr=1e-3)

        def step(model=model, optim=optim):
            optim.zero_grad(set_to_none=True)
            loss = model.nll_loss(data)
            loss.backward()
            optim.step()
            return loss
        steps[series] = step
    ms = {k: [] for k in steps}
    for r in range(rounds + 2):
        for series, fn in steps.items():
            t, _ = timed(fn)
            if r >= 2:
                ms[series].append(t)
    row = {k: summary(v) for k, v in ms.items()}
    row.update(shape=[N, ei.size(1), 40, 100, 2], features=feats,
               spread_ms=abs(row['plain_a']['ms_median'] - row['plain_b']['ms_median']),
               gain_ms=min(row['plain_a']['ms_median'], row['plain_b']['ms_median']) - row['token']['ms_median'])
    row['faster_by_more_than_spread'] = row['gain_ms'] > row['spread_ms']
    return row


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_token_query.py needs a GPU (no CPU fallback)')
    dev = torch.device('cuda:0')
    rounds, N, E = opt('--rounds', 7), opt('--nodes', 100_000), opt('--edges', 1_000_000)
    ei = torch.randint(0, N, (2, E), device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    result = {'rounds': rounds, 'layers': {}}
    for name, (L, D, H, dtype) in {'ampgcn_default_f32': (40, 100, 2, torch.float32),
                                   'ampgcn_default_bf16': (40, 100, 2, torch.bfloat16),
                                   'cfg3_f32': (20, 128, 4, torch.float32)}.items():
        result['layers'][name] = bench_layer(name, N, ei, L, D, H, dtype, rounds, dev)
        torch.cuda.empty_cache()
    if '--skip-model' not in sys.argv:
        result['ampgcn_step'] = bench_model(N, ei, rounds, dev)
    print(f'N = {N}, E = {E}, median of {rounds} rounds (min .. max), forward + backward, ms')
    print('| case | full + slice (a) | full + slice (b) | spread | forward_token | gain | > spread | token-pass GB | share of 8 TB/s |')
    print('|---|---|---|---|---|---|---|---|---|')
    fmt = lambda s: f'{s["ms_median"]:.2f} ({s["ms_min"]:.2f} .. {s["ms_max"]:.2f})'
    for name, r in result['layers'].items():
        print(f'| {name} | {fmt(r["full_a"])} | {fmt(r["full_b"])} | {r["spread_ms"]:.2f} | {fmt(r["token"])} | '
              f'{r["gain_ms"]:.2f} | {r["faster_by_more_than_spread"]} | {r["token_pass_bytes"]["total"] / 1e9:.1f} | '
              f'{r["token_bytes_over_call_time_share_of_hbm_peak"]:.3f} |')
    if 'ampgcn_step' in result:
        r = result['ampgcn_step']
        print(f'| AMPGCN step | {fmt(r["plain_a"])} | {fmt(r["plain_b"])} | {r["spread_ms"]:.2f} | {fmt(r["token"])} | '
              f'{r["gain_ms"]:.2f} | {r["faster_by_more_than_spread"]} | | |')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
