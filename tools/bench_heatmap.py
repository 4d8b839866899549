"""Developer benchmark: the fused attention heatmap (ampconv_attn_heatmap) beside the route without it --
attn_output_weights [E, L, L] followed by a device index_put_(accumulate=True) of sums and counts.

    python tools/bench_heatmap.py [N E L D H] [--select K | --all F] [--iters I]

--select K (default 30): K source and K destination features out of F = 1433; --all F: the full F x F table.
Prints both times (HIP events, warm-up, same process), their ratio and the fused call's fraction of HBM peak for its
algorithmic traffic: Q[d] and K[s] of the contributing edges (2 L D 4 bytes each), 2 L positions per edge, the edge
list and the table once.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ampnet_amd import _lib  # noqa: E402
from ampnet_amd.conv import functional as F_  # noqa: E402

HBM_PEAK = 8.0e12             # bytes / s, MI355X


def timeit(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    flags = ('--select', '--all', '--iters')
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] not in flags]
    N, E, L, D, H = (int(x) for x in args) if len(args) == 5 else (100000, 1000000, 20, 128, 8)
    iters = opt('--iters', 5)
    F = opt('--all', 1433)
    dev = torch.device('cuda:0')
    lib = _lib.load()
    torch.manual_seed(0)
    dh = D // H
    qkv = torch.randn(N * L, 3 * D, device=dev)
    ei = torch.randint(0, N, (2, E), device=dev)
    tok = torch.randint(0, F, (N, L), device=dev)
    if '--all' in sys.argv:
        src = dst = torch.arange(F, device=dev)
    else:
        K = opt('--select', 30)
        src, dst = torch.randperm(F, device=dev)[:K], torch.randperm(F, device=dev)[:K]
    rows, cols = src.numel(), dst.numel()
    pos = []
    for feats in (src, dst):
        m = torch.full((F,), -1, dtype=torch.int32, device=dev)
        m[feats] = torch.arange(feats.numel(), dtype=torch.int32, device=dev)
        pos.append(m)
    rowpos, colpos = pos[0][tok].contiguous(), pos[1][tok].contiguous()
    Qv, Kv = F_._view(qkv, 0, L, dh), F_._view(qkv, D, L, dh)
    tsum = torch.zeros(rows, cols, dtype=torch.int64, device=dev)
    tcnt = torch.zeros(rows, cols, dtype=torch.int64, device=dev)

    def fused():
        tsum.zero_()
        tcnt.zero_()
        _lib.check(lib.ampconv_attn_heatmap(Qv, Kv, ei.data_ptr(), E, N, None, rowpos.data_ptr(), colpos.data_ptr(), L, D,
                                            H, rows, cols, tsum.data_ptr(), tcnt.data_ptr(), 0, _lib.AMPCONV_F32,
                                            F_._stream()), 'ampconv_attn_heatmap')

    fsum = torch.zeros(rows * cols, dtype=torch.float32, device=dev)
    fcnt = torch.zeros(rows * cols, dtype=torch.int64, device=dev)

    def unfused(chunk=1 << 16):
        # attn_output_weights, then a scatter of every selected (edge, i, j): in chunks of edges so that the index
        # tensors stay small (the [E, L, L] weights alone are E L^2 4 bytes)
        fsum.zero_()
        fcnt.zero_()
        W = F_.attention_weights(Qv, Kv, ei, L, D, H)
        for e0 in range(0, E, chunk):
            e = ei[:, e0:e0 + chunk]
            r = rowpos[e[0]].to(torch.int64)[:, None, :]             # [e, 1, j]
            c = colpos[e[1]].to(torch.int64)[:, :, None]             # [e, i, 1]
            ok = (r >= 0) & (c >= 0)
            cell = (r * cols + c)[ok]
            w = W[e0:e0 + chunk][ok]
            fsum.index_put_((cell,), w, accumulate=True)
            fcnt.index_put_((cell,), torch.ones_like(cell), accumulate=True)

    t_f = timeit(fused, iters)
    t_u = timeit(unfused, max(1, iters // 2), warm=1)
    heat_f = (tsum.double() / (1 << 28) / tcnt.clamp(min=1).double()).reshape(-1)
    heat_u = (fsum.double() / fcnt.clamp(min=1).double())
    assert torch.equal(tcnt.reshape(-1), fcnt), 'counts differ'
    err = float((heat_f - heat_u).abs().max())
    contrib = int(((rowpos[ei[0]] >= 0).any(1) & (colpos[ei[1]] >= 0).any(1)).sum())
    nbytes = contrib * 2 * L * D * 4 + E * (2 * L * 4 + 16) + rows * cols * 16
    print(f'N={N} E={E} L={L} D={D} H={H} table={rows}x{cols} contributing_edges={contrib}')
    print(f'fused {t_f:.3f} ms | attn_output_weights + index_put_ {t_u:.3f} ms | ratio fused/unfused {t_f / t_u:.4f} | '
          f'algorithmic {nbytes / 1e9:.3f} GB -> {nbytes / (t_f * 1e-3) / 1e12:.3f} TB/s = '
          f'{nbytes / (t_f * 1e-3) / HBM_PEAK:.3f} of HBM peak | max |heat diff| {err:.2e}')


if __name__ == '__main__':
    main()
