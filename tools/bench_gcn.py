"""Developer benchmark: the GCN baseline's neighbourhood sum (ampconv_gcn_aggregate) beside the same operation composed
from torch ops on the same GPU in the same process, and a whole GCN training step beside the torch composition with the
materialised input.

    python tools/bench_gcn.py [N E C] [--rmat] [--rounds R] [--no-model]

Without arguments: the Cora shape (2708 / 10556, C = 16), BASELINE config 3's graph (100 k / 1 M uniform) with C = 16 and
C = 64, and config 5's R-MAT graph (2^21 nodes / 40 M edges, C = 16).  Per point, forward (destination-sorted CSR) and
transposed (source-sorted CSC), the median over the rounds of the HIP-event time after 3 warm-up rounds:
    hip:        gcn_aggregate's kernel on a cached EdgeCSR and dinv (what a training step sees after the first layer)
    index_add:  out.index_add_(0, dst, h[src] * w[:, None]) over the edge list after the self-loop step, w precomputed
    sparse.mm:  torch.sparse.mm(A_hat as a CSR tensor, h), A_hat precomputed
and the rate at which the kernel moves its algorithmic bytes, E (4 C + 4) gathered + 2 N 4 C + the pointers.
The model step (forward + backward of GCN(input='embedded') on the full Cora-sized graph, hidden 16) runs beside
    torch: X0 = cat(table, z) [N, F 100] materialised as the reference does, X0 @ W1^T, index_add aggregation, ReLU,
           @ W2^T, aggregation, log_softmax, nll, backward.
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

from ampnet_amd import GCN, EdgeCSR, gcn_norm  # noqa: E402
from ampnet_amd.gcn import _aggregate, zscore_stats  # noqa: E402

POINTS = [('cora', 2708, 10556, 16, False), ('cfg3', 100_000, 1_000_000, 16, False), ('cfg3', 100_000, 1_000_000, 64, False),
          ('cfg5 R-MAT', 1 << 21, 40_000_000, 16, True)]


def opt(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def rmat_edges(scale, E, gen, dev, a=0.57, b=0.19, c=0.19):
    """bench.py's R-MAT edge list (no de-duplication)."""
    src = torch.zeros(E, dtype=torch.int64, device=dev)
    dst = torch.zeros(E, dtype=torch.int64, device=dev)
    for _ in range(scale):
        r = torch.rand(E, generator=gen, device=dev)
        src = src * 2 + (r >= a + b).to(torch.int64)
        dst = dst * 2 + (((r >= a) & (r < a + b)) | (r >= a + b + c)).to(torch.int64)
    return torch.stack([src, dst])


def median_ms(fn, rounds):
    for _ in range(3):
        fn()
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def torch_operator(ei, N, dinv):
    """(src, dst, w) after the self-loop step, and A_hat / its transpose as CSR tensors (None where torch refuses)."""
    keep = ei[0] != ei[1]
    loops = torch.arange(N, device=ei.device)
    src, dst = torch.cat([ei[0][keep], loops]), torch.cat([ei[1][keep], loops])
    w = dinv[src] * dinv[dst]
    try:
        A = torch.sparse_coo_tensor(torch.stack([dst, src]), w, (N, N)).coalesce()
        return src, dst, w, A.to_sparse_csr(), A.t().coalesce().to_sparse_csr()
    except Exception as e:                                            # the comparison is a side measurement
        print(f'torch.sparse refused: {e}', file=sys.stderr)
        return src, dst, w, None, None


def bench_point(name, N, E, C, rmat, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(1234)
    ei = rmat_edges(N.bit_length() - 1, E, g, dev) if rmat else torch.randint(0, N, (2, E), generator=g, device=dev)
    csr = EdgeCSR(ei, N)
    dinv = gcn_norm(csr)
    h = torch.randn(N, C, generator=g, device=dev)
    src, dst, w, A, At = torch_operator(ei, N, dinv)
    indeg, outdeg = (csr.rowptr[1:] - csr.rowptr[:-1]).float(), (csr.cscptr[1:] - csr.cscptr[:-1]).float()
    row = {'point': name, 'N': N, 'E': E, 'C': C,
           'segments': {'in median': float(indeg.median()), 'in max': int(indeg.max()), 'out median': float(outdeg.median()),
                        'out max': int(outdeg.max())}}
    nbytes = E * (4 * C + 4) + 2 * N * 4 * C + 4 * (N + 1)
    for side, a, b, M in (('forward', dst, src, A), ('transposed', src, dst, At)):
        r = {'hip_ms': median_ms(lambda: _aggregate(h, csr, 'dst' if side == 'forward' else 'src', dinv, True, 1.0, None), rounds),
             'index_add_ms': median_ms(lambda: torch.zeros(N, C, device=dev).index_add_(0, a, h[b] * w[:, None]), rounds),
             'sparse_mm_ms': None if M is None else median_ms(lambda: torch.sparse.mm(M, h), rounds)}
        best = min(v for v in (r['index_add_ms'], r['sparse_mm_ms']) if v is not None)
        r.update(bytes=nbytes, GBps=nbytes / r['hip_ms'] / 1e6, hip_over_best_torch=r['hip_ms'] / best)
        row[side] = r
    # the two routes compute the same thing
    ref = torch.zeros(N, C, device=dev).index_add_(0, dst, h[src] * w[:, None])
    row['max_abs_diff_vs_index_add'] = float((_aggregate(h, csr, 'dst', dinv, True, 1.0, None) - ref).abs().max())
    return row


def bench_model(rounds, dev, N=2708, E=10556, Fdim=1433, De=99, hidden=16, C=7):
    import types
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(N, Fdim, generator=g) < 0.0127).float()
    x[torch.arange(N), torch.randint(0, Fdim, (N,), generator=g)] = 1.0
    data = types.SimpleNamespace(x=x.to(dev), edge_index=torch.randint(0, N, (2, E), generator=g).to(dev),
                                 y=torch.randint(0, C, (N,), generator=g).to(dev))
    torch.manual_seed(0)
    m = GCN(dev, Fdim, hidden, Fdim, C, feat_emb_dim=De, dropout_rate=0.0, dropout_adj_rate=0.0).to(dev).train()
    params = list(m.parameters())

    def hip_step():
        for p in params:
            p.grad = None
        F.nll_loss(m(data), data.y).backward()

    csr = EdgeCSR(data.edge_index, N)
    src, dst, w, _, _ = torch_operator(data.edge_index, N, gcn_norm(csr))
    table, W1, b1, W2, b2 = m.feature_embedding_table.weight, m.conv1.lin.weight, m.conv1.bias, m.conv2.lin.weight, m.conv2.bias

    def agg(t):
        return torch.zeros_like(t).index_add_(0, dst, t[src] * w[:, None])

    def torch_step():
        for p in params:
            p.grad = None
        mean, inv_std = zscore_stats(data.x)
        z = (data.x - mean) * inv_std
        X0 = torch.cat([table.unsqueeze(0).expand(N, Fdim, De), z.unsqueeze(-1)], dim=2).reshape(N, Fdim * (De + 1))
        a = torch.relu(agg(X0 @ W1.t()) + b1)
        F.nll_loss(F.log_softmax(agg(a @ W2.t()) + b2, dim=1), data.y).backward()

    out = {'shape': [N, E, Fdim, De, hidden, C], 'hip_ms': median_ms(hip_step, rounds)}
    g_hip = [p.grad.clone() for p in params]
    out['torch_materialised_ms'] = median_ms(torch_step, max(3, rounds // 4))
    out['max_rel_grad_diff'] = max(float((p.grad - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(params, g_hip))
    out['hip_over_torch'] = out['hip_ms'] / out['torch_materialised_ms']
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_gcn.py needs a GPU')
    dev = torch.device('cuda:0')
    args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith('--') and sys.argv[i - 1] != '--rounds']
    rounds = opt('--rounds', 20)
    points = [('custom', *(int(a) for a in args), '--rmat' in sys.argv)] if len(args) == 3 else POINTS
    result = {'device': torch.cuda.get_device_name(0), 'rounds': rounds, 'rows': []}
    for name, N, E, C, rmat in points:
        result['rows'].append(bench_point(name, N, E, C, rmat, rounds if E < 10_000_000 else max(5, rounds // 4), dev))
        torch.cuda.empty_cache()
    if '--no-model' not in sys.argv:
        result['model_step'] = bench_model(rounds, dev)
    print(f'{result["device"]}, fp32, median of {rounds} rounds')
    print('| point | N / E / C | pass | segments median / max | hip ms | index_add ms | sparse.mm ms | hip / best torch | GB/s |')
    print('|---|---|---|---|---|---|---|---|---|')
    for row in result['rows']:
        for side, key in (('forward', 'in'), ('transposed', 'out')):
            r, s = row[side], row['segments']
            sp = 'refused' if r['sparse_mm_ms'] is None else f'{r["sparse_mm_ms"]:.3f}'
            print(f'| {row["point"]} | {row["N"]} / {row["E"]} / {row["C"]} | {side} | {s[key + " median"]:.0f} / {s[key + " max"]} | '
                  f'{r["hip_ms"]:.3f} | {r["index_add_ms"]:.3f} | {sp} | {r["hip_over_best_torch"]:.3f} | {r["GBps"]:.0f} |')
    if 'model_step' in result:
        ms = result['model_step']
        print(f'model step (N, E, F, De, hidden, C) = {ms["shape"]}: hip {ms["hip_ms"]:.3f} ms, torch with the materialised input '
              f'{ms["torch_materialised_ms"]:.3f} ms, ratio {ms["hip_over_torch"]:.3f}')
    print(json.dumps(result))


if __name__ == '__main__':
    main()
