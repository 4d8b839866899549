#!/usr/bin/env python3
"""The reference's main training harness (experiments/cora_benchmark_graphsaint.py:59-135) on the
MI355X path, on a synthetic Cora-shaped graph (Cora itself is a network download):
AMPGCN(D=128, H=4, L=20) + GraphSAINT random-walk batches + Adam + cosine warm restarts +
node_norm-weighted NLL.  Everything between the data and the loss runs on the GPU.

    python examples/train_graphsaint.py [--epochs 3] [--dropout 0.1 --fused-glue] [--fused-head] [--layer-norm] [--token-readout]
                                        [--fused-adam [--clip M] [--track-grad-norm] [--bf16]] [--diagnostics K [--diag-dir DIR]]
                                        [--model gcn [--gcn-input {embedded,zscore,raw}] [--hidden 16]]

--model gcn trains the baseline behind the reference's `TRAIN_AMPCONV = False` (:27,58-75): the 2-layer GCN of
src/ampnet/module/gcn_classifier.py on the same batches, optimiser, schedule and loss.
"""
import argparse
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ampnet_amd import AMPGCN, GCN, FusedAdam, GraphSAINTRandomWalkSampler, HeadMetrics  # noqa: E402


def synthetic_cora(device, n=2708, f=1433, classes=7, seed=1):
    """Bag-of-words-like features whose present words depend on the class; homophilous edges."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, classes, (n,), generator=g)
    topic = torch.rand(classes, f, generator=g) < 0.03                  # class vocabulary
    x = ((torch.rand(n, f, generator=g) < 0.004) | (topic[y] & (torch.rand(n, f, generator=g) < 0.3))).float()
    x[torch.arange(n), torch.randint(0, f, (n,), generator=g)] = 1.0    # at least one present word
    src = torch.randint(0, n, (5278,), generator=g)
    same = torch.rand(5278, generator=g) < 0.8                           # 80 % intra-class edges
    perm = torch.argsort(y + torch.rand(n, generator=g) * 0.5)
    pos = torch.empty(n, dtype=torch.long); pos[perm] = torch.arange(n)
    near = perm[(pos[src] + torch.randint(1, 40, (5278,), generator=g)).clamp(max=n - 1)]
    dst = torch.where(same, near, torch.randint(0, n, (5278,), generator=g))
    ei = torch.cat([torch.stack([src, dst]), torch.stack([dst, src])], dim=1)   # both directions
    idx = torch.randperm(n, generator=g)
    mask = lambda a, b: torch.zeros(n, dtype=torch.bool).index_fill_(0, idx[a:b], True)
    return types.SimpleNamespace(x=x.to(device), y=y.to(device), edge_index=ei.to(device), num_nodes=n,
                                 train_mask=mask(0, 1400).to(device), test_mask=mask(1400, n).to(device))


def report(epoch, queued, model, diag_dir):
    """The epoch's queued diagnostics: per layer, over the queued batches, mean |grad|, max |grad| and the non-finite
    count; per activation site the dead share of a ReLU (zeros / numel); with diag_dir the reference's three figures for
    the last queued batch."""
    if not queued:
        return
    read = [(i, g.read(), a.read()) for i, g, a in queued]                  # behind the epoch's synchronise: no waiting
    print(f'  diagnostics of epoch {epoch}, batches {[i for i, _, _ in read]}:')
    for name in read[0][1]:
        rows = [g[name] for _, g, _ in read]
        print(f'    {name:48s} mean |grad| {sum(r["absmean"] for r in rows) / len(rows):.3e}  max |grad| '
              f'{max(r["absmax"] for r in rows):.3e}  non-finite {sum(r["nan"] + r["inf"] for r in rows)}')
    for name in read[0][2]:
        rows = [a[name] for _, _, a in read]
        dead = f'  dead {sum(r["zeros"] for r in rows) / max(sum(r["numel"] for r in rows), 1):.1%}' if 'ReLU' in name else ''
        print(f'    {name:48s} mean {sum(r["mean"] for r in rows) / len(rows):+.3e}  std '
              f'{sum(r["std"] for r in rows) / len(rows):.3e}{dead}  non-finite {sum(r["nan"] + r["inf"] for r in rows)}')
    if diag_dir is not None:
        i, g, a = read[-1]
        os.makedirs(diag_dir, exist_ok=True)
        model.plot_grad_flow(diag_dir, epoch, i, stats=g)
        model.visualize_gradients(diag_dir, epoch, i, stats=g)
        model.visualize_activations(diag_dir, None, epoch, i, stats=a)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', choices=('ampgcn', 'gcn'), default='ampgcn',
                    help="gcn: the reference's baseline (TRAIN_AMPCONV = False): GCN(hidden) on the HIP GCN kernels")
    ap.add_argument('--gcn-input', choices=('embedded', 'zscore', 'raw'), default='embedded',
                    help="with --model gcn: the first layer's input -- the reference's cat(embedding table, z-scored value) "
                         '(never formed in memory), the z-scored features alone, or the raw features of the demos')
    ap.add_argument('--hidden', type=int, default=16, help='with --model gcn: hidden_dim (gcn_classifier.py:21)')
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--class-defaults', action='store_true',
                    help="AMPGCN's class defaults (src/ampnet/module/amp_gcn.py:21-35: embedding_dim=100, heads=2, 40 sampled "
                         "vectors: what experiments/cora_benchmark_graphsaint_distributed.py:58 instantiates) instead of the "
                         "128 / 4 / 20 of experiments/cora_benchmark_graphsaint.py")
    ap.add_argument('--dropout', type=float, default=0.0, metavar='P',
                    help='dropout_rate of the model (the reference trains with 0.1, amp_gcn.py:31)')
    ap.add_argument('--fused-glue', action='store_true',
                    help='dropout, ReLU and token pooling around the layers as fused HIP passes (AMPGCN(fused_glue=True))')
    ap.add_argument('--layer-norm', action='store_true',
                    help='per-token LayerNorm behind each layer, fused with ReLU, dropout and the pooling (AMPGCN(layer_norm=True))')
    ap.add_argument('--fused-head', action='store_true',
                    help='Linear + log_softmax + node_norm-weighted NLL + train / test metrics as one HIP kernel per '
                         'direction (AMPGCN(fused_head=True).nll_loss): no read-back per step, one per epoch')
    ap.add_argument('--fused-adam', action='store_true',
                    help='ampnet_amd.FusedAdam instead of torch.optim.Adam: the whole step as one HIP launch, zero_grad() folded '
                         'into it (step(set_to_none=True))')
    ap.add_argument('--clip', type=float, default=None, metavar='M',
                    help='with --fused-adam: clip the global gradient norm to M on the device (FusedAdam(max_grad_norm=M))')
    ap.add_argument('--track-grad-norm', action='store_true',
                    help="with --fused-adam: print the last batch's gradient norm with the epoch's read-back")
    ap.add_argument('--bf16', action='store_true',
                    help='AMPGCN(storage_dtype=torch.bfloat16): the two AMPConv layers and the activations between them in '
                         'bf16 storage, table / norms / head in fp32; needs --fused-adam, which keeps fp32 master weights')
    ap.add_argument('--token-readout', action='store_true',
                    help='read token 0 of conv2 instead of the token mean (average_pooling_flag=False) and compute conv2 for '
                         'that token only: AMPGCN(readout_token_only=True), AMPConv.forward_token')
    ap.add_argument('--diagnostics', type=int, default=0, metavar='K',
                    help="every K-th batch queues the reference's gradient and activation diagnostics (experiments/"
                         'cora_benchmark_graphsaint.py:111-114) as device-side statistics (AMPGCN.gradient_stats / '
                         "activation_stats); they are read and printed with the epoch's one read-back")
    ap.add_argument('--diag-dir', default=None, metavar='DIR',
                    help="with --diagnostics: write the reference's three figures for the last queued batch of every epoch there")
    ap.add_argument('--pca-table', action='store_true',
                    help="the reference's PCA featuriser (amp_gcn.py:185-206): the feature table is the PCA scores of the feature "
                         'columns of data.x (AMPGCN.init_feature_table_from_pca, ampnet_amd.pca), frozen')
    args = ap.parse_args(argv)
    if args.pca_table and args.model == 'gcn':
        ap.error('--pca-table belongs to --model ampgcn')
    if args.diag_dir is not None and args.diagnostics <= 0:
        ap.error('--diag-dir needs --diagnostics K')
    if (args.clip is not None or args.track_grad_norm) and not args.fused_adam:
        ap.error('--clip and --track-grad-norm need --fused-adam')
    if args.bf16 and not args.fused_adam:
        ap.error('--bf16 needs --fused-adam: torch.optim.Adam would step the bf16 parameters themselves, and an update of '
                 'lr * O(1) on a weight near 1 is below half a bf16 ulp -- it is lost at every step; FusedAdam steps fp32 '
                 'master copies and writes the rounded result')
    if args.bf16 and args.model == 'gcn':
        ap.error('--bf16 belongs to --model ampgcn (GCN is float32 only)')
    if args.model == 'gcn' and (args.layer_norm or args.diagnostics > 0 or args.class_defaults or args.token_readout):
        ap.error('--layer-norm, --diagnostics, --class-defaults and --token-readout belong to --model ampgcn')
    device = torch.device('cuda:0')
    torch.manual_seed(1)
    data = synthetic_cora(device)
    D, H, L = (100, 2, 40) if args.class_defaults else (128, 4, 20)
    if args.model == 'gcn':
        model = GCN(device=device, num_node_features=1433, hidden_dim=args.hidden, num_sampled_vectors=1433, output_dim=7,
                    softmax_out=True, feat_emb_dim=99, val_emb_dim=1, dropout_rate=args.dropout, dropout_adj_rate=0.0,
                    input=args.gcn_input, fused_glue=args.fused_glue, fused_head=args.fused_head).to(device)
        what = f'sampler + 2 GCNConv layers ({args.gcn_input} input) fwd+bwd + Adam'
    else:
        model = AMPGCN(device=device, embedding_dim=D, num_heads=H, num_node_features=1433, num_sampled_vectors=L,
                       output_dim=7, softmax_out=True, feat_emb_dim=D - 1, val_emb_dim=1, dropout_rate=args.dropout,
                       dropout_adj_rate=0.0, fused_glue=args.fused_glue, fused_head=args.fused_head,
                       layer_norm=args.layer_norm, average_pooling_flag=not args.token_readout,
                       readout_token_only=args.token_readout,
                       storage_dtype=torch.bfloat16 if args.bf16 else torch.float32).to(device)
        what = 'sampler + 2 AMPConv layers fwd+bwd + Adam' + (', bf16 storage' if args.bf16 else '') + (
            ', conv2 for the read-out token only' if args.token_readout else '')
        if args.pca_table:
            fit = model.init_feature_table_from_pca(data.x, freeze=True)
            print(f'feature table = PCA scores of the {data.x.size(1)} feature columns: {D - 1} components hold '
                  f'{float(fit.explained_variance_ratio.sum()):.1%} of the variance; the table is frozen')
    loader = GraphSAINTRandomWalkSampler(data, batch_size=8, walk_length=150, num_steps=args.steps,
                                         sample_coverage=20, seed=1)
    trained = [p for p in model.parameters() if p.requires_grad]            # (--pca-table freezes the feature table)
    if args.fused_adam:
        opt = FusedAdam(trained, lr=0.005, weight_decay=1e-4, max_grad_norm=args.clip,
                        track_grad_norm=args.track_grad_norm)
        zero_grad, step = (lambda: None), (lambda: opt.step(set_to_none=True))
    else:
        opt = torch.optim.Adam(trained, lr=0.005, weight_decay=1e-4)
        zero_grad, step = opt.zero_grad, opt.step
    sched = torch.optim.lr_scheduler.CosineAnnealingWarmRestarts(opt, T_0=400, T_mult=2)
    t0 = time.time()
    history = []
    metrics = HeadMetrics(2, device) if args.fused_head else None

    def diagnose(queue, batch, i):                                          # after backward(), before the step
        if args.diagnostics > 0 and i % args.diagnostics == 0:
            queue.append((i, model.gradient_stats(), model.activation_stats(batch)))

    for epoch in range(args.epochs):
        tot = cnt = correct = 0
        queued = []
        torch.cuda.synchronize()
        te = time.time()
        if args.fused_head:
            metrics.zero_()
            for batch in loader:
                model.train()
                zero_grad()
                model.nll_loss(batch, masks=(batch.train_mask, batch.test_mask), metrics=metrics).backward()
                diagnose(queued, batch, cnt)
                step()
                sched.step()
                cnt += 1
            m = metrics.read()                                              # the epoch's one read-back
            tot, correct = m['loss_sum'][0], cnt * m['correct'][0] / max(m['count'][0], 1)    # accuracy over the epoch's nodes
            extra = (f'  test loss {m["loss_sum"][1] / cnt:.4f}  test acc {m["correct"][1] / max(m["count"][1], 1):.3f}'
                     + (f'  ({m["bad_labels"]} labels out of range)' if m['bad_labels'] else ''))
        else:
            extra = ''
            for batch in loader:
                model.train()
                zero_grad()
                out = model(batch)
                loss = (F.nll_loss(out, batch.y, reduction='none') * batch.node_norm)[batch.train_mask].sum()
                loss.backward()
                diagnose(queued, batch, cnt)
                step()
                sched.step()
                tot += loss.item(); cnt += 1
                correct += float((out.argmax(1) == batch.y)[batch.train_mask].float().mean())
        if args.fused_adam and opt.grad_norm is not None:
            extra += f'  grad norm {float(opt.grad_norm):.4f}'                   # after the epoch's read-back: no extra wait
        history.append((tot / cnt, correct / cnt))
        torch.cuda.synchronize()
        report(epoch, queued, model, args.diag_dir)
        print(f'epoch {epoch}: train loss {tot / cnt:.4f}  train acc {correct / cnt:.3f}{extra}  '
              f'({time.time() - t0:.1f} s; this epoch {time.time() - te:.3f} s = {1e3 * (time.time() - te) / cnt:.2f} ms '
              f'per sampled batch, {what})', flush=True)
    model.eval()
    with torch.no_grad():
        out = model(data)                                                   # full-graph eval (:159-163)
        acc = float((out.argmax(1) == data.y)[data.test_mask].float().mean())
    print(f'full-graph test accuracy {acc:.3f}')
    main.last_run = (model, opt)                                            # for callers that look at the trained state
    return history, acc


if __name__ == '__main__':
    main()
