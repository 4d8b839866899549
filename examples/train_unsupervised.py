#!/usr/bin/env python3
"""Unsupervised training of AMPGCN: the step the reference announces and leaves empty (synthetic_benchmark/
contrastive_ssl_AMPNet.py and predictive_ssl_AMPNet.py:79, `criterion = None  # Implement GraphSAGE unsupervised loss
function`), on the synthetic Cora-shaped graph of examples/train_graphsaint.py.  No label is read while training.

    python examples/train_unsupervised.py [--epochs 3] [--steps 20] [--negatives batch|K] [--kind skipgram|xent]
                                          [--window 2] [--bf16]

Loop: GraphSAINT sample() -> _collate -> walk_pairs (the walks the sampler drew ARE the positive pairs) -> model.embed
-> pair_loss -> FusedAdam.  --negatives batch: every node of the batch is a negative of every pair, a pair's own anchor
excluded (the contrastive setting); --negatives K: K uniform draws from the batch (GraphSAGE's 20).  At the end the
embeddings of the whole graph are scored by how often a node's nearest neighbour (cosine) shares its class.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ampnet_amd import AMPGCN, FusedAdam, GraphSAINTRandomWalkSampler, PairLoss, knn_classify, walk_pairs  # noqa: E402
from train_graphsaint import synthetic_cora  # noqa: E402


def neighbour_agreement(z, y):
    """Share of nodes whose nearest other node by cosine similarity has their class (the [N, N] similarities stay on chip)."""
    return float((knn_classify(z, y, 1) == y).float().mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--negatives', default='batch', help="'batch' (every node of the batch, anchors excluded) or a number K")
    ap.add_argument('--kind', choices=('skipgram', 'xent'), default='skipgram')
    ap.add_argument('--window', type=int, default=2, help='pairs (walk[i], walk[i + k]) for k = 1..window')
    ap.add_argument('--bf16', action='store_true', help='AMPGCN(storage_dtype=torch.bfloat16): bf16 embeddings and gradient')
    args = ap.parse_args(argv)
    in_batch = args.negatives == 'batch'
    K = None if in_batch else int(args.negatives)
    device = torch.device('cuda:0')
    torch.manual_seed(1)
    data = synthetic_cora(device)
    D, H, L = 128, 4, 20
    model = AMPGCN(device=device, embedding_dim=D, num_heads=H, num_node_features=1433, num_sampled_vectors=L, output_dim=7,
                   feat_emb_dim=D - 1, val_emb_dim=1, dropout_rate=0.0, dropout_adj_rate=0.0,
                   storage_dtype=torch.bfloat16 if args.bf16 else torch.float32).to(device)
    # final_linear_out is behind the embedding: it gets no gradient here and FusedAdam skips it
    opt = FusedAdam(model.parameters(), lr=0.005, weight_decay=1e-4)
    criterion = PairLoss(kind=args.kind, scale=D ** -0.5, exclude_anchor=in_batch, reduction='mean')
    sampler = GraphSAINTRandomWalkSampler(data, batch_size=8, walk_length=150, num_steps=args.steps, seed=1)
    gen = torch.Generator(device=device).manual_seed(2)
    model.eval()
    with torch.no_grad():
        print(f'before training: nearest-neighbour class agreement {neighbour_agreement(model.embed(data), data.y):.3f}')
    for epoch in range(args.epochs):
        model.train()
        total = torch.zeros((), device=device)
        torch.cuda.synchronize()
        te = time.time()
        for _ in range(args.steps):
            node_idx, edge_index, edge_id, walks = sampler.sample()
            batch = sampler._collate(node_idx, edge_index, edge_id)
            anchors, positives = walk_pairs(walks, node_idx, window=args.window)
            n_sub = node_idx.numel()
            negatives = (torch.arange(n_sub, device=device) if in_batch
                         else torch.randint(0, n_sub, (K,), generator=gen, device=device))
            loss = criterion(model.embed(batch), anchors, positives, negatives)
            loss.backward()
            opt.step(set_to_none=True)
            total += loss.detach()                                              # stays on the device
        torch.cuda.synchronize()
        print(f'epoch {epoch}: {args.kind} loss {float(total) / args.steps:.4f} over {anchors.numel()} pairs x '
              f'{negatives.numel()} negatives per batch ({1e3 * (time.time() - te) / args.steps:.2f} ms per batch)', flush=True)
    model.eval()
    with torch.no_grad():
        score = neighbour_agreement(model.embed(data), data.y)
    print(f'after training: nearest-neighbour class agreement {score:.3f}')
    return score


if __name__ == '__main__':
    main()
