#!/usr/bin/env python3
"""Masked feature modelling: the predictive self-supervised step the reference announces and leaves empty
(synthetic_benchmark/predictive_ssl_AMPNet.py, `criterion = None`), on the duplicated-XOR data of examples/train_xor.py.

    python examples/train_masked.py [--nodes 400] [--repeats 5] [--epochs 60] [--rate 0.3] [--mode value|token]
                                    [--graph knn|links] [--bf16]

Every node carries `repeats` noisy copies of its two XOR coordinates (synthetic_xor.py:24-60, feature_repeats = 5), every
copy is a token.  Each epoch hides a fresh share `rate` of the tokens behind the model's mask_token and asks the value
decoder behind conv2 for their z-scored values back (AMPGCN.masked_feature_loss): a hidden value is recoverable from its
copies in the same node, which is what a token-attention layer can learn.  No label is read while training.  FusedAdam steps
the model; the loss is read back once per epoch through MaskedMetrics.  Every few epochs the pooled embeddings
(AMPGCN.embed) are scored by leave-one-out nearest-neighbour classification of the XOR class (knn_classify), and both
curves are printed.

--mode value (default) hides the value and keeps the feature's embedding, so the decoder knows WHICH coordinate it is asked
for; --mode token is the reference's replacement of the whole token vector (gcn_classifier.py:151), under which the two
coordinates of a node can only be told apart by their neighbours' attention.
--graph links: the block-model link graph of create_xor_data (ampnet_amd.xor_link_dataset) in place of the kNN graph.
"""
import argparse
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from ampnet_amd import AMPGCN, FusedAdam, MaskedMetrics, knn_classify, knn_graph, xor_link_dataset  # noqa: E402


def duplicated_xor(n, noise_std, repeats, k, graph, device, seed):
    """x [n, 2 repeats] (the corner's coordinates tiled, independent noise on every copy), y [n] and the graph."""
    if n % 4:
        raise ValueError('the number of nodes has to be divisible by 4 (balanced XOR classes)')
    gen = torch.Generator(device=device).manual_seed(seed)
    corners = torch.tensor([[0., 0.], [0., 1.], [1., 0.], [1., 1.]], device=device)
    x = corners.repeat_interleave(n // 4, dim=0).repeat(1, repeats)
    y = torch.tensor([0, 1, 1, 0], device=device).repeat_interleave(n // 4)
    x = x + noise_std * torch.randn(x.shape, generator=gen, device=device)
    if graph == 'links':                                    # the same four corner groups in the same node order
        edge_index = xor_link_dataset(n, noise_std, 0.7, 0.1, seed=seed, device=device).edge_index
    else:
        edge_index = knn_graph(x, k)
    return types.SimpleNamespace(x=x, y=y, edge_index=edge_index, num_nodes=n)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=400)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--neighbours', type=int, default=10)
    ap.add_argument('--noise', type=float, default=0.1)
    ap.add_argument('--epochs', type=int, default=60)
    ap.add_argument('--rate', type=float, default=0.3)
    ap.add_argument('--mode', choices=('value', 'token'), default='value')
    ap.add_argument('--graph', choices=('knn', 'links'), default='knn')
    ap.add_argument('--bf16', action='store_true', help='AMPGCN(storage_dtype=torch.bfloat16)')
    args = ap.parse_args(argv)
    device = torch.device('cuda:0')
    torch.manual_seed(0)
    data = duplicated_xor(args.nodes, args.noise, args.repeats, args.neighbours, args.graph, device, seed=0)
    D = 8
    model = AMPGCN(device=device, embedding_dim=D, num_heads=2, num_node_features=2, num_sampled_vectors=2 * args.repeats,
                   output_dim=2, feat_emb_dim=D - 1, val_emb_dim=1, downsample_feature_vectors=False, dropout_rate=0.0,
                   dropout_adj_rate=0.0, feature_repeats=args.repeats, masked_modelling=True,
                   storage_dtype=torch.bfloat16 if args.bf16 else torch.float32).to(device)
    # final_linear_out is behind the embedding: it gets no gradient here and FusedAdam skips it
    opt = FusedAdam(model.parameters(), lr=0.01)
    metrics = MaskedMetrics(device)

    def knn_accuracy():
        model.eval()
        with torch.no_grad():
            z = model.embed(data).float()
        model.train()
        return float((knn_classify(z, data.y, 5, num_classes=2) == data.y).float().mean())

    print(f'{args.nodes} nodes x {2 * args.repeats} tokens, {data.edge_index.size(1)} edges, mask rate {args.rate}, mode {args.mode}')
    print(f'before training: 5-nearest-neighbour accuracy of the embeddings {knn_accuracy():.3f}')
    steps = 10
    curve = []
    torch.cuda.synchronize()
    t0 = time.time()
    for epoch in range(args.epochs):
        model.train()
        metrics.reset()
        for _ in range(steps):
            loss = model.masked_feature_loss(data, mask_rate=args.rate, mask_mode=args.mode, metrics=metrics)
            loss.backward()
            opt.step(set_to_none=True)
        mse = metrics.mse()                                 # the one read-back of the epoch
        if epoch % max(1, args.epochs // 10) == 0 or epoch == args.epochs - 1:
            acc = knn_accuracy()
            curve.append((epoch, mse, acc))
            print(f'epoch {epoch}: masked-value mse {mse:.4f} (of z-scored values: 1.0 = predicting the mean), '
                  f'kNN accuracy {acc:.3f}', flush=True)
    torch.cuda.synchronize()
    print(f'{args.epochs * steps} steps in {time.time() - t0:.1f} s')
    return curve


if __name__ == '__main__':
    main()
