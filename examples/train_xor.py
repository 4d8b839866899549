#!/usr/bin/env python3
"""The reference's synthetic XOR benchmark with its graph built on the device: duplicated-XOR node features
(synthetic_benchmark/synthetic_xor.py:24-60), their k-nearest-neighbour graph by ampnet_amd.knn_graph in place of
scikit-learn's NearestNeighbors, an [N, N] adjacency matrix and two Python loops (:69-101), and the model of
xor_training_utils.py:58-72 trained full-batch.

    python examples/train_xor.py [--nodes 400] [--neighbours 10] [--noise 0.1] [--epochs 200]
    python examples/train_xor.py --graph links [--same-prob 0.7] [--diff-prob 0.1]

--graph links: the reference's other XOR data, create_xor_data (:104-165) -- every ordered pair of nodes linked with
same_class_link_prob or diff_class_link_prob -- drawn on the device by ampnet_amd.xor_link_dataset in place of its
loops over an [N, N] matrix.

feature_repeats is 1, the value the reference's factory works with: it sets num_node_features = 2 feature_repeats next to
num_sampled_vectors = 2, which its full-width token branch takes only when the two agree.
"""
import argparse
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ampnet_amd import AMPGCN, knn_graph, xor_link_dataset  # noqa: E402

FEATURE_REPEATS = 1


def duplicated_xor(n, noise_std, k, device, gen):
    """x [n, 2 FEATURE_REPEATS], y [n] and the (k + 1)-nearest-neighbour graph (Euclidean, the node itself included)."""
    if n % 4:
        raise ValueError('the number of nodes has to be divisible by 4 (balanced XOR classes)')
    corners = torch.tensor([[0., 0.], [0., 1.], [1., 0.], [1., 1.]], device=device)
    x = corners.repeat_interleave(n // 4, dim=0).repeat(1, FEATURE_REPEATS)
    y = torch.tensor([0, 1, 1, 0], device=device).repeat_interleave(n // 4)
    x = x + noise_std * torch.randn(x.shape, generator=gen, device=device)
    return types.SimpleNamespace(x=x, y=y, edge_index=knn_graph(x, k), num_nodes=n)


def xor_links(n, noise_std, same_prob, diff_prob, device, seed):
    """create_xor_data's x, y and directed link graph (feature_repeats 1), y as class indices."""
    d = xor_link_dataset(n, noise_std, same_prob, diff_prob, seed=seed, device=device)
    return types.SimpleNamespace(x=d.x, y=d.y.long(), edge_index=d.edge_index, num_nodes=n)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=400)
    ap.add_argument('--neighbours', type=int, default=10)
    ap.add_argument('--noise', type=float, default=0.1)
    ap.add_argument('--epochs', type=int, default=200)
    ap.add_argument('--graph', choices=('knn', 'links'), default='knn')
    ap.add_argument('--same-prob', type=float, default=0.7, help='--graph links: same_class_link_prob')
    ap.add_argument('--diff-prob', type=float, default=0.1, help='--graph links: diff_class_link_prob')
    args = ap.parse_args(argv)
    device = torch.device('cuda:0')
    torch.manual_seed(0)
    gen = torch.Generator(device=device).manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.time()
    if args.graph == 'links':
        train = xor_links(args.nodes, args.noise, args.same_prob, args.diff_prob, device, seed=0)
        test = xor_links(args.nodes, args.noise, args.same_prob, args.diff_prob, device, seed=1)
    else:
        train = duplicated_xor(args.nodes, args.noise, args.neighbours, device, gen)
        test = duplicated_xor(args.nodes, args.noise, args.neighbours, device, gen)
    torch.cuda.synchronize()
    print(f'two graphs of {args.nodes} nodes x {train.edge_index.size(1)} edges built on the device in '
          f'{1e3 * (time.time() - t0):.1f} ms (first call: library load included)')
    model = AMPGCN(device=device, embedding_dim=3, num_heads=1, num_node_features=2 * FEATURE_REPEATS,
                   num_sampled_vectors=2, output_dim=2, softmax_out=True, feat_emb_dim=2, val_emb_dim=1,
                   downsample_feature_vectors=False, average_pooling_flag=True, dropout_rate=0.0, dropout_adj_rate=0.0,
                   feature_repeats=FEATURE_REPEATS).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    for epoch in range(args.epochs):
        model.train()
        opt.zero_grad()
        out = model(train)
        loss = F.nll_loss(out, train.y)
        loss.backward()
        opt.step()
        if epoch % max(1, args.epochs // 10) == 0 or epoch == args.epochs - 1:
            model.eval()
            with torch.no_grad():
                acc = float((out.argmax(1) == train.y).float().mean())
                test_acc = float((model(test).argmax(1) == test.y).float().mean())
            print(f'epoch {epoch}: loss {loss.detach().item():.4f}, train accuracy {acc:.3f}, test accuracy {test_acc:.3f}', flush=True)
    return test_acc


if __name__ == '__main__':
    main()
