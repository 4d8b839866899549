"""Feature-to-feature attention heatmap of a (here untrained) AMPGCN on a synthetic Cora-shaped graph: the flow of the
reference's experiments/visualize_cora_attn_coeffs.py without its plots.

    python examples/attention_heatmap.py [--out DIR] [--src-class A] [--dst-class B]

Runs the model once, takes the 30 most present features of the two classes and writes heatmap_arr_raw.npy [30, 30]
(rows = source features, columns = destination features) -- accumulated on the GPU by AMPGCN.attention_heatmap, the
[E, L, L] attention weights are never formed.  Plotting is left to the reader (seaborn.heatmap(np.load(...))).
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ampnet_amd import AMPGCN, top_features  # noqa: E402


def synthetic_cora(num_nodes=2708, num_features=1433, num_classes=7, num_edges=10556, seed=0):
    """Binary bag-of-words features whose frequent words depend on the class, and random edges that mostly stay inside
    a class (the shape of Planetoid/Cora, which this example does not download)."""
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, num_classes, (num_nodes,), generator=g)
    base = torch.rand(num_classes, num_features, generator=g) ** 8 * 0.3 + 0.005
    x = (torch.rand(num_nodes, num_features, generator=g) < base[y]).float()
    x[torch.arange(num_nodes), torch.randint(0, num_features, (num_nodes,), generator=g)] = 1.0   # no empty node
    src = torch.randint(0, num_nodes, (num_edges,), generator=g)
    same = torch.rand(num_edges, generator=g) < 0.8
    order = torch.argsort(y)
    start = torch.searchsorted(y[order], torch.arange(num_classes))
    size = torch.bincount(y, minlength=num_classes)
    inside = order[start[y[src]] + (torch.rand(num_edges, generator=g) * size[y[src]]).long().clamp(max=num_nodes - 1)]
    dst = torch.where(same, inside, torch.randint(0, num_nodes, (num_edges,), generator=g))
    return x, torch.stack([src, dst]), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='.')
    ap.add_argument('--src-class', type=int, default=0)
    ap.add_argument('--dst-class', type=int, default=1)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    x, edge_index, y = synthetic_cora()
    torch.manual_seed(0)
    model = AMPGCN(device=dev, embedding_dim=128, num_heads=4, num_node_features=x.size(1), num_sampled_vectors=20,
                   output_dim=7, feat_emb_dim=127, val_emb_dim=1, dropout_rate=0.0, dropout_adj_rate=0.0).to(dev)
    model.eval()
    data = types.SimpleNamespace(x=x.to(dev), edge_index=edge_index.to(dev))
    with torch.no_grad():
        model(data)
    src = top_features(data.x, y.to(dev), a.src_class, k=30)
    dst = top_features(data.x, y.to(dev), a.dst_class, k=30)
    heat = model.attention_heatmap('conv1', src, dst, node_class=y, src_class=a.src_class, dst_class=a.dst_class)
    path = os.path.join(a.out, 'heatmap_arr_raw.npy')
    np.save(path, heat.cpu().numpy())
    print(f'{path}: {tuple(heat.shape)}, {int((heat != 0).sum())} non-zero cells, max {float(heat.max()):.4f}')


if __name__ == '__main__':
    main()
