#!/usr/bin/env python
"""The figures of the reference's visualization/UMAP_testing.ipynb from ampnet_amd.umap: the 2-D UMAP scatter at
`n_neighbors=15, min_dist=0.1`, the notebook's sweeps over n_neighbors and min_dist, and its one 3-D figure, for the
synthetic XOR data of examples/train_xor.py -- no dataset is downloaded:

    default      AMPGCN.embed(data) of the XOR model after a short training, the nodes as samples (samples='rows')
    --columns    data.x with the feature columns as samples, the reference's featuriser view `fit_transform(x.T)`
                 (ampnet_amd.umap(x, samples='columns'): the transpose is never formed); the XOR features are repeated so
                 that there are enough columns for the neighbourhoods

Writes umap_2d.png, umap_n_neighbors.png, umap_min_dist.png and umap_3d.png into --out (matplotlib's object interface on
the Agg canvas); without matplotlib it prints the numbers only.

    python examples/umap_embeddings.py [--columns] [--nodes 400] [--epochs 100] [--seed 0] [--out DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ampnet_amd import AMPGCN, neighbor_preservation, umap  # noqa: E402
import train_xor  # noqa: E402

NEIGHBORS, MIN_DISTS = (5, 15, 30), (0.0, 0.1, 0.5, 0.99)          # the notebook's sweeps, cut to what 64 columns allow


def figures(panels, out):
    """panels: {file name: [(title, embedding [M, 2 or 3]), ...]}; one row of axes per file."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        print('matplotlib is not installed: no figures written')
        return
    os.makedirs(out, exist_ok=True)
    for name, (labels, items) in panels.items():
        fig = Figure(figsize=(4 * len(items), 4))
        FigureCanvasAgg(fig)
        for i, (title, y) in enumerate(items):
            y = y.cpu().numpy()
            three = y.shape[1] == 3
            ax = fig.add_subplot(1, len(items), i + 1, projection='3d' if three else None)
            ax.set_title(title)
            ax.scatter(*(y[:, c] for c in range(y.shape[1])), s=6, c=labels.cpu().numpy())
            ax.set_xlabel('UMAP 1')
            ax.set_ylabel('UMAP 2')
        fig.savefig(os.path.join(out, name), facecolor='white', bbox_inches='tight')
    print(f'wrote {", ".join(panels)} to {out}')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--columns', action='store_true', help="the feature columns as samples (the reference's x.T)")
    ap.add_argument('--nodes', type=int, default=400)
    ap.add_argument('--epochs', type=int, default=100)
    ap.add_argument('--seed', type=int, default=0, help='seed of the negative samples')
    ap.add_argument('--out', default='umap_figures', metavar='DIR')
    args = ap.parse_args(argv)
    device = torch.device('cuda:0')
    torch.manual_seed(0)
    gen = torch.Generator(device=device).manual_seed(0)
    data = train_xor.duplicated_xor(args.nodes, 0.1, 10, device, gen)
    if args.columns:
        rows = min(args.nodes, 256)                    # neighbor_preservation below takes the columns as rows of <= 256 features
        x = (data.x[:rows].repeat(1, 32) + 0.05 * torch.randn(rows, 64, generator=gen, device=device)).contiguous()
        kw, rows_of = dict(samples='columns'), x.t().contiguous()
        what, labels = 'Feature', torch.arange(64, device=device) % 2
    else:
        R = train_xor.FEATURE_REPEATS
        model = AMPGCN(device=device, embedding_dim=3, num_heads=1, num_node_features=2 * R, num_sampled_vectors=2, output_dim=2,
                       softmax_out=True, feat_emb_dim=2, val_emb_dim=1, downsample_feature_vectors=False,
                       average_pooling_flag=True, dropout_rate=0.0, dropout_adj_rate=0.0, feature_repeats=R).to(device)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        for _ in range(args.epochs):
            opt.zero_grad()
            F.nll_loss(model(data), data.y).backward()
            opt.step()
        model.eval()
        with torch.no_grad():
            x = model.embed(data).detach().float().contiguous()
        kw, rows_of, what, labels = dict(samples='rows'), x, 'Node Embedding', data.y
    fit = umap(x, n_neighbors=15, min_dist=0.1, seed=args.seed, **kw)
    kept = neighbor_preservation(rows_of, fit.embedding, 10)
    print(f'{fit.embedding.size(0)} samples: {fit.n_epochs} epochs, a = {fit.a:.4f}, b = {fit.b:.4f}, {fit.graph[1].numel()} entries in '
          f'the fuzzy graph, median sigma {float(fit.sigma.median()):.3g}; {kept:.1%} of the 10 nearest neighbours are kept')
    panels = {'umap_2d.png': (labels, [(f'{what} UMAP 2D Plot', fit.embedding)])}
    sweep = []
    for k in NEIGHBORS:
        y = umap(x, n_neighbors=k, seed=args.seed, **kw).embedding
        sweep.append((f'n_neighbors = {k}', y))
        print(f'n_neighbors {k}: {neighbor_preservation(rows_of, y, 10):.1%} kept')
    panels['umap_n_neighbors.png'] = (labels, sweep)
    sweep = []
    for d in MIN_DISTS:
        y = umap(x, min_dist=d, seed=args.seed, **kw).embedding
        sweep.append((f'min_dist = {d}', y))
        print(f'min_dist {d}: {neighbor_preservation(rows_of, y, 10):.1%} kept')
    panels['umap_min_dist.png'] = (labels, sweep)
    # the 3-d figure needs a start with three columns: PCA gives them if x has three features, else a seeded random start
    M = fit.embedding.size(0)
    init = 'pca' if min(x.shape) >= 3 else torch.randn(M, 3, generator=gen, device=device)
    panels['umap_3d.png'] = (labels, [(f'{what} UMAP 3D Plot', umap(x, 3, seed=args.seed, init=init, **kw).embedding)])
    figures(panels, args.out)


if __name__ == '__main__':
    main()
