#!/usr/bin/env python
"""The two figures of the reference's visualization/plot_TSNE_2D_plot.py from ampnet_amd.tsne: the 2-D t-SNE scatter of
an embedding and of its z-scored version (StandardScaler), for the synthetic XOR data of examples/train_xor.py -- no
dataset is downloaded:

    default      AMPGCN.embed(data) of the XOR model after a short training, the nodes as samples (samples='rows')
    --columns    data.x with the feature columns as samples, the reference's `TSNE(n_components=2, perplexity=10,
                 learning_rate=10).fit_transform(x.T)` (ampnet_amd.tsne(x, samples='columns'): the transpose is never
                 formed); the XOR features are repeated so that there are enough columns for the perplexity

Writes tsne_2d.png and normalized_tsne_2d.png into --out (matplotlib's object interface on the Agg canvas); without
matplotlib it prints the numbers only.

    python examples/tsne_embeddings.py [--columns] [--nodes 400] [--epochs 100] [--perplexity P] [--out DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ampnet_amd import AMPGCN, neighbor_preservation, tsne  # noqa: E402
import train_xor  # noqa: E402


def figures(fit, title, out, labels=None):
    """tsne_2d.png and normalized_tsne_2d.png (plot_TSNE_2D on the raw and the z-scored embedding)."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        print('matplotlib is not installed: no figures written')
        return
    os.makedirs(out, exist_ok=True)
    for name, head, y in (('tsne_2d.png', title, fit.embedding), ('normalized_tsne_2d.png', 'Normalized ' + title, fit.standardized())):
        fig = Figure()
        FigureCanvasAgg(fig)
        ax = fig.add_subplot()
        ax.set_title(head)
        y = y.cpu().numpy()
        ax.scatter(y[:, 0], y[:, 1], s=6, c=None if labels is None else labels.cpu().numpy())
        ax.set_xlabel('tSNE 1')
        ax.set_ylabel('tSNE 2')
        fig.savefig(os.path.join(out, name), facecolor='white', bbox_inches='tight')
    print(f'wrote tsne_2d.png and normalized_tsne_2d.png to {out}')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--columns', action='store_true', help="the feature columns as samples (the reference's x.T)")
    ap.add_argument('--nodes', type=int, default=400)
    ap.add_argument('--epochs', type=int, default=100)
    ap.add_argument('--perplexity', type=float, default=None, help='default: 30 for the nodes, 10 (the reference) for --columns')
    ap.add_argument('--out', default='tsne_figures', metavar='DIR')
    args = ap.parse_args(argv)
    device = torch.device('cuda:0')
    torch.manual_seed(0)
    gen = torch.Generator(device=device).manual_seed(0)
    data = train_xor.duplicated_xor(args.nodes, 0.1, 10, device, gen)
    if args.columns:
        rows = min(args.nodes, 256)                    # neighbor_preservation below takes the columns as rows of <= 256 features
        x = (data.x[:rows].repeat(1, 32) + 0.05 * torch.randn(rows, 64, generator=gen, device=device)).contiguous()
        fit = tsne(x, perplexity=args.perplexity or 10.0, learning_rate=10, samples='columns')
        title, labels = 'Feature tSNE Embedding 2D Plot', torch.arange(64, device=device) % 2
        k = 5
        kept = neighbor_preservation(x.t().contiguous(), fit.embedding, k)
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
            z = model.embed(data).detach().float().contiguous()
        fit = tsne(z, perplexity=args.perplexity or 30.0)
        title, labels = 'Node Embedding tSNE 2D Plot', data.y
        k = 10
        kept = neighbor_preservation(z, fit.embedding, k)
    print(f'{fit.embedding.size(0)} samples: KL divergence {fit.kl_divergence:.4f} after {fit.n_iter + 1} iterations at learning rate '
          f'{fit.learning_rate:g}; {kept:.1%} of the {k} nearest neighbours are kept; median precision {float(fit.beta.median()):.3g}')
    figures(fit, title, args.out, labels)


if __name__ == '__main__':
    main()
