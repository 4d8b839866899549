#!/usr/bin/env python
"""The two figures of the reference's visualization/plot_PCA_2D_plot.py from ampnet_amd.pca: the cumulative
explained-variance-ratio curve and the 2-D component scatter, for

    --of features     data.x transposed, the feature columns as samples (what the reference plots and what its PCA
                      featuriser embeds; ampnet_amd.pca(x, k, samples='columns'): the transpose is never formed)
    --of embeddings   AMPGCN.embed(data), the nodes as samples (samples='rows'); with --pca-table the model's feature
                      table is first set from the PCA of the features (AMPGCN.init_feature_table_from_pca)

on the synthetic Cora-shaped graph of examples/train_graphsaint.py.  The exact solver is used where the reference's
PCA() would pick the randomised one.  Writes cumulative_pca_expl_var_ratio.png and pca_2d.png into --out (matplotlib's
object interface on the Agg canvas, as the diagnostics figures); without matplotlib it prints the numbers only.

    python examples/pca_embeddings.py [--of features|embeddings] [--pca-table] [--out DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from ampnet_amd import AMPGCN, pca  # noqa: E402
from train_graphsaint import synthetic_cora  # noqa: E402


def figures(fit, title, out):
    """cumulative_pca_expl_var_ratio.png (plot_PCA_cumulative_expl_var_ratio) and pca_2d.png (plot_PCA_2D)."""
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError:
        print('matplotlib is not installed: no figures written')
        return
    os.makedirs(out, exist_ok=True)
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot()
    ax.set_title('Cumulative PCA Explained Variance Ratio')
    ax.plot(fit.all_explained_variance_ratio.cumsum(0).cpu().numpy())
    ax.set_xlabel('number of components')
    ax.set_ylabel('cumulative explained variance')
    fig.savefig(os.path.join(out, 'cumulative_pca_expl_var_ratio.png'), facecolor='white', bbox_inches='tight')
    fig = Figure()
    FigureCanvasAgg(fig)
    ax = fig.add_subplot()
    ax.set_title(title)
    scores = fit.scores.cpu().numpy()
    ax.scatter(scores[:, 0], scores[:, 1], s=6)
    ax.set_xlabel('First Component')
    ax.set_ylabel('Second Component')
    fig.savefig(os.path.join(out, 'pca_2d.png'), facecolor='white', bbox_inches='tight')
    print(f'wrote cumulative_pca_expl_var_ratio.png and pca_2d.png to {out}')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--of', choices=('features', 'embeddings'), default='features')
    ap.add_argument('--pca-table', action='store_true',
                    help='with --of embeddings: the feature table of the model is the PCA scores of the feature columns')
    ap.add_argument('--out', default='pca_figures', metavar='DIR')
    args = ap.parse_args(argv)
    if args.pca_table and args.of != 'embeddings':
        ap.error('--pca-table belongs to --of embeddings')
    device = torch.device('cuda:0')
    torch.manual_seed(1)
    data = synthetic_cora(device)
    if args.of == 'features':
        fit = pca(data.x, 2, samples='columns')
        title = 'Feature PCA Embedding 2D Plot'
    else:
        D, H, L = 128, 4, 20
        model = AMPGCN(device=device, embedding_dim=D, num_heads=H, num_node_features=1433, num_sampled_vectors=L, output_dim=7,
                       feat_emb_dim=D - 1, val_emb_dim=1, dropout_rate=0.0, dropout_adj_rate=0.0).to(device)
        if args.pca_table:
            model.init_feature_table_from_pca(data.x, freeze=True)
        model.eval()
        with torch.no_grad():
            z = model.embed(data)
        fit = pca(z.detach(), 2, samples='rows')
        title = 'Node Embedding PCA 2D Plot'
    cum = fit.all_explained_variance_ratio.cumsum(0)
    half = int((cum < 0.5).sum()) + 1
    print(f'{args.of}: {fit.scores.size(0)} samples of {fit.mean.numel()} features; the first two components hold '
          f'{float(fit.explained_variance_ratio.sum()):.1%} of the variance, {half} components hold half of it')
    figures(fit, title, args.out)


if __name__ == '__main__':
    main()
