#!/usr/bin/env python
"""The reference's two pictures of a graph from ampnet_amd.spring_layout -- no networkx, no dataset download:

    xor_graph.png        synthetic_benchmark/synthetic_xor.py's plot_graph: the directed k-nearest-neighbour graph of the
                         duplicated-XOR points (ampnet_amd.knn_graph on examples/train_xor.py's data, the point itself
                         included), nodes coloured by label, same-class edges green, cross-class edges red
    saint_subgraph.png   visualization/visualize_graphsaint_subgraphs.py's nx.draw(to_networkx(batch, to_undirected=True)):
                         one GraphSAINT random-walk sub-graph from the project's sampler, on the synthetic Cora of
                         examples/train_graphsaint.py

Both layouts are networkx's spring_layout (Fruchterman-Reingold, 50 iterations) computed on the device.  Writes the
figures into --out (matplotlib's object interface on the Agg canvas); without matplotlib it prints the numbers only.

    python examples/graph_layout.py [--nodes 40] [--neighbours 5] [--walks 10] [--walk-length 100] [--seed 0] [--out DIR]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from ampnet_amd import GraphSAINTRandomWalkSampler, spring_layout  # noqa: E402
import train_graphsaint  # noqa: E402
import train_xor  # noqa: E402


def edge_length_ratio(pos, edge_index):
    """The mean length of an edge over the mean distance of all pairs: how far the layout pulled the edges together."""
    d = (pos[edge_index[0]] - pos[edge_index[1]]).norm(dim=1)
    keep = edge_index[0] != edge_index[1]
    return float(d[keep].mean() / torch.cdist(pos, pos).mean())


def draw(path, title, pos, edge_index, labels, arrows):
    try:
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.collections import LineCollection
        from matplotlib.figure import Figure
    except ImportError:
        print('matplotlib is not installed: no figure written')
        return
    pos, ei, lab = pos.cpu().numpy(), edge_index.cpu().numpy(), labels.cpu().numpy()
    keep = ei[0] != ei[1]                                                   # a self-loop has no length to draw
    ei = ei[:, keep]
    fig = Figure(figsize=(7, 7))
    FigureCanvasAgg(fig)
    ax = fig.add_subplot(1, 1, 1)
    ax.set_title(title)
    same = lab[ei[0]] == lab[ei[1]]
    for colour, pick in (('g', same), ('r', ~same)):                        # plot_graph: green within a class, red across
        seg = [(pos[a], pos[b]) for a, b in ei[:, pick].T]
        ax.add_collection(LineCollection(seg, colors=colour, linewidths=0.6, alpha=0.7))
        if arrows:
            for a, b in ei[:, pick].T:
                ax.annotate('', xy=pos[b], xytext=pos[a], arrowprops=dict(arrowstyle='->', color=colour, lw=0.5, alpha=0.7))
    ax.scatter(pos[:, 0], pos[:, 1], c=lab, cmap='coolwarm', s=60 if len(pos) <= 100 else 8, zorder=3, edgecolors='k', linewidths=0.3)
    if len(pos) <= 100:
        for i, p in enumerate(pos):
            ax.annotate(str(i), p, ha='center', va='center', fontsize=5, zorder=4)
    ax.set_xlim(-1.1, 1.1)
    ax.set_ylim(-1.1, 1.1)
    ax.set_axis_off()
    os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
    fig.savefig(path, facecolor='white', bbox_inches='tight')
    print(f'wrote {path}')


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--nodes', type=int, default=40)
    ap.add_argument('--neighbours', type=int, default=5)
    ap.add_argument('--walks', type=int, default=10, help='GraphSAINT batch_size: random walks per sub-graph')
    ap.add_argument('--walk-length', type=int, default=100)
    ap.add_argument('--seed', type=int, default=0, help='seed of the start positions')
    ap.add_argument('--out', default='layout_figures', metavar='DIR')
    args = ap.parse_args(argv)
    device = torch.device('cuda:0')
    gen = torch.Generator(device=device).manual_seed(0)

    xor = train_xor.duplicated_xor(args.nodes, 0.1, args.neighbours, device, gen)
    fit = spring_layout(xor.edge_index, xor.num_nodes, symmetric=False, seed=args.seed)      # plot_graph's DiGraph
    cross = float((xor.y[xor.edge_index[0]] != xor.y[xor.edge_index[1]]).float().mean())
    print(f'XOR graph: {xor.num_nodes} nodes, {fit.graph[1].numel()} arcs ({cross:.1%} across the classes), k = {fit.k:.4f}, '
          f'{fit.iterations_run} iterations; an edge is {edge_length_ratio(fit.pos, xor.edge_index):.2f} x the mean distance')
    draw(os.path.join(args.out, 'xor_graph.png'), 'duplicated-XOR k-nearest-neighbour graph', fit.pos, xor.edge_index, xor.y, arrows=True)

    cora = train_graphsaint.synthetic_cora(device)
    loader = GraphSAINTRandomWalkSampler(cora, batch_size=args.walks, walk_length=args.walk_length, num_steps=1, seed=1)
    batch = next(iter(loader))
    fit = spring_layout(batch.edge_index, batch.num_nodes, seed=args.seed)                   # to_networkx(batch, to_undirected=True)
    print(f'GraphSAINT sub-graph: {batch.num_nodes} nodes, {fit.graph[1].numel() // 2} edges, k = {fit.k:.4f}, '
          f'{fit.iterations_run} iterations; an edge is {edge_length_ratio(fit.pos, batch.edge_index):.2f} x the mean distance')
    draw(os.path.join(args.out, 'saint_subgraph.png'), f'GraphSAINT sub-graph: {args.walks} walks of length {args.walk_length}', fit.pos,
         batch.edge_index, batch.y, arrows=False)


if __name__ == '__main__':
    main()
