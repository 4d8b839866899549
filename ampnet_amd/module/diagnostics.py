"""AMPGCN's gradient and activation diagnostics (reference src/ampnet/module/amp_gcn.py:278-405: plot_grad_flow,
visualize_gradients, visualize_activations) as a mixin of the model.

The reference's signatures and file names are kept.  The numbers are taken on the device (gradient_stats,
activation_stats: ampnet_amd/stats.py) instead of from host copies of the tensors, and the figures are drawn with
matplotlib from those numbers; seaborn's KDE curve and torch.mode are not reproduced.

The mixin knows nothing of the layer sequence: activation_stats asks AMPGCN._run for the tensors of one eval-mode pass.
"""
import torch
import torch.nn.functional as F

from ..stats import tensor_stats


class Diagnostics:
    """Needs of its host class: nn.Module, _run(data, feature_indices, sites), _tokens, _glue, downsampling_vectors,
    sampled_node_feat_indices, final_linear_out and device."""

    def gradient_stats(self, bins=30, median=True):
        """A TensorStats (ampnet_amd.tensor_stats) over the gradients the reference plots (amp_gcn.py:283,325): the
        parameters with "weight" in their name and a gradient, by name, in named_parameters() order -- counts, min / max /
        absmax, mean / absmean / std, a `bins`-bin histogram over each gradient's own range and the median.  Launches on
        the current stream and returns at once; `.read()` is the one synchronisation.  No `mode` (:297): on continuous
        data torch.mode returns the minimum, `zeros` and `min` say what it would."""
        grads = {n: p.grad for n, p in self.named_parameters() if 'weight' in n and p.grad is not None}
        return tensor_stats({n: g if g.is_contiguous() else g.contiguous() for n, g in grads.items()}, bins=bins,
                            median=median)

    def _diagnostic_seed(self):
        return (self._tokens[0]._seed * 1000003 + 0x5D1A6) & (2 ** 64 - 1)     # no call counter in it

    def _diagnostic_indices(self, data, feature_indices=None):
        """The feature indices of a diagnostic pass: the argument, else the model's own if they fit data.x, else a draw
        with _diagnostic_seed() (no call counter advanced, no emptiness read-back).  Full-width models have none."""
        if feature_indices is not None or not self.downsampling_vectors:
            return feature_indices
        own = self.sampled_node_feat_indices
        if own is not None and own.shape[0] == data.x.shape[0]:
            return own
        return self._tokens[0].sample(data.x.to(self.device).contiguous(), seed=self._diagnostic_seed())[0]

    def activation_stats(self, data, bins=50, feature_indices=None):
        """A TensorStats over the activations of an eval-mode, no_grad forward pass of `data` (amp_gcn.py:345-390), by
        site: "AmpConv 1", "ReLU 1", "AmpConv 2", "ReLU 2", "Average Pooling" (or "Class Token"), "Linear Out" (the logits
        before the log-softmax / sigmoid); with layer_norm=True the activations are "LayerNorm+ReLU 1" / "LayerNorm+ReLU 2"
        (the fused site never writes the bare norm).  Per site: counts (zeros / numel of a ReLU site is its dead share),
        moments, a `bins`-bin histogram over the site's own range and the median.  Where the configured forward fuses the
        second activation into the pooling (fused_glue, layer_norm) that site is materialised for this call only, by the
        same kernel family without the pooling.

        Differences from the reference: it stores both ReLUs under the key "ReLU 1", so its first one is lost -- both are
        kept here; it leaves the model in eval mode -- the previous `training` flag of every sub-module is restored
        here.  As forward does,
        the call sets conv1_embedding, conv2_embedding and sampled_node_feat_indices.  It advances NO seeded stream of the
        library: dropout is off, and the feature indices are `feature_indices`, else this model's
        sampled_node_feat_indices if they fit data.x (the batch that was just trained on), else drawn with a fixed seed
        that leaves the sampler's call counter alone (no check for nodes without present features: that would be a
        read-back)."""
        flags = [(m, m.training) for m in list(self.modules()) + list(self._glue)]
        self.eval()
        try:
            with torch.no_grad():
                sites = {}
                pooled = self._run(data, self._diagnostic_indices(data, feature_indices), sites)
                sites['Linear Out'] = F.linear(pooled.float(), self.final_linear_out.weight, self.final_linear_out.bias)
        finally:
            for m, flag in flags:                                      # every module's own flag, not the root's for all
                m.training = flag
        return tensor_stats(sites, bins=bins, median=True)

    @staticmethod
    def _figure(*args, **kwargs):
        """matplotlib's object interface on the Agg canvas: no pyplot state, no global backend switch."""
        try:
            from matplotlib.backends.backend_agg import FigureCanvasAgg
            from matplotlib.figure import Figure
        except ImportError as e:
            raise ImportError('the figures need matplotlib, which is not installed; the numbers behind them do not: '
                              'AMPGCN.gradient_stats() / AMPGCN.activation_stats(data) return them') from e
        fig = Figure(*args, **kwargs)
        FigureCanvasAgg(fig)
        return fig

    @staticmethod
    def _bars(ax, s, color, density=False):
        h, edges = s['hist'].astype('float64'), s['edges']
        width = edges[1:] - edges[:-1]
        if density and h.sum() > 0 and (width > 0).all():
            h = h / (h.sum() * width)
        if not (width > 0).all():                                      # a constant tensor: one bar of unit width
            edges, width = edges[:-1] - 0.5, 1.0
        else:
            edges = edges[:-1]
        ax.bar(edges, h, width=width, align='edge', color=color, alpha=0.6)

    def plot_grad_flow(self, save_path, epoch_idx, iter, stats=None):
        """amp_gcn.py:308-343: max- and mean-|gradient| bars per weight, written to
        <save_path>/gradient_flow_plots/gradient_flow_ep{epoch_idx}_itr{iter}; one read-back.  Returns the dict of
        gradient_stats(bins=0, median=False).read() it drew from.  stats: a gradient_stats() result queued earlier (or its
        read() dict) to draw instead of the gradients as they are now."""
        import os
        stats = self._read(stats) if stats is not None else self.gradient_stats(bins=0, median=False).read()
        fig = self._figure()
        ax = fig.add_subplot()
        layers = list(stats)
        at = list(range(len(layers)))
        ax.bar(at, [stats[n]['absmax'] for n in layers], alpha=0.1, lw=1, color='c')
        ax.bar(at, [stats[n]['absmean'] for n in layers], alpha=0.1, lw=1, color='b')
        ax.hlines(0, 0, len(layers) + 1, lw=2, color='k')
        ax.set_xticks(at)
        ax.set_xticklabels(layers, rotation='vertical')
        ax.set_xlim(left=0, right=max(len(layers), 1))
        ax.set_ylim(bottom=-0.001, top=0.02)                           # the reference's zoom on the low-gradient region
        ax.set_xlabel('Layers')
        ax.set_ylabel('average gradient')
        ax.set_title('Gradient flow')
        ax.grid(True)
        from matplotlib.lines import Line2D
        ax.legend([Line2D([0], [0], color=c, lw=4) for c in 'cbk'], ['max-gradient', 'mean-gradient', 'zero-gradient'])
        out = os.path.join(save_path, 'gradient_flow_plots')
        os.makedirs(out, exist_ok=True)
        fig.savefig(os.path.join(out, f'gradient_flow_ep{epoch_idx}_itr{iter}'), bbox_inches='tight', facecolor='white')
        return stats

    @staticmethod
    def _read(stats):
        return stats.read() if hasattr(stats, 'read') else stats

    def visualize_gradients(self, save_path, epoch_idx, iter, color="C0", stats=None):
        """amp_gcn.py:278-306: a 30-bin histogram per weight gradient with mean, median, std and the share of zeros in
        its title (no KDE curve, no mode), written to <save_path>/gradient_distrib_plots/
        gradient_distrib_epoch{epoch_idx}_itr{iter}; one read-back.  Returns the dict of gradient_stats().read().
        stats: as for plot_grad_flow (it needs bins and the median)."""
        import os
        stats = self._read(stats) if stats is not None else self.gradient_stats(bins=30, median=True).read()
        columns = max(len(stats), 1)
        fig = self._figure(figsize=(columns * 4, 4))
        for i, (name, s) in enumerate(stats.items()):
            ax = fig.add_subplot(1, columns, i + 1)
            self._bars(ax, s, color)
            ax.set_title(f'{name}\nMean: {s["mean"]:.4f}, Median: {s["median"]:.4f}\nSTD: {s["std"]:.4f}, '
                         f'zeros: {s["zeros"] / max(s["numel"], 1):.1%}')
            ax.set_xlabel('Grad magnitude')
        fig.suptitle('Gradient Magnitude Distribution', fontsize=14, y=1.05)
        fig.subplots_adjust(wspace=0.45)
        out = os.path.join(save_path, 'gradient_distrib_plots')
        os.makedirs(out, exist_ok=True)
        fig.savefig(os.path.join(out, f'gradient_distrib_epoch{epoch_idx}_itr{iter}'), bbox_inches='tight',
                    facecolor='white')
        return stats

    def visualize_activations(self, save_path, data, epoch_idx, iter, color="C0", stats=None):
        """amp_gcn.py:345-406: a 50-bin density histogram per activation site of activation_stats(data), written to
        <save_path>/act_distrib_ep{epoch_idx}_iter{iter}; one read-back.  Unlike the reference the model's training
        flag is restored and both ReLU sites are shown.  Returns the dict of activation_stats(data).read().  stats: an
        activation_stats() result queued earlier (or its read() dict); `data` is then not looked at."""
        import math
        import os
        stats = self._read(stats) if stats is not None else self.activation_stats(data, bins=50).read()
        columns = 2
        rows = math.ceil(len(stats) / columns)
        fig = self._figure(figsize=(columns * 2.7, rows * 2.5))
        for i, (name, s) in enumerate(stats.items()):
            ax = fig.add_subplot(rows, columns, i + 1)
            self._bars(ax, s, color, density=True)
            ax.set_title(f'{name}\nmean {s["mean"]:.3g}, median {s["median"]:.3g}\nstd {s["std"]:.3g}, '
                         f'zeros {s["zeros"] / max(s["numel"], 1):.1%}', fontsize=8)
        fig.suptitle('Activation distribution', fontsize=16)
        fig.subplots_adjust(hspace=0.9, wspace=0.4)
        os.makedirs(save_path, exist_ok=True)
        fig.savefig(os.path.join(save_path, f'act_distrib_ep{epoch_idx}_iter{iter}'))
        return stats
