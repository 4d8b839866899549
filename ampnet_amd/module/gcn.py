"""GCN on MI355X: the baseline every AMPNet result of the reference is compared against (the `TRAIN_AMPCONV = False`
side of its training scripts).

Mirrors reference src/ampnet/module/gcn_classifier.py:17-81: constructor arguments and their order, sub-module names and
therefore the state dict (feature_embedding_table.weight, conv1.bias, conv1.lin.weight, conv2.bias, conv2.lin.weight),
and the forward: dropout_adj -> embedded input -> conv1 -> ReLU -> dropout -> conv2 -> log_softmax (sigmoid with
softmax_out=False).  The reference builds the embedded input [N, F (feat_emb_dim + 1)] in a per-node Python loop on the
CPU (:91-109; 1.55 GB at Cora) and multiplies it by conv1's weight; here that product is computed from x without forming
the tensor (ampnet_amd.gcn.gcn_input_linear).  `input='zscore'` is the commented alternative of :70,83-89 (the z-scored x
alone), `input='raw'` the GCN of the two demos (examples/cora_benchmark.py:48-52); conv1.lin.weight is then [hidden, F].
Out of scope: the PCA / mask-token input (:111-159) and the plotting methods (ampnet_amd.tensor_stats works on any
module's gradients).  PyG parity is unpinned: include/ampconv.h, "GCN baseline", is the specification.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..conv.gcn_conv import GCNConv
from ..gcn import gcn_aggregate, gcn_input_linear, zscore_stats
from ..glue import ActDropout
from ..head import MAX_CLASSES, classifier_head, saint_nll_loss

INPUTS = ('embedded', 'zscore', 'raw')


class GCN(nn.Module):
    def __init__(self, device="cuda", num_node_features=1433, hidden_dim=16, num_sampled_vectors=40, output_dim=7,
                 softmax_out=True, feat_emb_dim=99, val_emb_dim=1, downsample_feature_vectors=True, dropout_rate=0.1,
                 dropout_adj_rate=0.1, *, input='embedded', seed=0, fused_glue=False, fused_head=False):
        super().__init__()
        if input not in INPUTS:
            raise ValueError(f'input must be one of {INPUTS}, got {input!r}')
        if val_emb_dim != 1:
            raise ValueError('val_emb_dim must be 1: the reference concatenates ONE z-scored value per feature '
                             '(gcn_classifier.py:101; its reshape raises for any other value)')
        if input == 'embedded' and num_sampled_vectors != num_node_features:
            raise ValueError(f"input='embedded' needs num_sampled_vectors ({num_sampled_vectors}) == num_node_features "
                             f'({num_node_features}): the reference reshapes [N, num_node_features, emb_dim] to [N, '
                             'num_sampled_vectors * emb_dim] (gcn_classifier.py:106), which raises otherwise -- with its '
                             'own default constructor (40 against 1433) included')
        self.device = device
        self.emb_dim = feat_emb_dim + val_emb_dim
        self.num_sampled_vectors = num_sampled_vectors
        self.num_node_features = num_node_features
        self.hidden_dim, self.output_dim = hidden_dim, output_dim
        self.softmax_out = softmax_out
        self.feat_emb_dim, self.val_emb_dim = feat_emb_dim, val_emb_dim
        self.downsample_feature_vectors = downsample_feature_vectors
        self.dropout_rate, self.dropout_adj_rate = dropout_rate, dropout_adj_rate
        self.input = input
        # same sub-module names as the reference => same state-dict keys; the table exists in every input mode, as there
        self.feature_embedding_table = nn.Embedding(num_embeddings=num_node_features, embedding_dim=feat_emb_dim)
        channels = num_node_features * (self.emb_dim if input == 'embedded' else 1)
        self.conv1 = GCNConv(channels, hidden_dim)
        self.act1 = nn.ReLU()
        self.drop1 = nn.Dropout(p=dropout_rate)
        self.conv2 = GCNConv(hidden_dim, output_dim)
        self.act_out = nn.Sigmoid()
        # fused_glue: ReLU -> dropout on [N, hidden] as one HIP pass, the mask from this library's seeded stream
        # (ampnet_amd/glue.py); in a list like AMPGCN's: the site has no parameters and the state dict stays the reference's
        self.fused_glue = bool(fused_glue)
        self._glue = [ActDropout(dropout_rate, 'relu', seed, site=11)] if self.fused_glue else []
        # fused_head: aggregation commutes with conv2.lin, so conv2(a) = (A_hat a) W2^T + b2 and the classifier head
        # kernel (ampnet_amd/head.py) runs on the aggregated [N, hidden] rows; nll_loss() fuses the loss behind it as well
        self.fused_head = bool(fused_head)
        if self.fused_head and output_dim > MAX_CLASSES:
            raise ValueError(f'fused_head supports output_dim <= {MAX_CLASSES}, got {output_dim}')

    def _hidden(self, data):
        """forward() up to the input of conv2: ([N, hidden] activations, the batch's edge_index after dropout_adj)."""
        x, edge_index = data.x.to(self.device), data.edge_index.to(self.device)
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError('GCN needs float32 node features on the GPU (no CPU fallback)')
        if x.dim() != 2 or x.size(1) != self.num_node_features:
            raise ValueError(f'GCN expects x [N, {self.num_node_features}], got {tuple(x.shape)}')
        if self.training and self.dropout_adj_rate > 0:                       # dropout_adj (gcn_classifier.py:67)
            keep = torch.rand(edge_index.size(1), device=edge_index.device) >= self.dropout_adj_rate
            edge_index = edge_index[:, keep]
        x = x.contiguous()
        mean = inv_std = table = None
        if self.input != 'raw':
            mean, inv_std = zscore_stats(x)
        if self.input == 'embedded':
            table = self.feature_embedding_table.weight
        h = gcn_input_linear(x, self.conv1.lin.weight, table, mean, inv_std)
        h = self.conv1.aggregate(h, edge_index)
        if self.fused_glue:
            self._glue[0].train(self.training)
            return self._glue[0](h), edge_index
        return self.drop1(self.act1(h)), edge_index

    def _aggregated(self, data):
        """A_hat a for the hidden activations a: the rows the head and the loss kernels multiply by conv2.lin.weight."""
        a, edge_index = self._hidden(data)
        return gcn_aggregate(a, edge_index, None, self.conv2.improved, self.conv2.add_self_loops)

    def nll_loss(self, data, y=None, node_norm=None, masks=None, grad_mask=0, metrics=None):
        """AMPGCN.nll_loss's contract on the baseline: (F.nll_loss(model(data), y, reduction='none') * node_norm)
        [masks[grad_mask]].sum() with conv2's linear map, the log-softmax, the loss and the metrics of every mask in one
        kernel per direction and no device synchronisation (ampnet_amd.saint_nll_loss on the aggregated [N, hidden]
        rows).  Needs softmax_out=True."""
        if not self.softmax_out:
            raise ValueError('nll_loss needs softmax_out=True (no fused loss for the sigmoid output)')
        if y is None:
            y = data.y
        if node_norm is None:
            node_norm = getattr(data, 'node_norm', None)
        rows = self._aggregated(data)
        return saint_nll_loss(rows, self.conv2.lin.weight, self.conv2.bias, y.to(self.device),
                              None if node_norm is None else node_norm.to(self.device), masks, grad_mask, metrics)

    def forward(self, data):
        if self.fused_head:
            return classifier_head(self._aggregated(data), self.conv2.lin.weight, self.conv2.bias,
                                   'log_softmax' if self.softmax_out else 'sigmoid')
        a, edge_index = self._hidden(data)
        x = self.conv2(a, edge_index)
        return F.log_softmax(x, dim=1) if self.softmax_out else self.act_out(x)
