"""AMPGCN on MI355X: the reference's 2-layer model around AMPConv, with its featuriser on the device.

What is mirrored.  Reference src/ampnet/module/amp_gcn.py:20-118 gives the constructor arguments and the sub-module
names, and therefore the state-dict keys: feature_embedding_table, conv1, conv2, final_linear_out.  Its forward
(:239-276) is
    dropout_adj -> featurise -> drop1 -> conv1 -> ReLU -> drop2 -> conv2 -> ReLU -> drop3 -> token pooling
    -> Linear -> log_softmax
with both poolings of :268-271 (token mean, or token 0 with `average_pooling_flag=False`) and both featuriser branches of
:120-183 (feature_tokens.py).  The model is pinned against the reference's class by tests/golden/model_*.npz
(oracle/make_golden_ampgcn.py).  Out of scope: the PCA featuriser variant (:185-237).

One walk, three sites.  `_run` is the only function that knows the layer sequence:
    tokens -> entry -> conv1 -> between -> conv2 -> readout -> pooled [N, embedding_dim]
The constructor picks the three site objects once.  Plain: the PyTorch ops (_TorchSite around drop1 / drop2 / drop3,
torch's random stream).  `fused_glue=True`: one fused HIP pass per site (ampnet_amd/glue.py), masks from this library's
seeded stream.  `layer_norm=True`: the per-token LayerNorm sites norm1, norm2 of
experiments/cora_overfit_one_subgraph.py:46-107 (ampnet_amd/norm.py) in place of `between` and `readout`.  Every site
is called as `site(x)` in the forward pass; `site.activate(x)` is the same site with dropout off and without the pooling,
which is what the activation diagnostics show.

Behind the walk.  `forward` applies final_linear_out and the log_softmax / sigmoid, as one HIP kernel with
`fused_head=True`; `nll_loss` fuses the training loss and its metrics behind the head as well (ampnet_amd/head.py).  The
gradient and activation diagnostics of :278-405 are in diagnostics.py.

The random streams.  The per-node Python sampling loop of :132-149 is replaced by csrc/featurizer.hip with this
library's own seeded stream; `forward(data, feature_indices=...)` takes the indices of another stream (the tests use the
reference's own).

`storage_dtype=torch.bfloat16` (not in the reference): the two AMPConv layers, their parameters and every [N, L*D] tensor
between the featuriser and the pooling are stored in bf16 -- the library's fastest edge and projection kernels --; the
embedding table, the LayerNorm sites and final_linear_out stay fp32, and so does every accumulation.  Train it with
ampnet_amd.FusedAdam, which steps the bf16 parameters on fp32 masters.

`readout_token_only=True` (not in the reference; needs `average_pooling_flag=False`): conv2 is computed for the read-out
token only, `conv2.forward_token(between(h1), edge_index, 0)` -- its Q projection, out-projection and their gradients run
over N rows instead of N*L, its edge passes are the one-query-token family (csrc/edge_token.hip) -- and the readout site
receives [N, D]: one token, pooling `token0` over L = 1.  In eval mode, or with dropout_rate=0, outputs and gradients
equal the unflagged model's within the fp32 (bf16) bars of the tests.  In training, drop3's mask on [N, D] is another
draw from the same distribution than the unflagged model's mask on [N, L*D] -- for torch's stream and for the seeded
fused stream alike, which is keyed by element index.  conv2_embedding and the 'AmpConv 2' / activation diagnostics are
[N, D]; attention_heatmap(layer='conv2') raises; conv1 is untouched.  nll_loss, fused_head, fused_glue, layer_norm and
storage_dtype=torch.bfloat16 all work with the flag.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..conv import AMPConv
from ..glue import ActDropout, TokenReadout
from ..head import MAX_CLASSES, classifier_head, saint_nll_loss
from ..masked import MaskedValueHead, masked_value_loss
from ..norm import NormTokenReadout, TokenLayerNorm
from .diagnostics import Diagnostics
from .feature_tokens import FeatureTokens


class _TorchSite:
    """A site of the unfused model as PyTorch ops: [ReLU ->] nn.Dropout [-> token pooling], the interface of the fused
    sites (ampnet_amd/glue.py).  Holds no parameters; `drop` is the model's own drop1 / drop2 / drop3."""

    def __init__(self, drop, relu=True, embed_dim=None, mean=True):
        self.drop, self.relu, self.embed_dim, self.mean = drop, relu, embed_dim, mean

    def activate(self, x):
        return F.relu(x) if self.relu else x

    def __call__(self, x):
        x = self.drop(self.activate(x))
        if self.embed_dim is None:
            return x
        x = x.reshape(x.shape[0], x.shape[1] // self.embed_dim, self.embed_dim)
        return x.mean(dim=1) if self.mean else x[:, 0]                        # token mean / token 0 (amp_gcn.py:268-271)


class AMPGCN(Diagnostics, nn.Module):
    def __init__(self, device="cuda", embedding_dim=100, num_heads=2, num_node_features=1433,
                 num_sampled_vectors=40, output_dim=7, softmax_out=True, feat_emb_dim=99, val_emb_dim=1,
                 downsample_feature_vectors=True, average_pooling_flag=True, dropout_rate=0.1,
                 dropout_adj_rate=0.1, feature_repeats=5, seed=0, fused_glue=False, fused_head=False, layer_norm=False,
                 storage_dtype=torch.float32, readout_token_only=False, masked_modelling=False):
        super().__init__()
        if readout_token_only and average_pooling_flag:
            raise ValueError('readout_token_only=True needs average_pooling_flag=False: with the token mean every token '
                             'of conv2 is read')
        self.readout_token_only = bool(readout_token_only)
        if storage_dtype not in _lib.DTYPES:
            raise ValueError(f'storage_dtype is torch.float32 or torch.bfloat16, got {storage_dtype}')
        self.storage_dtype = storage_dtype
        assert embedding_dim == feat_emb_dim + val_emb_dim, \
            "Feature and value dimensions do not add up to total embedding dimension"
        if val_emb_dim != 1:
            raise ValueError('val_emb_dim must be 1: the reference concatenates ONE z-scored value per token '
                             '(amp_gcn.py:147,175; its reshape raises for any other value)')
        self.device = device
        self.downsampling_vectors = downsample_feature_vectors
        self.average_pooling_flag = average_pooling_flag
        self.feature_repeats = feature_repeats
        self.feat_emb_dim, self.val_emb_dim = feat_emb_dim, val_emb_dim
        self.dropout_rate = dropout_rate
        self.emb_dim = embedding_dim
        self.num_sampled_vectors = num_sampled_vectors
        self.num_node_features = num_node_features
        self.output_dim = output_dim
        self.softmax_out = softmax_out
        self.dropout_adj_rate = dropout_adj_rate
        self.sampled_node_feat_indices = None
        self.conv1_embedding = self.conv2_embedding = None
        # same sub-module names as the reference => same state-dict keys
        self._tokens = [FeatureTokens(num_node_features, feat_emb_dim, num_sampled_vectors, seed, storage_dtype)]
        self.feature_embedding_table = self._tokens[0].feature_embedding_table
        if not average_pooling_flag:               # defined (and in the state dict) but never used by forward,
            self.cls_token = nn.Parameter(torch.zeros(1, 1, self.emb_dim))    # exactly as amp_gcn.py:55-57,268-271
            nn.init.normal_(self.cls_token, std=.02)
        self.conv1 = AMPConv(embed_dim=embedding_dim, num_heads=num_heads)
        self.drop1 = nn.Dropout(p=dropout_rate)
        self.conv2 = AMPConv(embed_dim=embedding_dim, num_heads=num_heads)
        self.drop2 = nn.Dropout(p=dropout_rate)
        self.final_linear_out = nn.Linear(in_features=embedding_dim, out_features=output_dim)
        self.drop3 = nn.Dropout(p=dropout_rate)
        self.act_out = nn.Sigmoid()
        # storage_dtype=torch.bfloat16: the layers are built in fp32 (the reference's RNG consumption) and then cast, so the
        # initial parameters are the rounded fp32 ones under the same keys; everything else stays fp32.
        if storage_dtype != torch.float32:
            self.conv1.to(storage_dtype)
            self.conv2.to(storage_dtype)
        # fused_glue: drop1, ReLU -> drop2 and ReLU -> drop3 -> pooling as one HIP pass each (ampnet_amd/glue.py), masks from
        # this library's seeded stream instead of torch's.  Kept in a list like _tokens: the sites have no parameters and
        # the state dict stays the reference's.  Off (the default): the PyTorch ops below, torch's random stream.
        self.fused_glue = bool(fused_glue)
        pooling = 'mean' if average_pooling_flag else 'token0'
        self._glue = [ActDropout(dropout_rate, 'identity', seed, site=1), ActDropout(dropout_rate, 'relu', seed, site=2),
                      TokenReadout(embedding_dim, dropout_rate, 'relu', pooling, seed, site=3)] if self.fused_glue else []
        # layer_norm: the deeper reference model's per-token nn.LayerNorm behind each layer (experiments/
        # cora_overfit_one_subgraph.py:46-107, sub-modules norm1, norm2 as there): conv1 -> [norm1 -> ReLU -> drop2] -> conv2
        # -> [norm2 -> ReLU -> drop3 -> pooling], each bracket ONE HIP pass (ampnet_amd/norm.py) whatever fused_glue says;
        # their masks are always this library's.  Off (the default): no such sub-modules, the reference class's state dict.
        self.layer_norm = bool(layer_norm)
        if self.layer_norm:
            self.norm1 = TokenLayerNorm(embedding_dim, p=dropout_rate, activation='relu', seed=seed, site=4)
            self.norm2 = NormTokenReadout(embedding_dim, p=dropout_rate, activation='relu', pooling=pooling, seed=seed,
                                          site=5)
        # fused_head: final_linear_out -> log_softmax / sigmoid as one HIP kernel per direction on the module's own weight
        # and bias (ampnet_amd/head.py); nll_loss() below fuses the loss and its metrics behind it as well.
        self.fused_head = bool(fused_head)
        if self.fused_head and output_dim > MAX_CLASSES:
            raise ValueError(f'fused_head supports output_dim <= {MAX_CLASSES}, got {output_dim}')
        # the three sites of _run's walk (entry, between, readout), picked once; a tuple, so nothing is registered twice
        torch_sites = (_TorchSite(self.drop1, relu=False), _TorchSite(self.drop2),
                       _TorchSite(self.drop3, embed_dim=embedding_dim, mean=average_pooling_flag))
        self._sites = tuple(self._glue) if self.fused_glue else torch_sites
        if self.layer_norm:
            self._sites = (self._sites[0], self.norm1, self.norm2)
        # masked_modelling: the masked-autoencoder parameter of the reference's model classes under its name, shape and
        # init (gcn_one_layer.py:43-54; commented out in amp_gcn.py:60) and the value decoder of masked_feature_loss().
        # Created behind every other sub-module: their init RNG consumption and values do not change.  Both stay fp32
        # under bf16 storage.  Off (the default): neither exists, the reference class's state dict.
        self.masked_modelling = bool(masked_modelling)
        self.token_mask = None
        if self.masked_modelling:
            self.mask_token = nn.Parameter(torch.zeros(1, embedding_dim))
            nn.init.normal_(self.mask_token, std=.02)
            self.value_decoder = MaskedValueHead(embedding_dim)

    def _check_storage(self):
        """model.float() / model.to(torch.bfloat16) cast every parameter; the kernels behind the table, the norm sites and
        the head read fp32 and the layers read storage_dtype."""
        convs = {p.dtype for conv in (self.conv1, self.conv2) for p in conv.parameters()}
        rest = {p.dtype for n, p in self.named_parameters() if not n.startswith(('conv1.', 'conv2.'))}
        if convs != {self.storage_dtype} or rest != {torch.float32}:
            raise ValueError(f'AMPGCN(storage_dtype={self.storage_dtype}) needs conv1 / conv2 in {self.storage_dtype} and every '
                             f'other parameter in torch.float32, found {sorted(map(str, convs))} and {sorted(map(str, rest))}: '
                             f'a cast of the whole model (model.float(), model.to(torch.bfloat16)) is not a storage mode -- '
                             f'construct the model with the storage_dtype you want')

    def init_feature_table_from_pca(self, x, freeze=True):
        """feature_embedding_table.weight = the PCA scores of the feature columns of x [N, num_node_features], the
        reference's PCA featuriser (FeatureTokens.load_pca_table); freeze=True takes the table out of training."""
        return self._tokens[0].load_pca_table(x, freeze)

    def init_feature_table_from_umap(self, x, freeze=True, **umap_args):
        """feature_embedding_table.weight = the UMAP embedding of the feature columns of x [N, num_node_features], the
        reference's UMAP featuriser (FeatureTokens.load_umap_table); umap_args go to ampnet_amd.umap; freeze=True takes
        the table out of training."""
        return self._tokens[0].load_umap_table(x, freeze, **umap_args)

    def _run(self, data, feature_indices=None, sites=None, featurise=None, readout=True):
        """The layer walk up to the token pooling: [N, embedding_dim], the input of final_linear_out.  Sets
        conv1_embedding, conv2_embedding and sampled_node_feat_indices.  sites: a dict that receives, in this order, the
        tensors the diagnostics show -- both layer outputs, each followed by its site's activate(), and the pooled rows.
        featurise: a function x -> (tokens [N, L * D], sampled indices) in place of the model's featuriser (the masked
        tokens of masked_feature_loss); readout=False: the walk stops behind conv2 and returns its raw output."""
        self._check_storage()
        x, edge_index = data.x.to(self.device), data.edge_index.to(self.device)
        if self.training and self.dropout_adj_rate > 0:                       # dropout_adj (amp_gcn.py:241)
            keep = torch.rand(edge_index.size(1), device=edge_index.device) >= self.dropout_adj_rate
            edge_index = edge_index[:, keep]
        if featurise is not None:
            x, sampled = featurise(x)
        elif self.downsampling_vectors:
            x, sampled = self._tokens[0](x, feature_indices)
        else:
            x, sampled = self._tokens[0].forward_all(x, self.feature_repeats)
        self.sampled_node_feat_indices = sampled
        for site in self._glue:                                               # a plain list, not sub-modules: train() and
            site.train(self.training)                                         # eval() miss them
        entry, between, readout_site = self._sites
        self.conv1_embedding = h1 = self.conv1(entry(x), edge_index)
        if self.readout_token_only:                                           # [N, D]: token 0 is all the readout reads
            self.conv2_embedding = h2 = self.conv2.forward_token(between(h1), edge_index, 0)
        else:
            self.conv2_embedding = h2 = self.conv2(between(h1), edge_index)
        if not readout:
            return h2
        pooled = readout_site(h2)
        if sites is not None:
            act = 'LayerNorm+ReLU' if self.layer_norm else 'ReLU'
            shown = {'AmpConv 1': h1, act + ' 1': between.activate(h1), 'AmpConv 2': h2, act + ' 2': readout_site.activate(h2),
                     'Average Pooling' if self.average_pooling_flag else 'Class Token': pooled}
            sites.update((k, v.contiguous()) for k, v in shown.items())
        return pooled

    def _pooled(self, data, feature_indices=None):
        """forward() up to the token pooling: [N, embedding_dim], the input of final_linear_out."""
        return self._run(data, feature_indices)

    def embed(self, data, feature_indices=None):
        """The node embeddings: the pooled [N, embedding_dim] rows in front of final_linear_out, with their gradient --
        what an unsupervised loss trains (ampnet_amd.pair_loss).  Sets conv1_embedding, conv2_embedding and
        sampled_node_feat_indices as forward does."""
        return self._pooled(data, feature_indices)

    def nll_loss(self, data, y=None, node_norm=None, masks=None, grad_mask=0, metrics=None, feature_indices=None):
        """The reference's training loss (F.nll_loss(model(data), y, reduction='none') * node_norm)[masks[grad_mask]].sum()
        with the head, the loss and the metrics of every mask fused into one kernel per direction and no device
        synchronisation (ampnet_amd.saint_nll_loss; `metrics`: a HeadMetrics).  y and node_norm default to data.y and
        data.node_norm (no weights if the batch has none).  Sets conv1_embedding, conv2_embedding and
        sampled_node_feat_indices as forward does.  Needs softmax_out=True: there is no fused loss for the sigmoid."""
        if not self.softmax_out:
            raise ValueError('nll_loss needs softmax_out=True (no fused loss for the sigmoid output)')
        if y is None:
            y = data.y
        if node_norm is None:
            node_norm = getattr(data, 'node_norm', None)
        pooled = self._pooled(data, feature_indices)
        y = y.to(self.device)
        return saint_nll_loss(pooled, self.final_linear_out.weight, self.final_linear_out.bias, y,
                              None if node_norm is None else node_norm.to(self.device), masks, grad_mask, metrics)

    def masked_feature_loss(self, data, mask_rate=0.15, mask_mode='token', feature_indices=None, token_mask=None,
                            metrics=None):
        """The predictive self-supervised loss (the `criterion` that experiments/predictive_ssl_AMPNet.py leaves open): a
        share mask_rate of the tokens is hidden behind mask_token (mask_mode 'token': the whole token vector, the
        reference's replacement at gcn_classifier.py:151; 'value': its z-scored value alone, the feature's identity kept),
        the model runs dropout_adj -> masked tokens -> entry site -> conv1 -> between site -> conv2, and value_decoder reads
        conv2's raw output: the mean squared error of the hidden values over the masked tokens, a 0-dim tensor on the
        device (ampnet_amd.masked_value_loss; no readout site, no pooling, no device synchronisation behind the
        featuriser).  token_mask [N, L] bool replays a mask instead of drawing one; metrics: a MaskedMetrics.  Sets
        conv1_embedding, conv2_embedding and sampled_node_feat_indices as forward does, and token_mask.  Needs
        AMPGCN(masked_modelling=True); raises with readout_token_only=True (conv2 then computes one token)."""
        if not self.masked_modelling:
            raise ValueError('masked_feature_loss needs AMPGCN(masked_modelling=True): the model has no mask_token and no '
                             'value_decoder')
        if self.readout_token_only:
            raise ValueError('masked_feature_loss needs every token of conv2: readout_token_only=True computes one')
        found = {}

        def featurise(x):
            repeats = None if self.downsampling_vectors else (self.feature_repeats or 1)
            tokens, sampled, found['masked'], found['target'] = self._tokens[0].forward_masked(
                x, feature_indices if self.downsampling_vectors else None, rate=mask_rate, mode=mask_mode,
                mask_token=self.mask_token, masked=token_mask, full_width_repeats=repeats)
            return tokens, sampled

        h2 = self._run(data, featurise=featurise, readout=False)
        self.token_mask = found['masked']
        return masked_value_loss(h2, found['masked'], found['target'], self.value_decoder.weight, self.value_decoder.bias,
                                 metrics)

    def forward(self, data, feature_indices=None):
        x = self._pooled(data, feature_indices)
        if self.fused_head:
            return classifier_head(x, self.final_linear_out.weight, self.final_linear_out.bias,
                                   'log_softmax' if self.softmax_out else 'sigmoid')
        x = self.final_linear_out(x.float())                                  # (bf16 storage: the pooled rows are bf16)
        return F.log_softmax(x, dim=1) if self.softmax_out else self.act_out(x)

    def attention_heatmap(self, layer='conv1', src_features=None, dst_features=None, *, num_features=None,
                          **selection):
        """Feature-to-feature attention heatmap of `layer` ('conv1' / 'conv2') for the last forward pass, with this
        model's own sampled_node_feat_indices: what experiments/visualize_cora_attn_coeffs.py:212-216 computes by hand
        (AMPConv.attention_heatmap; `selection`: edge_mask / node_class, src_class, dst_class)."""
        if self.sampled_node_feat_indices is None:
            raise RuntimeError('attention_heatmap needs the sampled feature indices of a forward pass '
                               '(downsample_feature_vectors=True)')
        if src_features is None and num_features is None:
            num_features = self.num_node_features
        return getattr(self, layer).attention_heatmap(self.sampled_node_feat_indices, src_features, dst_features,
                                                      num_features=num_features, **selection)
