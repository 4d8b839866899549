"""AMPGCN on MI355X: the reference's 2-layer model around AMPConv with its featuriser on the device.

Mirrors reference src/ampnet/module/amp_gcn.py:20-118 (constructor arguments, sub-module names and
therefore state-dict keys: feature_embedding_table, conv1, conv2, final_linear_out) and :239-276
(forward: dropout_adj -> featurise -> conv1 -> ReLU -> conv2 -> ReLU -> token pooling -> Linear
-> log_softmax; `fused_glue=True` runs the dropouts, activations and the pooling between those as fused HIP passes,
`fused_head=True` the Linear and the log_softmax / sigmoid as one more, and `nll_loss` the training loss behind them;
`layer_norm=True` adds the per-token LayerNorm sites norm1, norm2 of experiments/cora_overfit_one_subgraph.py:46-107).  Both featuriser branches of :120-183 are here: down-sampling of the present features
(:127-153, the Cora harness) and the full-width branch (:170-181, `downsample_feature_vectors=False`,
the XOR harness of synthetic_benchmark/xor_training_utils.py:58-72); both poolings of :268-271 (token mean,
or token 0 with `average_pooling_flag=False`).  The gradient and activation diagnostics of :278-405 (plot_grad_flow,
visualize_gradients, visualize_activations) are here with the reference's signatures and file names, drawn with matplotlib
from numbers taken on the device (gradient_stats, activation_stats: ampnet_amd/stats.py) instead of from host copies of
the tensors; seaborn's KDE curve and torch.mode are not reproduced.  Out of scope: the PCA featuriser variant (:185-237).
The per-node Python
sampling loop of :132-149 is replaced by csrc/featurizer.hip; the random stream is this library's (seeded);
`forward(data, feature_indices=...)` takes the indices of another stream (tests: the reference's own).
Pinned against the reference's class by tests/golden/model_*.npz (oracle/make_golden_ampgcn.py).

`storage_dtype=torch.bfloat16` (not in the reference): the two AMPConv layers, their parameters and every [N, L*D] tensor
between the featuriser and the pooling are stored in bf16 -- the library's fastest edge and projection kernels --; the
embedding table, the LayerNorm sites and final_linear_out stay fp32, and so does every accumulation.  Train it with
ampnet_amd.FusedAdam, which steps the bf16 parameters on fp32 masters.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib
from ..conv import AMPConv
from ..glue import ActDropout, TokenReadout, act_dropout
from ..head import MAX_CLASSES, classifier_head, saint_nll_loss
from ..norm import NormTokenReadout, TokenLayerNorm, norm_act_dropout
from ..stats import tensor_stats
from ..graph import _stream




class _BuildTokens(torch.autograd.Function):
    """tokens[n, l] = concat(table[idx[n, l]], zscore(x)[n, idx[n, l]]); gradient to `table` only
    (x is data; the reference's x_.requires_grad_(True) leaf is never used by an optimiser).  `dtype` is the storage of
    the tokens (float32 or bfloat16: the fp32 value rounded to nearest even) and of the gradient that comes back for them;
    the table and its gradient are fp32 either way."""

    @staticmethod
    def forward(ctx, table, x, mean, inv_std, idx, dtype=torch.float32):
        lib = _lib.load()
        if table.dtype != torch.float32:
            raise ValueError(f'the feature embedding table is {table.dtype}: it stays float32 (the featuriser kernels read '
                             f'fp32; AMPGCN(storage_dtype=torch.bfloat16) casts the conv layers only)')
        N, Fdim = x.shape
        L, De = idx.size(1), table.size(1)
        out = torch.empty(N, L, De + 1, dtype=dtype, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_feat_build_as(x.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), idx.data_ptr(),
                                                 table.data_ptr(), N, Fdim, L, De, out.data_ptr(), _lib.DTYPES[dtype],
                                                 _stream()), 'ampconv_feat_build_as')
        ctx.save_for_backward(idx)
        ctx.dims = (N, L, De, table.size(0))
        ctx.storage = dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        (idx,) = ctx.saved_tensors
        N, L, De, Fdim = ctx.dims
        dtable = torch.empty(Fdim, De, dtype=torch.float32, device=dout.device)
        dout = dout.to(ctx.storage).contiguous()
        with torch.cuda.device(dout.device):
            _lib.check(lib.ampconv_feat_table_grad_from(dout.data_ptr(), idx.data_ptr(), N, L, De, Fdim, dtable.data_ptr(),
                                                        _lib.DTYPES[ctx.storage], _stream()), 'ampconv_feat_table_grad_from')
        return dtable, None, None, None, None, None


class FeatureTokens(nn.Module):
    """z-score + present-feature sampling + embedding concat (amp_gcn.py:120-183, downsampling branch)."""

    def __init__(self, num_node_features, feat_emb_dim, num_sampled_vectors, seed=0, token_dtype=torch.float32):
        super().__init__()
        if token_dtype not in _lib.DTYPES:
            raise ValueError(f'tokens are written as float32 or bfloat16, not {token_dtype}')
        self.token_dtype = token_dtype
        self.feature_embedding_table = nn.Embedding(num_embeddings=num_node_features, embedding_dim=feat_emb_dim)
        self.num_sampled_vectors = num_sampled_vectors
        self._seed, self._calls = int(seed), 0

    def zscore_stats(self, x):
        lib = _lib.load()
        N, Fdim = x.shape
        mean = torch.empty(Fdim, dtype=torch.float32, device=x.device)
        inv_std = torch.empty(Fdim, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_feat_zscore_stats(x.data_ptr(), N, Fdim, mean.data_ptr(), inv_std.data_ptr(),
                                                     _stream()), 'ampconv_feat_zscore_stats')
        return mean, inv_std

    def sample(self, x, seed=None):
        lib = _lib.load()
        N, Fdim = x.shape
        L = self.num_sampled_vectors
        idx = torch.empty(N, L, dtype=torch.int32, device=x.device)
        empty = torch.zeros(1, dtype=torch.int32, device=x.device)
        if seed is None:
            self._calls += 1
            seed = (self._seed * 1000003 + self._calls) & (2 ** 64 - 1)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_feat_sample_present(x.data_ptr(), N, Fdim, L, seed, idx.data_ptr(),
                                                       empty.data_ptr(), _stream()), 'ampconv_feat_sample_present')
        return idx, empty

    def forward_all(self, x, feature_repeats):
        """Full-width branch (amp_gcn.py:170-181): token f of a node = concat(tile(table, feature_repeats)[f],
        zscore(x)[node, f]) for EVERY feature column f; no sampling (returns indices None like the reference)."""
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError('FeatureTokens needs float32 node features on the GPU (no CPU fallback)')
        x = x.contiguous()
        reps = int(feature_repeats) if feature_repeats else 1
        table = self.feature_embedding_table.weight
        if reps > 1:
            table = table.repeat(reps, 1)                       # torch.tile(weight, [feature_repeats, 1])
        if table.size(0) != x.size(1) or x.size(1) != self.num_sampled_vectors:
            raise ValueError(f'full-width tokens need num_node_features * feature_repeats ({table.size(0)}) == '
                             f'x.shape[1] ({x.size(1)}) == num_sampled_vectors ({self.num_sampled_vectors}) '
                             '(torch.cat / reshape of amp_gcn.py:174-181 raise otherwise)')
        idx = torch.arange(x.size(1), dtype=torch.int32, device=x.device).repeat(x.size(0), 1)
        mean, inv_std = self.zscore_stats(x)
        tokens = _BuildTokens.apply(table.contiguous(), x, mean, inv_std, idx, self.token_dtype)
        return tokens.view(x.size(0), -1), None

    def forward(self, x, idx=None):
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError('FeatureTokens needs float32 node features on the GPU (no CPU fallback)')
        x = x.contiguous()
        if idx is not None:
            idx = torch.as_tensor(idx, device=x.device)
            # given indices go straight into table[f] and x[n, f] on the device: refuse what would read out of bounds
            # (one read-back, on this replay path only)
            if idx.dim() != 2 or idx.size(0) != x.size(0) or idx.numel() == 0 or idx.is_floating_point():
                raise ValueError(f'feature indices must be integers [{x.size(0)}, num_sampled_vectors], got '
                                 f'{idx.dtype} {tuple(idx.shape)}')
            lo, hi = int(idx.min()), int(idx.max())
            width = min(x.size(1), self.feature_embedding_table.num_embeddings)
            if lo < 0 or hi >= width:
                raise ValueError(f'feature indices outside [0, {width}): min {lo}, max {hi}')
            idx = idx.to(torch.int32)
        if idx is None:
            idx, empty = self.sample(x)
            if int(empty.item()):
                raise ValueError('a node has no present (non-zero) feature to sample from '
                                 '(np.random.choice raises in the reference, amp_gcn.py:135)')
        mean, inv_std = self.zscore_stats(x)
        tokens = _BuildTokens.apply(self.feature_embedding_table.weight, x, mean, inv_std, idx.contiguous(),
                                    self.token_dtype)
        return tokens.view(x.size(0), -1), idx


class AMPGCN(nn.Module):
    def __init__(self, device="cuda", embedding_dim=100, num_heads=2, num_node_features=1433,
                 num_sampled_vectors=40, output_dim=7, softmax_out=True, feat_emb_dim=99, val_emb_dim=1,
                 downsample_feature_vectors=True, average_pooling_flag=True, dropout_rate=0.1,
                 dropout_adj_rate=0.1, feature_repeats=5, seed=0, fused_glue=False, fused_head=False, layer_norm=False,
                 storage_dtype=torch.float32):
        super().__init__()
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

    def _pooled(self, data, feature_indices=None):
        """forward() up to the token pooling: [N, embedding_dim], the input of final_linear_out.
        (_activation_sites below walks the same layer sequence in eval mode and keeps every intermediate tensor: a change
        of the sequence here has to be made there as well; tests/test_gpu_diagnostics.py holds the two together.)"""
        self._check_storage()
        x, edge_index = data.x.to(self.device), data.edge_index.to(self.device)
        if self.training and self.dropout_adj_rate > 0:                       # dropout_adj (amp_gcn.py:241)
            keep = torch.rand(edge_index.size(1), device=edge_index.device) >= self.dropout_adj_rate
            edge_index = edge_index[:, keep]
        if self.downsampling_vectors:
            x, sampled = self._tokens[0](x, feature_indices)
        else:
            x, sampled = self._tokens[0].forward_all(x, self.feature_repeats)
        self.sampled_node_feat_indices = sampled
        for site in self._glue:
            site.train(self.training)
        x = self.conv1(self._glue[0](x) if self.fused_glue else self.drop1(x), edge_index)
        self.conv1_embedding = x
        if self.layer_norm:                                                   # norm -> ReLU -> dropout (-> pooling): one pass each
            x = self.conv2(self.norm1(x), edge_index)
            self.conv2_embedding = x
            return self.norm2(x)
        if self.fused_glue:
            x = self.conv2(self._glue[1](x), edge_index)
            self.conv2_embedding = x
            return self._glue[2](x)
        x = self.conv2(self.drop2(F.relu(x)), edge_index)
        self.conv2_embedding = x
        x = self.drop3(F.relu(x))
        x = x.reshape(x.shape[0], x.shape[1] // self.emb_dim, self.emb_dim)
        return x.mean(dim=1) if self.average_pooling_flag else x[:, 0]      # token mean / token 0 (amp_gcn.py:268-271)

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

    # ---- diagnostics (amp_gcn.py:278-405): the numbers on the device, the figures from the numbers
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
                sites = self._activation_sites(data, feature_indices)
        finally:
            for m, flag in flags:                                      # every module's own flag, not the root's for all
                m.training = flag
        return tensor_stats(sites, bins=bins, median=True)

    def _activation_sites(self, data, feature_indices):
        self._check_storage()
        x, edge_index = data.x.to(self.device), data.edge_index.to(self.device)
        if self.downsampling_vectors:
            idx = feature_indices
            if idx is None and self.sampled_node_feat_indices is not None \
                    and self.sampled_node_feat_indices.shape[0] == x.shape[0]:
                idx = self.sampled_node_feat_indices
            if idx is None:
                idx = self._tokens[0].sample(x.contiguous(), seed=self._diagnostic_seed())[0]
            x, sampled = self._tokens[0](x, idx)
        else:
            x, sampled = self._tokens[0].forward_all(x, self.feature_repeats)
        self.sampled_node_feat_indices = sampled
        for site in self._glue:                                        # a plain list, not sub-modules: eval() misses them
            site.train(False)
        D, sites = self.emb_dim, {}

        def activation(h, norm):
            if self.layer_norm:
                return norm_act_dropout(h, D, norm.weight, norm.bias, norm.eps, 0.0, norm.activation, False)
            return act_dropout(h, 0.0, 'relu', False) if self.fused_glue else F.relu(h)

        act_name = 'LayerNorm+ReLU' if self.layer_norm else 'ReLU'
        h = self.conv1(x, edge_index)                                  # drop1 is the identity in eval mode
        self.conv1_embedding = sites['AmpConv 1'] = h
        a = sites[act_name + ' 1'] = activation(h, getattr(self, 'norm1', None))
        h = self.conv2(a, edge_index)
        self.conv2_embedding = sites['AmpConv 2'] = h
        a = sites[act_name + ' 2'] = activation(h, getattr(self, 'norm2', None))
        if self.layer_norm:
            pooled = self.norm2(h)
        elif self.fused_glue:
            pooled = self._glue[2](h)
        else:
            a = a.reshape(a.shape[0], a.shape[1] // D, D)
            pooled = a.mean(dim=1) if self.average_pooling_flag else a[:, 0]
        sites['Average Pooling' if self.average_pooling_flag else 'Class Token'] = pooled.contiguous()
        sites['Linear Out'] = F.linear(pooled.float(), self.final_linear_out.weight, self.final_linear_out.bias)
        return {k: v.contiguous() for k, v in sites.items()}

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
