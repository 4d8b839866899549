"""AMPGCN's featuriser on the device (csrc/featurizer.hip): z-score of the node features, sampling of the present features
and the concatenation with their embedding rows, in place of the reference's per-node Python loop
(src/ampnet/module/amp_gcn.py:120-183).  Both branches are here: down-sampling (FeatureTokens.forward, the Cora harness)
and full width (FeatureTokens.forward_all, the XOR harness)."""
import torch
import torch.nn as nn

from .. import _lib
from ..gcn import zscore_stats
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
        return zscore_stats(x)

    def load_pca_table(self, x, freeze=True):
        """The reference's PCA featuriser (amp_gcn.py:185-206): row f of the table becomes the first feat_emb_dim principal
        component scores of feature column f of x [N, F] -- `pca.fit_transform(x.numpy().transpose())`, amp_gcn.py:196,
        under the exact solver (ampnet_amd.pca, samples='columns').  With forward / forward_all this gives its tokens
        concat(pca_row[f], zscore(x)[n, f]).  freeze: the table takes no gradient from then on (the reference's PCA
        rows are constants).  Returns the PCAResult."""
        from ..pca import pca
        table = self.feature_embedding_table
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.size(1) != table.num_embeddings:
            raise ValueError(f'load_pca_table: x has to be [N, {table.num_embeddings}] (one column per row of the table), got '
                             f'{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}')
        res = pca(x.detach().to(table.weight.device), table.embedding_dim, samples='columns')
        with torch.no_grad():
            table.weight.copy_(res.scores)
        if freeze:
            table.weight.requires_grad_(False)
        return res

    def load_umap_table(self, x, freeze=True, **umap_args):
        """The reference's UMAP featuriser (src/ampnet/utils/preprocess.py:29-68): row f of the table becomes the
        feat_emb_dim-dimensional UMAP embedding of feature column f of x [N, F] --
        `UMAP(n_neighbors=15, n_components=feat_emb_dim, min_dist=0.1).fit_transform(x.T)` as ampnet_amd.umap computes it
        (samples='columns'; umap_args are passed on).  freeze: the table takes no gradient from then on.  Returns the
        UMAPResult."""
        from ..umap import umap
        table = self.feature_embedding_table
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.size(1) != table.num_embeddings:
            raise ValueError(f'load_umap_table: x has to be [N, {table.num_embeddings}] (one column per row of the table), got '
                             f'{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}')
        if 'samples' in umap_args:
            raise ValueError("load_umap_table: the samples are the feature columns of x (samples='columns')")
        res = umap(x.detach().to(table.weight.device), table.embedding_dim, samples='columns', **umap_args)
        with torch.no_grad():
            table.weight.copy_(res.embedding)
        if freeze:
            table.weight.requires_grad_(False)
        return res

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

    def forward_masked(self, x, idx=None, *, rate, mode='token', mask_token, masked=None, full_width_repeats=None):
        """The tokens of masked feature modelling (ampnet_amd/masked.py): `forward` -- or, with full_width_repeats given,
        `forward_all(x, full_width_repeats)` -- with a share `rate` of the tokens hidden behind `mask_token` (the reference
        models' parameter, [1, feat_emb_dim + 1] float32): mode 'token' replaces the whole token vector
        (gcn_classifier.py:151), 'value' its z-scored value alone.  The mask is drawn from this module's seeded stream, or
        `masked` [N, L] bool is replayed.  Returns (tokens [N, L * D], idx [N, L] -- None at full width --, masked [N, L]
        bool, target [N, L] float32: the z-scored value of every token).  Gradients reach the table and mask_token."""
        from ..masked import build_masked_tokens
        if not x.is_cuda or x.dtype != torch.float32:
            raise ValueError('FeatureTokens needs float32 node features on the GPU (no CPU fallback)')
        x = x.contiguous()
        table = self.feature_embedding_table.weight
        if full_width_repeats is not None:
            if idx is not None:
                raise ValueError('full-width tokens take every feature column: feature indices cannot be given')
            reps = int(full_width_repeats) if full_width_repeats else 1
            if reps > 1:
                table = table.repeat(reps, 1)
            if table.size(0) != x.size(1) or x.size(1) != self.num_sampled_vectors:
                raise ValueError(f'full-width tokens need num_node_features * feature_repeats ({table.size(0)}) == '
                                 f'x.shape[1] ({x.size(1)}) == num_sampled_vectors ({self.num_sampled_vectors}) '
                                 '(torch.cat / reshape of amp_gcn.py:174-181 raise otherwise)')
            used, sampled = torch.arange(x.size(1), dtype=torch.int32, device=x.device).repeat(x.size(0), 1), None
        else:
            if idx is not None:
                idx = torch.as_tensor(idx, device=x.device)
                if idx.dim() != 2 or idx.size(0) != x.size(0) or idx.numel() == 0 or idx.is_floating_point():
                    raise ValueError(f'feature indices must be integers [{x.size(0)}, num_sampled_vectors], got '
                                     f'{idx.dtype} {tuple(idx.shape)}')
                lo, hi = int(idx.min()), int(idx.max())
                width = min(x.size(1), table.size(0))
                if lo < 0 or hi >= width:
                    raise ValueError(f'feature indices outside [0, {width}): min {lo}, max {hi}')
                idx = idx.to(torch.int32)
            else:
                idx, empty = self.sample(x)
                if int(empty.item()):
                    raise ValueError('a node has no present (non-zero) feature to sample from '
                                     '(np.random.choice raises in the reference, amp_gcn.py:135)')
            used = sampled = idx.contiguous()
        self._calls += 1
        seed = (self._seed * 1000003 + self._calls) & (2 ** 64 - 1)
        mean, inv_std = self.zscore_stats(x)
        tokens, mask, target = build_masked_tokens(table, mask_token, x, mean, inv_std, used, seed=seed, rate=rate, mode=mode,
                                                   masked=masked, dtype=self.token_dtype)
        return tokens.view(x.size(0), -1), sampled, mask.view(torch.bool), target

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
