"""Feature-to-feature attention heatmaps, accumulated on the GPU.

The reference's interpretability result (experiments/visualize_cora_attn_coeffs.py:212-216, calculate_attn_heatmap)
averages every coefficient of `conv.attn_output_weights [E, L, L]` into the cell (feature of the source token, feature
of the destination token), optionally only over the edges between two node classes.  Here one fused kernel
(csrc/attn_heatmap.hip, ampconv_attn_heatmap) computes scores, softmax and head mean per edge and adds them straight
into the table: `[E, L, L]` never exists.

    heat = AttentionHeatmap(src_features=top_a, dst_features=top_b)
    for batch in loader:                                  # any number of batches / ranks
        model(batch)
        heat.update(model.conv1, model.sampled_node_feat_indices, node_class=batch.y, src_class=a, dst_class=b)
    heat.all_reduce()                                     # optional: sum over ranks
    table = heat.result()                                 # [rows, cols] float64, rows = source features

The tables are 64-bit integers (weights in [0, 1] quantised to 2^-SHIFT, error <= 2^-(SHIFT+1) per term and per mean):
integer addition is associative, so `update` over split edge sets, `merge` and `all_reduce` give bitwise the same
tables as one pass over everything.
"""
import torch
import torch.distributed as dist

from . import _lib

SHIFT = 28                                  # AMPCONV_HEATMAP_SHIFT of include/ampconv.h (checked against the library)
MAX_TRIPLES = (1 << (63 - SHIFT)) - 1       # (edge, i, j) triples one accumulator takes before a cell could overflow


def _feature_list(features, name):
    t = torch.as_tensor(features, dtype=torch.int64).reshape(-1).cpu()
    if t.numel() == 0:
        raise ValueError(f'{name} is empty')
    if int(t.min()) < 0:
        raise ValueError(f'{name} holds a negative feature id')
    if torch.unique(t).numel() != t.numel():
        raise ValueError(f'{name} holds a feature id more than once')
    return t


class AttentionHeatmap:
    """Accumulator of a [len(src_features), len(dst_features)] heatmap: rows = source features, columns = destination
    features, as in the reference.

    dst_features=None: the same list as src_features.  src_features=None with num_features=F: the full F x F table.
    `sum` / `cnt` are int64 tables on the device of the first layer fed to `update` (on the CPU if the accumulator has
    only been merged into); `triples` counts the (edge, i, j) terms they may hold (the overflow guard)."""

    def __init__(self, src_features=None, dst_features=None, num_features=None):
        if src_features is None:
            if num_features is None:
                raise ValueError('give src_features, or num_features for the full table')
            src_features = torch.arange(int(num_features))
        self.src_features = _feature_list(src_features, 'src_features')
        self.dst_features = self.src_features if dst_features is None else _feature_list(dst_features, 'dst_features')
        top = int(max(self.src_features.max(), self.dst_features.max())) + 1
        if num_features is not None and int(num_features) < top:
            raise ValueError(f'num_features={num_features} but a selected feature id is {top - 1}')
        self.num_features = None if num_features is None else int(num_features)
        self.shift = SHIFT
        self.num_heads = None               # of the layers fed so far (recorded; the weights are quantised after the head mean)
        self.triples = 0
        self.sum = torch.zeros(self.shape, dtype=torch.int64)
        self.cnt = torch.zeros(self.shape, dtype=torch.int64)
        self._pos = {}

    @property
    def shape(self):
        return (self.src_features.numel(), self.dst_features.numel())

    @property
    def device(self):
        return self.sum.device

    def to(self, device):
        self.sum, self.cnt = self.sum.to(device), self.cnt.to(device)
        return self

    # ------------------------------------------------------------------ accumulation
    def _reserve(self, triples):
        if triples < 0 or self.triples + triples > MAX_TRIPLES:
            raise ValueError(f'AttentionHeatmap would hold {self.triples + triples} (edge, i, j) terms: more than '
                             f'{MAX_TRIPLES} could overflow an int64 cell at 2^-{self.shift} resolution; merge fewer '
                             'batches into one accumulator')

    def _positions(self, token_features, device):
        """rowpos, colpos [N, L] int32: where each token's feature sits among the selected features, -1 = not selected."""
        tok = torch.as_tensor(token_features).to(device=device, dtype=torch.int64)
        if tok.dim() != 2:
            raise ValueError(f'token_features must be [num_nodes, L], got {tuple(tok.shape)}')
        F = self.num_features
        if F is None:
            F = max(int(tok.max()) + 1 if tok.numel() else 0,
                    int(max(self.src_features.max(), self.dst_features.max())) + 1)
        elif tok.numel() and (int(tok.min()) < 0 or int(tok.max()) >= F):
            raise ValueError(f'token_features holds an id outside [0, {F})')
        key = (str(device), F)
        if key not in self._pos:
            self._pos.clear()
            maps = []
            for feats in (self.src_features, self.dst_features):
                m = torch.full((F,), -1, dtype=torch.int32, device=device)
                m[feats.to(device)] = torch.arange(feats.numel(), dtype=torch.int32, device=device)
                maps.append(m)
            self._pos[key] = maps
        pos_src, pos_dst = self._pos[key]
        if tok.numel() and int(tok.min()) < 0:
            raise ValueError('token_features holds a negative id')
        return pos_src[tok].contiguous(), pos_dst[tok].contiguous()

    def update(self, layer, token_features, *, edge_mask=None, node_class=None, src_class=None, dst_class=None):
        """Add the edges of `layer`'s last forward pass.  token_features [N, L]: the feature id of every token
        (AMPGCN.sampled_node_feat_indices).  Edge selection: all edges, AND `edge_mask` [E] bool if given, AND -- if
        `node_class` [N] is given -- the edges whose source has class `src_class` and whose destination has class
        `dst_class` (either may be None: any class)."""
        if not getattr(layer, 'softmax', True):
            raise NotImplementedError('attention heatmaps of softmax=False layers are not implemented: their scores '
                                      'are unbounded, so the fixed-point accumulation has no error bound')
        if layer._attn_ctx is None:
            layer._attn_missing('attention_heatmap')
            raise RuntimeError('attention_heatmap needs the projection buffer of a forward pass: run the layer first')
        Qv, Kv, _, edge_index, L = layer._attn_views()
        device = edge_index.device
        q_buf, _, _, _, shared = layer._attn_ctx
        N = q_buf.size(0) // L
        rowpos, colpos = self._positions(token_features, device)
        if tuple(rowpos.shape) != (N, L):
            raise ValueError(f'token_features is {tuple(rowpos.shape)}, the layer ran on {N} nodes of {L} tokens')
        E = edge_index.size(1)
        edge_index = edge_index.contiguous()
        mask = None
        if edge_mask is not None:
            mask = torch.as_tensor(edge_mask, device=device).to(torch.bool).reshape(-1)
            if mask.numel() != E:
                raise ValueError(f'edge_mask has {mask.numel()} entries for {E} edges')
        if node_class is not None:
            cls = torch.as_tensor(node_class, device=device).reshape(-1)
            if cls.numel() != N:
                raise ValueError(f'node_class has {cls.numel()} entries for {N} nodes')
            keep = torch.ones(E, dtype=torch.bool, device=device)
            if src_class is not None:
                keep &= cls[edge_index[0]] == src_class
            if dst_class is not None:
                keep &= cls[edge_index[1]] == dst_class
            mask = keep if mask is None else mask & keep
        elif src_class is not None or dst_class is not None:
            raise ValueError('src_class / dst_class need node_class')
        if self.sum.device != device:
            if self.triples:
                self.to(device)
            else:
                self.sum = torch.zeros(self.shape, dtype=torch.int64, device=device)
                self.cnt = torch.zeros(self.shape, dtype=torch.int64, device=device)
        self._reserve(E * L * L)
        lib = _lib.load()
        if lib.ampconv_attn_heatmap_shift() != self.shift:
            raise _lib.AmpconvError('libampconv.so was built with another AMPCONV_HEATMAP_SHIFT than this binding')
        mask_u8 = None if mask is None else mask.to(torch.uint8).contiguous()
        rows, cols = self.shape
        from .conv.functional import _stream
        with torch.cuda.device(device):
            rc = lib.ampconv_attn_heatmap(Qv, Kv, edge_index.data_ptr(), E, N,
                                          None if mask_u8 is None else mask_u8.data_ptr(),
                                          rowpos.data_ptr(), colpos.data_ptr(), L, layer.embed_dim, layer.num_heads,
                                          rows, cols, self.sum.data_ptr(), self.cnt.data_ptr(), self.triples,
                                          _lib.AMPCONV_F32, _stream())
        _lib.check(rc, 'ampconv_attn_heatmap')
        self.triples += E * L * L
        self.num_heads = layer.num_heads
        return self

    def _check_same(self, other):
        if not isinstance(other, AttentionHeatmap):
            raise TypeError('merge needs another AttentionHeatmap')
        if self.shape != other.shape or self.shift != other.shift:
            raise ValueError(f'cannot merge a {other.shape} heatmap (shift {other.shift}) into a {self.shape} one '
                             f'(shift {self.shift})')
        if not (torch.equal(self.src_features, other.src_features) and torch.equal(self.dst_features, other.dst_features)):
            raise ValueError('cannot merge heatmaps over different feature lists')

    def merge(self, other):
        """Add another accumulator over the same feature lists (exact: integer addition)."""
        self._check_same(other)
        self._reserve(other.triples)
        self.sum += other.sum.to(self.sum.device)
        self.cnt += other.cnt.to(self.cnt.device)
        self.triples += other.triples
        if self.num_heads is None:
            self.num_heads = other.num_heads
        return self

    def all_reduce(self, group=None):
        """Sum the tables over the ranks of `group` (int64 SUM: every rank ends with bitwise the same tables, equal to
        a `merge` of all of them).  Beside distributed.GradientAllReducer: "nccl" is RCCL on ROCm, "gloo" on the CPU."""
        meta = torch.tensor([self.triples], dtype=torch.int64, device=self.sum.device)
        dist.all_reduce(meta, op=dist.ReduceOp.SUM, group=group)
        total = int(meta.item())
        self._reserve(total - self.triples)
        flat = torch.cat([self.sum.reshape(-1), self.cnt.reshape(-1)])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        n = self.sum.numel()
        self.sum.copy_(flat[:n].view_as(self.sum))
        self.cnt.copy_(flat[n:].view_as(self.cnt))
        self.triples = total
        return self

    # ------------------------------------------------------------------ results
    def counts(self):
        """[rows, cols] int64: the number of (edge, i, j) terms in every cell."""
        return self.cnt.clone()

    def result(self):
        """[rows, cols] float64: mean attention weight per (source feature, destination feature), 0 where nothing
        arrived.  (The weights are quantised after the head mean, so there is no division by the head count.)"""
        s = self.sum.to(torch.float64) / float(1 << self.shift)
        c = self.cnt.to(torch.float64)
        return torch.where(self.cnt > 0, s / c.clamp(min=1.0), torch.zeros_like(s))


def top_features(x, node_class, cls, k=30):
    """The `k` features present (non-zero) in the most nodes of class `cls`, most frequent first, int64 on x's device:
    the reference's get_top_30_feature_idxs_for_class (visualize_cora_attn_coeffs.py), on the device.  A convenience:
    features with EQUAL counts at the cut may come out in another order -- or be other members of the tie -- than
    np.argpartition picks in the reference; pass explicit feature lists where that matters."""
    node_class = torch.as_tensor(node_class, device=x.device).reshape(-1)
    counts = x[node_class == cls].sum(dim=0)             # feature_presence_counts of the reference
    return torch.topk(counts, min(int(k), counts.numel())).indices
