"""The unsupervised GraphSAGE loss over (anchor, positive, negatives) triples of node embeddings, fused (csrc/pair_loss.hip).

The reference announces this step and leaves it empty: synthetic_benchmark/contrastive_ssl_AMPNet.py and
predictive_ssl_AMPNet.py end in `criterion = None  # Implement GraphSAGE unsupervised loss function` (:79) under the
TensorFlow affinity / neg_cost / _skipgram_loss they quote (:14-49).  A PyTorch composite of it (index_select, matmul,
logsumexp, autograd) forms the [B, S] logits several times -- 38 GB per copy with every node of a 96 k-node GraphSAINT
batch as a negative of 100 k pairs.  Here the logits are tiled on chip and never written: one kernel sequence per
direction, the upstream gradient read from the device, loss and gradient bitwise reproducible.  The contract is
include/ampconv.h, "pair loss".  There is no eager fallback: what the kernels do not take raises ValueError.
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr as _ptr
from .graph import _stream
from .head import _rows

KINDS = {'skipgram': 0, 'xent': 1}                            # AMPCONV_PAIR_* of include/ampconv.h
MAX_D = 256                                                   # AMPCONV_PAIR_MAX_D
_SUPPORTED = (f'supported: z [N, D] float32 or bfloat16 on the GPU with 1 <= D <= {MAX_D}, anchors / positives [B] and '
              'negatives [S] int64 on the same device, S >= 1 unless B == 0 (ampnet_amd has no CPU fallback)')


def _workspace(lib, B, S, D, device):
    return torch.empty(max(int(lib.ampconv_pair_loss_workspace_bytes(B, S, D)), 256), dtype=torch.uint8, device=device)


class _PairLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, anchors, positives, negatives, weight, kind, scale, neg_weight, exclude, check):
        lib = _lib.load()
        z, ldz = _rows(z)
        N, D = z.shape
        B, S = anchors.numel(), negatives.numel()
        dev = z.device
        aff = torch.empty(B, dtype=torch.float32, device=dev)
        neg_term = torch.empty(B, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        oob = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _workspace(lib, B, S, D, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ampconv_pair_loss_fwd(z.data_ptr(), N, D, ldz, anchors.data_ptr(), positives.data_ptr(), B,
                                                 negatives.data_ptr(), S, _ptr(weight), kind, scale, neg_weight, exclude,
                                                 aff.data_ptr(), neg_term.data_ptr(), loss.data_ptr(), oob.data_ptr(),
                                                 ws.data_ptr(), ws.numel(), _lib.DTYPES[z.dtype], _stream()),
                       'ampconv_pair_loss_fwd')
        if check and int(oob.item()):
            raise ValueError(f'pair_loss: anchors, positives or negatives hold node ids outside [0, {N})')
        ctx.save_for_backward(z, anchors, positives, negatives, weight, aff, neg_term)
        ctx.args = (ldz, kind, scale, neg_weight, exclude)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        z, anchors, positives, negatives, weight, aff, neg_term = ctx.saved_tensors
        ldz, kind, scale, neg_weight, exclude = ctx.args
        N, D = z.shape
        B, S = anchors.numel(), negatives.numel()
        dev = z.device
        g = g.contiguous().float()                            # the upstream gradient stays on the device
        dz = torch.empty(N, D, dtype=z.dtype, device=dev)
        slot_ptr = slot_idx = None
        if B > 0:
            # node-sorted slot list (slot b: anchor b, B + b: positive b, 2 B + s: negative s); the stable sort fixes the
            # order of every node's sum
            ids = torch.cat((anchors, positives, negatives)).clamp_(0, N - 1)
            ids, order = torch.sort(ids, stable=True)
            slot_idx = order.to(torch.int32)
            slot_ptr = torch.searchsorted(ids, torch.arange(N + 1, device=dev)).to(torch.int32)
        ws = _workspace(lib, B, S, D, dev)
        with torch.cuda.device(dev):
            _lib.check(lib.ampconv_pair_loss_bwd(z.data_ptr(), N, D, ldz, anchors.data_ptr(), positives.data_ptr(), B,
                                                 negatives.data_ptr(), S, _ptr(weight), kind, scale, neg_weight, exclude,
                                                 aff.data_ptr(), neg_term.data_ptr(), g.data_ptr(), _ptr(slot_ptr),
                                                 _ptr(slot_idx), dz.data_ptr(), D, ws.data_ptr(), ws.numel(),
                                                 _lib.DTYPES[z.dtype], _stream()), 'ampconv_pair_loss_bwd')
        return dz, None, None, None, None, None, None, None, None, None


def _ids(t, name, dev):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != torch.int64 or t.dim() != 1:
        raise ValueError(f'pair_loss: {name} has to be a 1-d int64 tensor on the GPU of z; {_SUPPORTED}')
    return t.contiguous()


def pair_loss(z, anchors, positives, negatives, *, kind='skipgram', weight=None, neg_weight=1.0, scale=1.0,
              exclude_anchor=False, reduction='sum', check_indices=False):
    """The unsupervised GraphSAGE loss of the embeddings z [N, D] over B (anchor, positive) pairs that share S negatives,
    a 0-dim float32 tensor on the device with the gradient to z (in z's dtype):
        kind='skipgram': sum_b w_b (log sum_s exp(scale <a_b, n_s>) - scale <a_b, p_b>)     (the reference's quoted
                         _skipgram_loss, negated: what an optimizer minimises)
        kind='xent':     sum_b w_b (softplus(-scale <a_b, p_b>) + neg_weight sum_s softplus(scale <a_b, n_s>))
    with a_b = z[anchors[b]], p_b = z[positives[b]], n_s = z[negatives[s]].  exclude_anchor: the negatives equal to a
    pair's anchor are left out of its sum (for `negatives = every node of the batch`).  weight [B] float32 or None (1; no
    gradient).  reduction: 'sum' or 'mean' (over the B pairs).  Node ids outside [0, N) are clamped, never followed;
    check_indices=True reads the bounds flag back once and raises ValueError for them.  The [B, S] logits never reach
    memory; loss and gradient are bitwise reproducible."""
    if kind not in KINDS:
        raise ValueError(f'kind must be one of {sorted(KINDS)}, got {kind!r}')
    if reduction not in ('sum', 'mean'):
        raise ValueError(f"reduction must be 'sum' or 'mean', got {reduction!r}")
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or not 1 <= z.size(1) <= MAX_D:
        raise ValueError(f'pair_loss: z has shape {tuple(z.shape) if isinstance(z, torch.Tensor) else None}; {_SUPPORTED}')
    if z.dtype not in _lib.DTYPES:
        raise ValueError(f'pair_loss: z is {z.dtype}; {_SUPPORTED}')
    for t, name in ((anchors, 'anchors'), (positives, 'positives'), (negatives, 'negatives')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f'pair_loss: {name} has to be a 1-d int64 tensor; {_SUPPORTED}')
    B, S = anchors.numel(), negatives.numel()
    if positives.numel() != B:
        raise ValueError(f'pair_loss: {B} anchors and {positives.numel()} positives; {_SUPPORTED}')
    if B > 0 and (S < 1 or z.size(0) < 1):
        raise ValueError(f'pair_loss: {B} pairs need at least one negative and one node; {_SUPPORTED}')
    if not z.is_cuda:
        raise ValueError(f'pair_loss: z has to be on the GPU; {_SUPPORTED}')
    dev = z.device
    anchors, positives, negatives = (_ids(t, n, dev) for t, n in ((anchors, 'anchors'), (positives, 'positives'),
                                                                   (negatives, 'negatives')))
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.device != dev or weight.dtype != torch.float32 or \
                weight.shape != (B,):
            raise ValueError(f'pair_loss: weight has to be float32 [B = {B}] on the GPU of z, or None')
        weight = weight.detach().contiguous()
    loss = _PairLoss.apply(z, anchors, positives, negatives, weight, KINDS[kind], float(scale), float(neg_weight),
                           int(bool(exclude_anchor)), bool(check_indices))
    return loss / B if reduction == 'mean' and B > 0 else loss


class PairLoss(nn.Module):
    """pair_loss with its options held by a module: PairLoss(kind, ...)(z, anchors, positives, negatives, weight=None)."""

    def __init__(self, kind='skipgram', neg_weight=1.0, scale=1.0, exclude_anchor=False, reduction='sum',
                 check_indices=False):
        super().__init__()
        if kind not in KINDS:
            raise ValueError(f'kind must be one of {sorted(KINDS)}, got {kind!r}')
        if reduction not in ('sum', 'mean'):
            raise ValueError(f"reduction must be 'sum' or 'mean', got {reduction!r}")
        self.kind, self.neg_weight, self.scale = kind, float(neg_weight), float(scale)
        self.exclude_anchor, self.reduction, self.check_indices = bool(exclude_anchor), reduction, bool(check_indices)

    def forward(self, z, anchors, positives, negatives, weight=None):
        return pair_loss(z, anchors, positives, negatives, kind=self.kind, weight=weight, neg_weight=self.neg_weight,
                         scale=self.scale, exclude_anchor=self.exclude_anchor, reduction=self.reduction,
                         check_indices=self.check_indices)

    def extra_repr(self):
        return (f'kind={self.kind!r}, neg_weight={self.neg_weight}, scale={self.scale}, '
                f'exclude_anchor={self.exclude_anchor}, reduction={self.reduction!r}')


def walk_pairs(walks, node_idx=None, window=1, symmetric=False):
    """(anchors, positives) from random walks [n_walks, length]: the pairs (walks[:, i], walks[:, i + k]) for
    k = 1..window, in k-major order, then walk, then i.  node_idx (the sorted list GraphSAINTRandomWalkSampler.sample()
    returns): relabel both to sub-graph ids with torch.searchsorted.  symmetric: the reversed pairs follow.  Self pairs
    (a walk that stays on a node) are kept: dropping them would need a synchronisation.  Plain torch ops, CPU or GPU."""
    if walks.dim() != 2:
        raise ValueError(f'walks must be [n_walks, length], got {tuple(walks.shape)}')
    if int(window) < 1:
        raise ValueError(f'window must be at least 1, got {window}')
    length = walks.size(1)
    a = [walks[:, :length - k].reshape(-1) for k in range(1, min(int(window), length - 1) + 1)]
    p = [walks[:, k:].reshape(-1) for k in range(1, min(int(window), length - 1) + 1)]
    anchors = torch.cat(a) if a else walks.new_empty(0)
    positives = torch.cat(p) if p else walks.new_empty(0)
    if node_idx is not None:
        anchors = torch.searchsorted(node_idx, anchors)
        positives = torch.searchsorted(node_idx, positives)
    if symmetric:
        anchors, positives = torch.cat((anchors, positives)), torch.cat((positives, anchors))
    return anchors, positives
