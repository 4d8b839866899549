"""k nearest neighbours over node embeddings, fused (csrc/knn.hip): the consumer of the embeddings `pair_loss` trains.

The [Q, S] score matrix is tiled on chip and never written -- a dense `z @ z.t()` is 37 GB at one 96 k-node GraphSAINT
batch --, the best k of every query are kept in LDS and [Q, k] comes out.  `knn_graph` is the reference's graph
construction (synthetic_benchmark/synthetic_xor.py:69-101: scikit-learn's NearestNeighbors, an [N, N] adjacency matrix
and two Python loops) and `knn_classify` the nearest-neighbour evaluation of an embedding.  The contract is
include/ampconv.h, "nearest neighbours".  There is no eager fallback: what the kernels do not take raises ValueError.
"""
import torch

from . import _lib
from .graph import _stream
from .head import _rows

METRICS = {'dot': 0, 'cosine': 1, 'l2': 2}                    # AMPCONV_KNN_* of include/ampconv.h
MAX_D, MAX_K = 256, 64                                        # AMPCONV_KNN_MAX_D, AMPCONV_KNN_MAX_K
_SUPPORTED = (f'supported: x [N, D] float32 or bfloat16 on the GPU with 1 <= D <= {MAX_D}, 1 <= k <= {MAX_K}, queries / '
              'keys 1-d int64 on the same device or None (ampnet_amd has no CPU fallback)')


def _check_id_list(t, name):
    """The kernel reads count int64 values from the list's address: another dtype or shape never reaches it."""
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1):
        what = f'{t.dtype} {tuple(t.shape)}' if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f'knn: {name} has to be a 1-d int64 tensor or None, got {what}')


def _id_list(t, name, dev):
    if t is None:
        return None
    if t.device != dev:
        raise ValueError(f'knn: {name} is on {t.device}, it has to be on the device of x ({dev})')
    return t.contiguous()


def knn(x, k, *, queries=None, keys=None, metric='dot', exclude_self=False, check_indices=False):
    """(idx int64 [Q, k], score float32 [Q, k]): for every query row x[queries[q]] the k best of the key rows
    x[keys[s]] (None: every node, in order), best first, under
        metric='dot':    <a, b>, descending;      'cosine': <a, b> / (max(|a|, 1e-12) max(|b|, 1e-12)), descending;
        metric='l2':     the squared distance |a|^2 + |b|^2 - 2 <a, b> (clamped at 0), ascending.
    Ties go to the key that comes first in `keys`.  exclude_self: a key that is the query's own node is no candidate;
    a pair whose score is NaN is none either.  A row with fewer than k candidates ends in idx = -1 with score -inf
    (+inf for 'l2').  x may be a row-strided view; the outputs carry no gradient.  Node ids outside [0, N) are clamped,
    never followed; check_indices=True reads the bounds flag back once and raises ValueError for them.  The result is
    bitwise reproducible and a row does not depend on the other queries of the call."""
    if metric not in METRICS:
        raise ValueError(f'metric must be one of {sorted(METRICS)}, got {metric!r}')
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not 1 <= x.size(1) <= MAX_D:
        raise ValueError(f'knn: x has shape {tuple(x.shape) if isinstance(x, torch.Tensor) else None}; {_SUPPORTED}')
    if x.dtype not in _lib.DTYPES:
        raise ValueError(f'knn: x is {x.dtype}; {_SUPPORTED}')
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise ValueError(f'knn: k = {k!r}; {_SUPPORTED}')
    _check_id_list(queries, 'queries')
    _check_id_list(keys, 'keys')
    if not x.is_cuda:
        raise ValueError(f'knn: x has to be on the GPU; {_SUPPORTED}')
    dev = x.device
    queries, keys = _id_list(queries, 'queries', dev), _id_list(keys, 'keys', dev)
    x, ldx = _rows(x.detach())
    N, D = x.shape
    Q = N if queries is None else queries.numel()
    S = N if keys is None else keys.numel()
    if Q > 0 and N < 1:
        raise ValueError(f'knn: {Q} queries and no node; {_SUPPORTED}')
    idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
    score = torch.empty(Q, k, dtype=torch.float32, device=dev)
    if Q == 0:
        return idx, score
    lib = _lib.load()
    oob = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.ampconv_knn_workspace_bytes(Q, S, N, D, k)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ampconv_knn(x.data_ptr(), N, D, ldx, _lib.ptr(queries), Q, _lib.ptr(keys), S, k, METRICS[metric],
                                   int(bool(exclude_self)), idx.data_ptr(), score.data_ptr(), oob.data_ptr(),
                                   ws.data_ptr(), ws.numel(), _lib.DTYPES[x.dtype], _stream()), 'ampconv_knn')
    if check_indices and int(oob.item()):
        raise ValueError(f'knn: queries or keys hold node ids outside [0, {N})')
    return idx, score


def knn_graph(x, k, *, metric='l2', loop=True, check_finite=False):
    """edge_index int64 [2, N (k + 1)] of the k-nearest-neighbour graph of the rows of x, the reference's construction
    (synthetic_xor.py:69-101): every node's k + 1 nearest with the node itself a candidate (loop=True), or its k nearest
    others (loop=False: [2, N k]); edge_index[0] is the node, edge_index[1] its neighbours in ascending id order, rows in
    order.  k + 1 > N (loop=False: k > N - 1) raises ValueError: the shape never depends on the data.
    A row of x that holds a NaN has no neighbour and is nobody's neighbour: the missing entries of edge_index[1] are -1
    (they sort to the front of their row), which is NOT a node id -- indexing with such an edge_index reads out of range.
    Nothing is read back by default; check_finite=True reads one flag back and raises ValueError if an entry is missing."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError(f'knn_graph: x has to be [N, D]; {_SUPPORTED}')
    if isinstance(k, bool) or not isinstance(k, int) or k < 1:
        raise ValueError(f'knn_graph: k = {k!r}; {_SUPPORTED}')
    N, m = x.size(0), k + 1 if loop else k
    if m > (N if loop else N - 1):
        raise ValueError(f'knn_graph: {m} neighbours per node{"" if loop else " besides itself"} and {N} nodes')
    idx, _ = knn(x, m, metric=metric, exclude_self=not loop)
    if check_finite and bool((idx < 0).any()):
        raise ValueError('knn_graph: some nodes have fewer neighbours than asked for (rows of x with NaN): edge_index would hold -1')
    nbr = idx.sort(dim=1).values
    row = torch.arange(N, device=x.device).repeat_interleave(m)
    return torch.stack((row, nbr.reshape(-1)))


def knn_classify(z, y, k, *, queries=None, keys=None, metric='cosine', exclude_self=True, num_classes=None):
    """int64 [Q]: the majority label among every query's k nearest keys (y [N] integer labels of the nodes).  Ties go to
    the smaller class id, empty slots do not vote and a row without a neighbour gets -1.  num_classes=None reads
    y.max() back once."""
    if not isinstance(y, torch.Tensor) or y.dim() != 1 or y.is_floating_point() or y.dtype == torch.bool:
        raise ValueError('knn_classify: y has to be a 1-d integer tensor of node labels')
    if isinstance(z, torch.Tensor) and z.dim() == 2 and y.numel() != z.size(0):
        raise ValueError(f'knn_classify: {y.numel()} labels for {z.size(0)} nodes')
    idx, _ = knn(z, k, queries=queries, keys=keys, metric=metric, exclude_self=exclude_self)
    y = y.to(idx.device).long()
    C = int(num_classes) if num_classes is not None else (int(y.max()) + 1 if y.numel() else 1)
    found = idx >= 0
    votes = torch.zeros(idx.size(0), C, dtype=torch.int64, device=idx.device)
    votes.scatter_add_(1, y[idx.clamp(min=0)].clamp(0, C - 1), found.long())
    label = votes.argmax(dim=1)                              # the first maximum: the smaller class id
    return torch.where(found.any(dim=1), label, torch.full_like(label, -1))
