"""The GCN baseline's two operators on HIP kernels (csrc/gcn.hip): the normalised neighbourhood sum of a GCNConv layer
and the first layer's linear map over the reference's embedded input.

Every training script of the reference carries `TRAIN_AMPCONV = True  # If False, trains a simple 2-layer GCN`
(experiments/cora_benchmark_graphsaint.py:27,58-75); the baseline is src/ampnet/module/gcn_classifier.py:17-81, two PyG
GCNConv layers.  PyG is not a dependency here and parity with PyG itself is UNPINNED: the semantics of include/ampconv.h,
"GCN baseline" -- a restatement of PyG 2.0-2.1's gcn_norm / GCNConv -- are the specification (tests/gcn_reference.py is
its fp64 model).  fp32 throughout, no float atomics: all results are bitwise reproducible run to run.  There is no eager
fallback: what the kernels do not take raises ValueError.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import ptr as _ptr
from .graph import EdgeCSR, _stream, graph_cache

LONG_SEGMENT = _lib.GCN_LONG_SEGMENT      # a CSR / CSC segment from this length on is summed by whole workgroups


def _pad4(c):
    return (c + 3) // 4 * 4


def _empty_rows(N, C, device):
    """[N, C] float32 with its row stride rounded up to 4 floats: the kernels' 16-byte path (C = 7 -> stride 8)."""
    return torch.empty(N, _pad4(C), dtype=torch.float32, device=device)[:, :C]


def _rows(t):
    """t as the kernels read it: unit stride inside a row, rows at least C apart (such a view is read in place)."""
    N, C = t.shape
    if N <= 1 or C == 0:
        return t.contiguous()
    if t.stride(1) != 1 or t.stride(0) < C:
        t = t.contiguous()
    return t


def _ld(t):
    return t.stride(0) if t.size(0) > 1 else max(t.size(1), 1)


def _check_rows(t, name, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f'{what}: {name} has to be a tensor on the GPU (ampnet_amd has no CPU fallback)')
    if t.dtype != torch.float32:
        raise ValueError(f'{what}: {name} is {t.dtype}; float32 only (bf16 storage is out of scope for the GCN baseline)')


def _csr(edge_index, num_nodes):
    if isinstance(edge_index, EdgeCSR):
        if num_nodes is not None and int(num_nodes) != edge_index.num_nodes:
            raise ValueError(f'the EdgeCSR has {edge_index.num_nodes} nodes, num_nodes says {num_nodes}')
        return edge_index
    if num_nodes is None:
        raise ValueError('num_nodes is needed with an edge_index tensor')
    return graph_cache.get(edge_index, num_nodes)          # shape / dtype / device errors come from EdgeCSR


def gcn_norm(edge_index, num_nodes=None, improved=False, add_self_loops=True):
    """dinv [N] float32 = deg^-1/2 (0 where deg == 0) of PyG's gcn_norm: with add_self_loops every loop of the input is
    dropped and one loop of weight fill = 2 (improved) or 1 is added per node; deg sums the weights of a node's incoming
    edges, duplicates counted as often as they occur.  edge_index: [2, E] int64 on the GPU (messages src -> dst) or an
    EdgeCSR.  Cached on the EdgeCSR per (improved, add_self_loops): both layers and both backward passes of a batch share
    one launch, the way graph_cache shares the CSR."""
    csr = _csr(edge_index, num_nodes)
    key = (bool(improved), bool(add_self_loops))
    cache = csr.__dict__.setdefault('_gcn_dinv', {})
    if key not in cache:
        lib = _lib.load()
        dinv = torch.empty(max(csr.num_nodes, 1), dtype=torch.float32, device=csr.device)
        with torch.cuda.device(csr.device):
            _lib.check(lib.ampconv_gcn_norm(csr.rowptr.data_ptr(), csr.col.data_ptr(), csr.num_nodes, int(key[1]),
                                            2.0 if key[0] else 1.0, dinv.data_ptr(), _stream()), 'ampconv_gcn_norm')
        cache[key] = dinv[:csr.num_nodes]
    return cache[key]


def _has_long(csr, side):
    """False when the graph's long-segment plan (one read-back at EdgeCSR construction) shows that no segment of that
    side exceeds hub_chunk <= 128 < LONG_SEGMENT entries: the long-segment kernels are then not launched at all."""
    if csr.num_edges < LONG_SEGMENT:
        return False
    if getattr(csr, 'hub_chunk', 0) and csr.hub_chunk < LONG_SEGMENT and csr.num_edges > csr.hub_chunk:
        return (csr.hub_dst_chunks if side == 'dst' else csr.hub_src_chunks) > 0
    return True


def _aggregate(h, csr, side, dinv, self_loops, fill, bias):
    lib = _lib.load()
    N, C = h.shape
    out = _empty_rows(N, C, h.device)
    if N == 0 or C == 0:
        return out
    ptr, idx = (csr.rowptr, csr.col) if side == 'dst' else (csr.cscptr, csr.crow)
    ws, nws = None, 0
    if _has_long(csr, side):
        nws = int(lib.ampconv_gcn_aggregate_workspace_bytes(N, csr.num_edges, C))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=h.device)
    with torch.cuda.device(h.device):
        _lib.check(lib.ampconv_gcn_aggregate(h.data_ptr(), _ld(h), C, ptr.data_ptr(), idx.data_ptr(), dinv.data_ptr(),
                                             int(self_loops), fill, None if bias is None else bias.data_ptr(),
                                             out.data_ptr(), _ld(out), N, csr.num_edges,
                                             None if ws is None else ws.data_ptr(), nws, _stream()),
                   'ampconv_gcn_aggregate')
    return out


def colsum(g):
    """sum over the rows of g [N, C] in a fixed order (bitwise reproducible): [C] float32."""
    lib = _lib.load()
    g = _rows(g)
    N, C = g.shape
    out = torch.empty(C, dtype=torch.float32, device=g.device)
    if C == 0:
        return out
    nws = int(lib.ampconv_gcn_colsum_workspace_bytes(N, C))
    ws = torch.empty(nws, dtype=torch.uint8, device=g.device)
    with torch.cuda.device(g.device):
        _lib.check(lib.ampconv_gcn_colsum(g.data_ptr(), _ld(g), N, C, out.data_ptr(), ws.data_ptr(), nws, _stream()),
                   'ampconv_gcn_colsum')
    return out


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias, csr, dinv, self_loops, fill):
        ctx.args = (csr, dinv, self_loops, fill)
        return _aggregate(_rows(h), csr, 'dst', dinv, self_loops, fill, None if bias is None else bias.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        csr, dinv, self_loops, fill = ctx.args
        dout = _rows(dout.float())
        dh = _aggregate(dout, csr, 'src', dinv, self_loops, fill, None) if ctx.needs_input_grad[0] else None
        db = colsum(dout) if ctx.needs_input_grad[1] else None
        return dh, db, None, None, None, None


def gcn_aggregate(h, edge_index, bias=None, improved=False, add_self_loops=True):
    """out = A_hat h + bias with A_hat[d, s] = dinv[d] w dinv[s] summed over the edges s -> d after gcn_norm's self-loop
    step (the propagate step of PyG's GCNConv): [N, C] float32, gradients to h (the same kernel on the source-sorted
    CSC: A_hat's weights are symmetric in their two factors) and to bias (a fixed-order column sum).  h: [N, C] float32
    on the GPU, N = the graph's nodes (a row-strided view is read in place); edge_index: [2, E] int64 on the GPU or an
    EdgeCSR.  The result is a [N, C] view of rows padded to a multiple of 4 floats."""
    _check_rows(h, 'h', 'gcn_aggregate')
    if h.dim() != 2:
        raise ValueError(f'gcn_aggregate: h has to be [N, C], got {tuple(h.shape)}')
    if bias is not None:
        _check_rows(bias, 'bias', 'gcn_aggregate')
        if bias.shape != (h.size(1),) or bias.device != h.device:
            raise ValueError(f'gcn_aggregate: bias has to be [C = {h.size(1)}] on the device of h, got {tuple(bias.shape)}')
    csr = _csr(edge_index, h.size(0))
    if csr.device != h.device:
        raise ValueError('gcn_aggregate: h and the graph are on different devices')
    dinv = gcn_norm(csr, None, improved, add_self_loops)
    return _Aggregate.apply(h, bias, csr, dinv, bool(add_self_loops), 2.0 if improved else 1.0)


class _InputLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, table, mean, inv_std):
        lib = _lib.load()
        N, Fdim = x.shape
        C = weight.size(0)
        De = 0 if table is None else table.size(1)
        weight = weight.contiguous()
        table = None if table is None else table.contiguous()
        h = _empty_rows(N, C, x.device)
        nws = int(lib.ampconv_gcn_input_workspace_bytes(N, Fdim, C))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
        if N > 0:
            with torch.cuda.device(x.device):
                _lib.check(lib.ampconv_gcn_input_fwd(x.data_ptr(), N, Fdim, _ptr(mean), _ptr(inv_std), weight.data_ptr(),
                                                     _ptr(table), De, C, h.data_ptr(), _ld(h), ws.data_ptr(), nws,
                                                     _stream()), 'ampconv_gcn_input_fwd')
        ctx.save_for_backward(x, weight, table, mean, inv_std)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        x, weight, table, mean, inv_std = ctx.saved_tensors
        N, Fdim = x.shape
        C = weight.size(0)
        De = 0 if table is None else table.size(1)
        g = _rows(g.float())
        dW = torch.empty_like(weight)
        dtable = None if table is None else torch.empty_like(table)
        nws = int(lib.ampconv_gcn_input_workspace_bytes(N, Fdim, C))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.ampconv_gcn_input_bwd(x.data_ptr(), N, Fdim, _ptr(mean), _ptr(inv_std), weight.data_ptr(),
                                                 _ptr(table), De, C, g.data_ptr(), _ld(g), dW.data_ptr(), _ptr(dtable),
                                                 ws.data_ptr(), nws, _stream()), 'ampconv_gcn_input_bwd')
        return None, dW, dtable, None, None


def zscore_stats(x):
    """(mean, inv_std) [F] float32 of sklearn's StandardScaler over the rows of x (ampconv_feat_zscore_stats)."""
    lib = _lib.load()
    N, Fdim = x.shape
    mean = torch.empty(Fdim, dtype=torch.float32, device=x.device)
    inv_std = torch.empty(Fdim, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(lib.ampconv_feat_zscore_stats(x.data_ptr(), N, Fdim, mean.data_ptr(), inv_std.data_ptr(), _stream()),
                   'ampconv_feat_zscore_stats')
    return mean, inv_std


def gcn_input_linear(x, weight, table=None, mean=None, inv_std=None):
    """The first GCN layer's linear map over the reference's embedded input (gcn_classifier.py:91-109) without forming
    that [N, F (De + 1)] tensor: with z = (x - mean) inv_std and weight [C, F (De + 1)] viewed as [C, F, De + 1],
        h[n, j] = sum_f z[n, f] weight[j, f, De] + sum_f sum_k table[f, k] weight[j, f, k]
    which equals cat(table, z[n]) flattened times weight^T up to fp32 re-association.  table None: weight [C, F], the
    z-scored input alone; mean and inv_std None as well: the raw x.  x [N, F] float32 on the GPU is data: gradients go
    to weight and table only.  Returns a [N, C] view of rows padded to a multiple of 4 floats."""
    for name, t in (('x', x), ('weight', weight)) + ((('table', table),) if table is not None else ()):
        _check_rows(t, name, 'gcn_input_linear')
    if x.dim() != 2 or weight.dim() != 2 or x.size(0) < 1 or x.size(1) < 1:
        raise ValueError(f'gcn_input_linear: x has to be [N, F], weight [C, F (De + 1)], got {tuple(x.shape)}, '
                         f'{tuple(weight.shape)}')
    De = 0 if table is None else table.size(1)
    if table is not None and (table.dim() != 2 or table.size(0) != x.size(1) or De < 1):
        raise ValueError(f'gcn_input_linear: table has to be [F = {x.size(1)}, De >= 1], got {tuple(table.shape)}')
    if weight.size(1) != x.size(1) * (De + 1):
        raise ValueError(f'gcn_input_linear: weight has {weight.size(1)} columns, F (De + 1) = {x.size(1) * (De + 1)}')
    if (mean is None) != (inv_std is None) or (table is not None and mean is None):
        raise ValueError('gcn_input_linear: mean and inv_std come together, and a table needs them')
    return _InputLinear.apply(x.contiguous(), weight, table, mean, inv_std)
