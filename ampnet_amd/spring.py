"""Force-directed graph layout (csrc/spring.hip): the reference's picture of a graph -- `nx.spring_layout(G)` in
synthetic_benchmark/synthetic_xor.py (plot_graph) and `nx.draw(g)`, whose default layout is the same, in
visualization/visualize_graphsaint_subgraphs.py.

`spring_layout(edge_index, num_nodes, ...)` computes what networkx 3.4.2's `spring_layout` computes (Fruchterman-Reingold)
as include/ampconv.h ("Spring layout") restates it; that text and the fp64 model in tests/spring_reference.py are the
specification, parity with networkx's values is pinned by the fixtures under tests/golden/spring.  The adjacency comes
from one stable library sort, and every iteration is two calls: ampconv_spring_repulsion (the N x N repulsive term, tiled
on chip, never written) and ampconv_spring_step (attraction over the CSR, the move, and the temperature / stopping rule
on the device).  networkx's loop is synchronous itself, so nothing about it changes: no atomics, two runs give the same
bits, another seed gives other bits.  The host reads nothing back during the layout: the `break` of networkx is a latch
in the device state, and `iterations_run` is read only when asked for.  There is no autograd and no CPU fallback: what
the kernels do not take raises ValueError.
"""
import math

import torch

from . import _lib
from .graph import _stream

MAX_N, PART = _lib.SPRING_MAX_N, _lib.SPRING_PART
_SUPPORTED = (f'supported: edge_index int64 [2, E] on the GPU, 0 <= num_nodes <= {MAX_N}, dim 2 or 3, pos float32 '
              '[num_nodes, dim] on the same device (ampnet_amd has no CPU fallback)')


def adjacency(edge_index, num_nodes, weight=None, symmetric=True):
    """(indptr int64 [N + 1], indices int64 [nnz], val float32 [nnz]): the CSR of the adjacency matrix that networkx
    lays out, indices ascending within a row.  symmetric=True (no weights): the union of both directions, duplicates
    collapsed, weight 1 -- `to_networkx(data, to_undirected=True)`.  symmetric=False keeps the direction (a DiGraph: row
    i is attracted along its out-edges only); without weights duplicates collapse to weight 1, with `weight` (float
    [E]; symmetric has to be False) duplicate entries are summed, in fp64 in the order of the edge list.  Self-loops
    are kept: they contribute exactly 0.  One stable library sort of the keys: bitwise reproducible."""
    N = int(num_nodes)
    dev = edge_index.device
    r, c = edge_index[0], edge_index[1]
    if weight is None:
        key = r * N + c
        if symmetric:
            key = torch.cat((key, c * N + r))
        key = torch.sort(key, stable=True).values
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]
        key = key[first]
        val = torch.ones(key.numel(), dtype=torch.float32, device=dev)
    else:
        key, order = torch.sort(r * N + c, stable=True)
        w = weight.double()[order]
        first = torch.ones_like(key, dtype=torch.bool)
        first[1:] = key[1:] != key[:-1]
        seg = torch.cumsum(first, 0) - 1
        at = torch.arange(key.numel(), device=dev)
        rank = at - at[first][seg]                              # the position of an entry among its duplicates
        key = key[first]
        total = torch.zeros(key.numel(), dtype=torch.float64, device=dev)
        for d in range(int(rank.max()) + 1 if rank.numel() else 0):      # one read-back, a one-time stage; 1 round without duplicates
            pick = rank == d
            total[seg[pick]] += w[pick]                         # distinct targets per round: no atomics
        val = total.float()
    indptr = torch.searchsorted(key, torch.arange(N + 1, device=dev) * N)
    return indptr, key % N if N else key, val.contiguous()


def uniform_start(num_nodes, dim, seed, device):
    """float32 [N, dim] uniform in [0, 1): y[i, c] = (draw(seed, i, c) >> 40) 2^-24, the library's counter-based stream."""
    lib = _lib.load()
    y = torch.empty(num_nodes, dim, dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        _lib.check(lib.ampconv_spring_start(y.data_ptr(), num_nodes, dim, int(seed) & (2 ** 64 - 1), _stream()), 'ampconv_spring_start')
    return y


class SpringLayout:
    """The device state of the iteration: y in two buffers, the CSR, rep, the workspaces and
    state = {t, dt, ran, done} (float64 [4]; state_int is the same memory as int64).  step() is one iteration
    (ampconv_spring_repulsion, ampconv_spring_step); once done is set it copies y and changes nothing else.  part
    (tests): the part length, through ampconv_spring_step_split."""

    def __init__(self, y0, indptr, indices, val, k, iterations, threshold=1e-4, fixed=None, part=None):
        self.lib = _lib.load()
        dev = y0.device
        self.N, self.dim, self.nnz = y0.size(0), y0.size(1), indices.numel()
        # both buffers dense row-major whatever the strides of y0 (a transposed view is a legal start): the kernels read
        # and write them as [N, dim] arrays
        first = y0.detach().clone(memory_format=torch.contiguous_format)
        self.y = [first, torch.empty_like(first)]
        self.indptr, self.indices = indptr.contiguous(), indices.contiguous()
        self.val = None if val is None else val.contiguous()
        self.fixed = None if fixed is None else fixed.to(torch.uint8).contiguous()
        self.k, self.threshold, self.part = float(k), float(threshold), part
        first_two = y0[:, :2].double()
        t0 = (first_two.max(dim=0).values - first_two.min(dim=0).values).max() * 0.1     # networkx: the first two columns only
        self.state = torch.zeros(4, dtype=torch.float64, device=dev)
        # tensor / tensor: an IEEE division (a division by a Python number is a product with its reciprocal)
        self.state[0], self.state[1] = t0, t0 / torch.tensor(float(int(iterations) + 1), dtype=torch.float64, device=dev)
        self.state_int = self.state.view(torch.int64)
        self.rep = torch.empty(self.N, self.dim, dtype=torch.float64, device=dev)
        self.ws_rep = torch.empty(max(int(self.lib.ampconv_spring_repulsion_workspace_bytes(self.N, self.dim)), 256),
                                  dtype=torch.uint8, device=dev)
        self.ws_step = torch.empty(max(int(self.lib.ampconv_spring_step_workspace_bytes(self.N, self.nnz, self.dim)), 256),
                                   dtype=torch.uint8, device=dev)

    def repulsion(self):
        """ampconv_spring_repulsion of the current positions into self.rep (left as it is once done is set)."""
        with torch.cuda.device(self.y[0].device):
            _lib.check(self.lib.ampconv_spring_repulsion(self.y[0].data_ptr(), self.N, self.dim, self.rep.data_ptr(),
                                                         self.state.data_ptr(), self.ws_rep.data_ptr(), self.ws_rep.numel(),
                                                         _stream()), 'ampconv_spring_repulsion')

    def step(self):
        lib, (y_in, y_out) = self.lib, self.y
        self.repulsion()
        head = (y_in.data_ptr(), y_out.data_ptr(), self.N, self.dim, self.indptr.data_ptr(), _lib.ptr(self.indices if self.nnz else None),
                _lib.ptr(self.val), self.nnz, _lib.ptr(self.fixed), self.rep.data_ptr(), self.k, self.threshold, self.state.data_ptr())
        with torch.cuda.device(y_in.device):
            tail = (self.ws_step.data_ptr(), self.ws_step.numel(), _stream())
            if self.part is None:
                _lib.check(lib.ampconv_spring_step(*head, *tail), 'ampconv_spring_step')
            else:
                _lib.check(lib.ampconv_spring_step_split(*head, int(self.part), *tail), 'ampconv_spring_step_split')
        self.y = [y_out, y_in]

    @property
    def iterations_run(self):
        """The iterations that moved the positions (a read-back)."""
        return int(self.state_int[2])


class SpringResult:
    """pos float32 [N, dim]; graph = (indptr, indices, val), the CSR that was laid out; k, the optimal distance as
    used; iterations_run (a property: the one read-back, taken only when asked for), the iterations before networkx's
    stopping rule held, at most `iterations`."""

    def __init__(self, pos, graph, k, state=None):
        self.pos, self.graph, self.k, self._state = pos, graph, k, state

    @property
    def iterations_run(self):
        return 0 if self._state is None else int(self._state[2])


def rescale(y, scale, center):
    """networkx's rescale_layout(pos, scale) + center on the device: the fp64 column means subtracted, times
    scale / max|y| (skipped where the maximum is 0), plus center; rounded to float32 once."""
    y = y.double()
    y = y - y.mean(dim=0)
    lim = y.abs().max()
    y = y * torch.where(lim > 0, scale / lim, torch.ones_like(lim))
    return (y + center).float()


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def _check(edge_index, num_nodes, weight, symmetric, dim, k, pos, fixed, iterations, threshold, scale, center, seed):
    if not isinstance(edge_index, torch.Tensor) or edge_index.dim() != 2 or edge_index.size(0) != 2 or edge_index.dtype != torch.int64:
        raise ValueError(f'spring_layout: edge_index has to be an int64 [2, E] tensor; {_SUPPORTED}')
    if isinstance(num_nodes, bool) or not isinstance(num_nodes, int) or not 0 <= num_nodes <= MAX_N:
        raise ValueError(f'spring_layout: num_nodes = {num_nodes!r} has to be an integer in [0, {MAX_N}]')
    if isinstance(dim, bool) or not isinstance(dim, int) or dim not in (2, 3):
        raise ValueError(f'spring_layout: dim = {dim!r} has to be 2 or 3')
    if not isinstance(symmetric, bool):
        raise ValueError(f'spring_layout: symmetric = {symmetric!r} has to be a bool')
    dev, E, N = edge_index.device, edge_index.size(1), num_nodes
    if N == 0 and E:
        raise ValueError('spring_layout: edges given for a graph without nodes')
    if weight is not None:
        if symmetric:
            raise ValueError('spring_layout: weights describe directed entries: pass symmetric=False (and both directions '
                             'of an undirected edge)')
        if not isinstance(weight, torch.Tensor) or not weight.is_floating_point() or tuple(weight.shape) != (E,) or weight.device != dev:
            raise ValueError(f'spring_layout: weight has to be a float [{E}] tensor on the device of edge_index')
        if weight.requires_grad:
            raise ValueError('spring_layout: weight requires grad, and the layout has no autograd (pass weight.detach())')
    if k is not None and (not _number(k) or not k > 0):
        raise ValueError(f'spring_layout: k = {k!r} has to be None or a positive number')
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 0 <= iterations <= 1 << 24:
        raise ValueError(f'spring_layout: iterations = {iterations!r} has to be a non-negative integer')
    if not _number(threshold):
        raise ValueError(f'spring_layout: threshold = {threshold!r} has to be a finite number')
    if scale is not None and not _number(scale):
        raise ValueError(f'spring_layout: scale = {scale!r} has to be None or a finite number')
    if center is not None:
        try:
            center = [float(v) for v in center]
        except (TypeError, ValueError):
            raise ValueError(f'spring_layout: center = {center!r} has to be None or {dim} numbers') from None
        if len(center) != dim or not all(math.isfinite(v) for v in center):
            raise ValueError('spring_layout: length of center coordinates must match dimension of layout')
    if isinstance(seed, bool) or not isinstance(seed, int):
        raise ValueError(f'spring_layout: seed = {seed!r} has to be an integer')
    if pos is not None:
        if not isinstance(pos, torch.Tensor) or pos.dtype != torch.float32 or tuple(pos.shape) != (N, dim) or pos.device != dev:
            raise ValueError(f'spring_layout: pos has to be a float32 [{N}, {dim}] tensor on the device of edge_index (rows of NaN: '
                             'no position given)')
        if pos.requires_grad:
            raise ValueError('spring_layout: pos requires grad, and the layout has no autograd (pass pos.detach())')
    if fixed is not None:
        if pos is None:
            raise ValueError('spring_layout: nodes are fixed without positions given')
        ok = isinstance(fixed, torch.Tensor) and fixed.device == dev and (
            (fixed.dtype == torch.bool and tuple(fixed.shape) == (N,)) or (fixed.dtype == torch.int64 and fixed.dim() == 1))
        if not ok:
            raise ValueError(f'spring_layout: fixed has to be a bool [{N}] mask or an int64 tensor of node ids on the device of '
                             'edge_index')
    if not edge_index.is_cuda:
        raise ValueError(f'spring_layout: edge_index has to be on the GPU; {_SUPPORTED}')
    return center


def spring_layout(edge_index, num_nodes, *, weight=None, symmetric=True, dim=2, k=None, pos=None, fixed=None, iterations=50,
                  threshold=1e-4, scale=1.0, center=None, seed=0):
    """networkx's spring_layout(G, k, pos, fixed, iterations, threshold, weight, scale, center, dim, seed) of the graph
    with nodes 0 .. num_nodes - 1 and the edges edge_index [2, E] (`adjacency` turns them into the matrix networkx
    reads: symmetric=True is an undirected Graph, symmetric=False a DiGraph, weight the edge attribute).  pos: a float32
    [N, dim] start, rows of NaN where no position is given (those start at rand dom_size + center); None: uniform in
    [0, 1) from the library's stream under `seed`.  fixed: a bool [N] mask or int64 node ids that keep their given
    position; with fixed nodes there is no rescaling, and k defaults to dom_size / sqrt(N).  scale=None: no rescaling.
    Returns a SpringResult; nothing carries a gradient and two runs give the same bits.  Invalid arguments raise
    ValueError before any stage of the layout runs (adjacency, start, iteration, rescaling); what can only be told from
    the values -- node ids out of range, a fixed node without a position, an infinite coordinate -- costs a few torch
    reductions and one read-back first."""
    center = _check(edge_index, num_nodes, weight, symmetric, dim, k, pos, fixed, iterations, threshold, scale, center, seed)
    N, dev = num_nodes, edge_index.device
    center_t = torch.tensor(center if center is not None else [0.0] * dim, dtype=torch.float64, device=dev)
    if N == 0:
        return SpringResult(torch.empty(0, dim, dtype=torch.float32, device=dev), None, k)
    if N == 1:
        return SpringResult(center_t.float()[None, :], None, k)
    edge_index = edge_index.detach()
    if bool(((edge_index < 0) | (edge_index >= N)).any()):
        raise ValueError(f'spring_layout: edge_index names nodes outside [0, {N})')
    mask = None
    if fixed is not None:
        if fixed.dtype == torch.bool:
            mask = fixed
        else:
            if bool(((fixed < 0) | (fixed >= N)).any()):
                raise ValueError(f'spring_layout: fixed names nodes outside [0, {N})')
            mask = torch.zeros(N, dtype=torch.bool, device=dev)
            mask[fixed] = True
    dom_size = 1.0
    if pos is not None:
        given = ~torch.isnan(pos).any(dim=1)
        facts = torch.stack((given.all().double(), given.any().double(), torch.where(given[:, None], pos, pos.new_full((), -math.inf)).max().double(),
                             (given | ~mask).all().double() if mask is not None else given.new_ones(()).double(),
                             torch.isinf(pos).any().double())).cpu()
        if not bool(facts[3]):
            raise ValueError('spring_layout: nodes are fixed without positions given')
        if bool(facts[1]) and float(facts[2]) != 0:
            dom_size = float(facts[2])
        if bool(facts[4]):
            raise ValueError('spring_layout: pos holds an infinite coordinate')
        y0 = pos.detach()
        if not bool(facts[0]):
            rand = (uniform_start(N, dim, seed, dev).double() * dom_size + center_t).float()
            y0 = torch.where(given[:, None], y0, rand)
    else:
        y0 = uniform_start(N, dim, seed, dev)
    if k is None:
        k = (dom_size if fixed is not None else 1.0) / math.sqrt(N)
    graph = adjacency(edge_index, N, None if weight is None else weight.detach(), symmetric)
    state = SpringLayout(y0, *graph, k, iterations, threshold, mask)
    for _ in range(iterations):
        state.step()
    y = state.y[0]
    if fixed is None and scale is not None:
        y = rescale(y, float(scale), center_t)
    return SpringResult(y, graph, float(k), state.state_int)
