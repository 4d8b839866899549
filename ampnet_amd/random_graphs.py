"""Random graphs with class structure, drawn on the GPU (csrc/sbm.hip): the link data of the reference's
`create_xor_data` (synthetic_benchmark/synthetic_xor.py:104-165: two nested Python loops over an [N, N] matrix and two
more to list the edges) and the graph of its `Random_Partition_Graph` (synthetic_rpg.py:39-121, networkx's random
partition graph).  Both are stochastic block models.

`stochastic_block_model(sizes, p, ...)` draws what include/ampconv.h ("THE BLOCK MODEL") states: every unit (node u,
block b) walks its candidates with geometric skips from the library's counter-based stream, so the work follows the edges
and not the N^2 pairs, every pair is an independent Bernoulli trial -- the distribution of networkx's
`stochastic_block_model(sizes, p, directed=, selfloops=)` -- and a (sizes, p, flags, seed) tuple gives the same
edge_index element for element on any device.  That text and the numpy model in tests/sbm_reference.py are the
specification; bit parity with networkx's or the reference's random stream is not possible and not claimed.  Three steps:
ampconv_sbm_count, one torch.cumsum, ampconv_sbm_fill; the host reads the total back once, to allocate.  No atomics: two
runs give the same bits.  There is no CPU fallback: a non-GPU device raises ValueError.
"""
import math

import numpy as np
import torch

from . import _lib
from .graph import _stream

MAX_K = _lib.SBM_MAX_K
MAX_E = MAX_N = 2 ** 31 - 1


class BlockModelGraph:
    """edge_index int64 [2, E] and block int64 [N] on the device, num_nodes.  Directed: the edges in row-major
    (row, col) order.  Undirected: the pairs u <= v in that order, then their mirrors (v, u), v != u, in the same order."""

    def __init__(self, edge_index, block, num_nodes):
        self.edge_index, self.block, self.num_nodes = edge_index, block, num_nodes

    def __iter__(self):                        # edge_index, block, num_nodes = stochastic_block_model(...)
        return iter((self.edge_index, self.block, self.num_nodes))

    def __repr__(self):
        return f'BlockModelGraph(num_nodes={self.num_nodes}, num_edges={self.edge_index.size(1)})'


class XorLinkData:
    """x float32 [N, 2], y float32 [N], edge_index int64 [2, E], num_nodes: create_xor_data's tensors without the dense
    adjacency matrix."""

    def __init__(self, x, y, edge_index, num_nodes):
        self.x, self.y, self.edge_index, self.num_nodes = x, y, edge_index, num_nodes

    def __iter__(self):
        return iter((self.x, self.y, self.edge_index, self.num_nodes))


def _validate(sizes, p, directed):
    """(sizes int64 [K], P float64 [K, K]) as numpy arrays, or ValueError.  Runs before the library is loaded."""
    try:
        s = np.asarray(sizes)
        P = np.asarray(p, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f'sizes and p have to be numeric arrays: {e}') from None
    if s.ndim != 1 or s.size == 0:
        raise ValueError(f'sizes has to be a non-empty list of block sizes, got shape {s.shape}')
    if s.dtype.kind not in 'iu' and not (s.dtype.kind == 'f' and np.isfinite(s).all() and (s == np.floor(s)).all()):
        raise ValueError('sizes has to hold integers')
    if (s < 0).any():
        raise ValueError('sizes has to be non-negative')
    K = s.size
    if K > MAX_K:
        raise ValueError(f'{K} blocks: at most {MAX_K} (AMPCONV_SBM_MAX_K)')
    if int(s.astype(object).sum()) > MAX_N:
        raise ValueError(f'sum(sizes) has to be at most {MAX_N}')
    if P.shape != (K, K):
        raise ValueError(f'p has to be [{K}, {K}] for {K} blocks, got shape {P.shape}')
    if not np.isfinite(P).all():
        raise ValueError('p has to be finite')
    if (P < 0).any() or (P > 1).any():
        raise ValueError('every entry of p has to lie in [0, 1]')
    if not directed and not np.array_equal(P, P.T):
        raise ValueError('p has to be symmetric for an undirected graph')
    return s.astype(np.int64), np.ascontiguousarray(P)


def _device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise ValueError(f'device {dev}: the generator runs on the GPU (ampnet_amd has no CPU fallback)')
    return torch.device('cuda', torch.cuda.current_device()) if dev.index is None else dev


def stochastic_block_model(sizes, p, *, directed=False, selfloops=False, seed=0, device='cuda'):
    """The stochastic block model of include/ampconv.h: block b holds sizes[b] consecutive nodes, a pair (u, v) is an
    edge with probability p[block(u)][block(v)] (p [K, K], symmetric unless directed), independently.  Returns a
    BlockModelGraph.  More than 2^31 - 1 edges: ValueError, before any is written."""
    s, P = _validate(sizes, p, directed)
    dev = _device(device)
    lib = _lib.load()
    K, N = s.size, int(s.sum())
    seed = int(seed) & (2 ** 64 - 1)
    with np.errstate(divide='ignore'):
        lq = np.log1p(-P)                                            # the table of THE BLOCK MODEL: host fp64
    block = torch.repeat_interleave(torch.arange(K, device=dev), torch.from_numpy(s).to(dev), output_size=N)
    if N == 0:
        return BlockModelGraph(torch.empty(2, 0, dtype=torch.int64, device=dev), block, 0)
    P_d, lq_d = torch.from_numpy(P).to(dev), torch.from_numpy(lq).to(dev)
    mirrors = not directed
    # count and, for the undirected graph with self loops, the mirror count: the rows of one tensor, so one scan
    counts = torch.empty(2 if mirrors and selfloops else 1, N * K, dtype=torch.int64, device=dev)
    head = (s.ctypes.data, K, P_d.data_ptr(), lq_d.data_ptr(), int(directed), int(selfloops), seed)
    with torch.cuda.device(dev):
        _lib.check(lib.ampconv_sbm_count(*head, counts[0].data_ptr(), counts[1].data_ptr() if counts.size(0) == 2 else None,
                                         _stream()), 'ampconv_sbm_count')
        ends = torch.cumsum(counts, dim=1)
        totals = ends[:, -1].tolist()                                # the one read-back: the sizes to allocate
        e_upper = totals[0]
        e_mirror = 0 if not mirrors else totals[-1]
        E = e_upper + e_mirror
        if E > MAX_E:
            raise ValueError(f'{E} edges: at most {MAX_E} (2^31 - 1); lower p or the sizes')
        edge_index = torch.empty(2, E, dtype=torch.int64, device=dev)
        if E:
            off = ends - counts                                      # exclusive
            moff = off[-1] if mirrors else None
            _lib.check(lib.ampconv_sbm_fill(*head, off[0].data_ptr(), _lib.ptr(moff), e_upper, edge_index[0].data_ptr(),
                                            edge_index[1].data_ptr(), E, _stream()), 'ampconv_sbm_fill')
    return BlockModelGraph(edge_index, block, N)


def random_partition_graph(sizes, p_in, p_out, *, directed=False, seed=0, device='cuda'):
    """The reference's Random_Partition_Graph (synthetic_rpg.py:39-58; networkx's random_partition_graph): nodes of the
    same group are linked with probability p_in (its Homophily), nodes of different groups with p_out (Heterophily); no
    self loops.  sizes: the group sizes (N_groups * [N_vertices] there)."""
    for name, v in (('p_in', p_in), ('p_out', p_out)):
        if not (isinstance(v, (int, float)) and 0.0 <= v <= 1.0):
            raise ValueError(f'{name} must be in [0, 1]')
    K = len(sizes)
    P = np.where(np.eye(K, dtype=bool), float(p_in), float(p_out))
    return stochastic_block_model(sizes, P, directed=directed, selfloops=False, seed=seed, device=device)


def gnp_random_graph(n, p, *, directed=False, seed=0, device='cuda'):
    """G(n, p): every pair an edge with probability p, no self loops (networkx's fast_gnp_random_graph)."""
    if not (isinstance(p, (int, float)) and 0.0 <= p <= 1.0):
        raise ValueError('p must be in [0, 1]')
    return stochastic_block_model([int(n)], [[float(p)]], directed=directed, selfloops=False, seed=seed, device=device)


XOR_CORNERS = ((0., 0.), (0., 1.), (1., 0.), (1., 1.))
XOR_LABELS = (0., 1., 1., 0.)


def xor_link_matrix(same_class_link_prob, diff_class_link_prob):
    """P [4, 4] of the XOR link data: P[a][b] by equality of the corner groups' labels."""
    y = np.asarray(XOR_LABELS)
    return np.where(y[:, None] == y[None, :], float(same_class_link_prob), float(diff_class_link_prob))


def xor_link_dataset(num_samples, noise_std=0.1, same_class_link_prob=0.7, diff_class_link_prob=0.1, seed=0, device='cuda'):
    """create_xor_data's data (synthetic_xor.py:104-165): four corner groups of num_samples // 4 nodes with labels
    [0, 1, 1, 0], x = corner + noise_std * randn (a torch generator seeded with `seed`), and a directed graph without
    self loops in which row -> col is an edge with same_class_link_prob or diff_class_link_prob by label equality.
    Returns an XorLinkData (x, y, edge_index, num_nodes); the dense adjacency matrix of the reference is not built."""
    if num_samples % 4 != 0 or num_samples < 0:
        raise ValueError('num_samples must be an integer divisible by 4.')
    for name, v in (('same_class_link_prob', same_class_link_prob), ('diff_class_link_prob', diff_class_link_prob)):
        if not (isinstance(v, (int, float)) and 0.0 <= v < 1.0):
            raise ValueError(f'{name} must be a float percent between 0 and 1.')
    if not (isinstance(noise_std, (int, float)) and math.isfinite(noise_std) and noise_std >= 0):
        raise ValueError('noise_std must be a finite non-negative number')
    dev = _device(device)
    repeats = num_samples // 4
    g = stochastic_block_model([repeats] * 4, xor_link_matrix(same_class_link_prob, diff_class_link_prob), directed=True,
                               selfloops=False, seed=seed, device=dev)
    gen = torch.Generator(device=dev).manual_seed(int(seed) & (2 ** 63 - 1))
    corners = torch.tensor(XOR_CORNERS, dtype=torch.float32, device=dev)
    labels = torch.tensor(XOR_LABELS, dtype=torch.float32, device=dev)
    x = corners[g.block] + float(noise_std) * torch.randn(num_samples, 2, generator=gen, dtype=torch.float32, device=dev)
    return XorLinkData(x, labels[g.block], g.edge_index, num_samples)
