"""GCNConv on the HIP path: PyG 2.0-2.1's layer restated (parity with PyG itself is unpinned: include/ampconv.h,
"GCN baseline", is the specification).

    out = A_hat (x lin.weight^T) + bias,    A_hat = D^-1/2 (A + fill I) D^-1/2 after gcn_norm's self-loop step

Same constructor names, sub-module `lin` (no bias, Glorot-uniform) and parameter `bias` (zeros) as the reference's
`from torch_geometric.nn import GCNConv` (src/ampnet/module/gcn_classifier.py:13,52-55), so the state-dict keys are
`lin.weight` and `bias`.  Out of scope: normalize=False, edge_weight, cached=True.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ..gcn import gcn_aggregate


class GCNConv(nn.Module):
    def __init__(self, in_channels, out_channels, improved=False, add_self_loops=True, bias=True, normalize=True):
        super().__init__()
        if not normalize:
            raise ValueError('GCNConv(normalize=False) is out of scope: the kernels form the symmetric normalisation '
                             'on the fly (ampnet_amd has no eager fallback)')
        if int(in_channels) < 1 or int(out_channels) < 1:
            raise ValueError(f'GCNConv needs in_channels, out_channels >= 1, got {in_channels}, {out_channels}')
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.improved, self.add_self_loops = bool(improved), bool(add_self_loops)
        self.lin = nn.Linear(self.in_channels, self.out_channels, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.empty(self.out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin.weight)               # PyG: Linear(weight_initializer='glorot')
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def aggregate(self, h, edge_index):
        """A_hat h + bias for an already transformed h [N, out_channels]."""
        return gcn_aggregate(h, edge_index, self.bias, self.improved, self.add_self_loops)

    def forward(self, x, edge_index):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise ValueError('GCNConv needs its input on the GPU (ampnet_amd has no CPU fallback)')
        if x.dtype != torch.float32:
            raise ValueError(f'GCNConv takes float32, got {x.dtype}')
        if x.dim() != 2 or x.size(1) != self.in_channels:
            raise ValueError(f'GCNConv expects [N, {self.in_channels}], got {tuple(x.shape)}')
        return self.aggregate(F.linear(x, self.lin.weight), edge_index)

    def extra_repr(self):
        return f'{self.in_channels}, {self.out_channels}, improved={self.improved}, add_self_loops={self.add_self_loops}'
