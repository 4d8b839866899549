"""AMPConv -- drop-in for reference src/ampnet/conv/amp_conv.py:9-51 on MI355X.

Same constructor, method names, attribute names and state-dict keys as the
reference class:

    AMPConv(embed_dim, num_heads)                       amp_conv.py:10
    .forward(x, edge_index) -> [N, L*D]                 amp_conv.py:24-26
    .message(x_i, x_j)      -> [E, L*D]                 amp_conv.py:28-51
    .aggregate(inputs, index, dim_size=N) (aggr='mean') amp_conv.py:11
    .multi_head_attention   (nn.MultiheadAttention: parameter container, identical
                             init and keys `multi_head_attention.in_proj_weight` ...)
    .attn_output [E, L, D], .attn_output_weights [E, L, L]   amp_conv.py:12-13,39

All arithmetic runs in libampconv.so (hand-written HIP for gfx950) plus dense
GEMMs on the per-node rows; there is no CPU or eager fallback -- inputs that are
not on the GPU, or a missing shared library, raise.
"""
import os
import warnings

import torch
import torch.nn as nn

from .. import _lib
from ..graph import EdgeCSR, graph_cache
from . import functional as F_
from . import linear as FL_

try:                                            # PyG is optional (absent in the build image)
    from torch_geometric.nn import MessagePassing as _PyGMessagePassing
except Exception:                               # pragma: no cover - depends on the environment
    _PyGMessagePassing = None


class InvalidConfiguration(ValueError, RuntimeError):
    """x.shape[1] is not a multiple of embed_dim (the reference prints
    "Error, invalid configuration" and then torch.reshape raises RuntimeError,
    amp_conv.py:32-35)."""


class _MessagePassingBase(nn.Module):
    """Minimal stand-in with PyG's method names when torch_geometric is absent."""

    def __init__(self, aggr='mean'):
        super().__init__()
        self.aggr = aggr

    def update(self, inputs):
        return inputs


MessagePassing = _PyGMessagePassing if _PyGMessagePassing is not None else _MessagePassingBase


class AMPConv(MessagePassing):
    def __init__(self, embed_dim, num_heads, softmax=True):
        """softmax=False: the reference's softmax-free attention (its custom_multihead_attn.py copy,
        amp_conv.py:6,17; conv/linear.py here) -- same parameters and state-dict keys."""
        super().__init__(aggr='mean')
        self.softmax = bool(softmax)
        self._attn_ctx = None
        self._attn_plane_bounds = None
        self._attn_output = None
        self._attn_output_weights = None
        # what the lazy per-edge outputs (attn_output, attn_output_weights) need is the projection
        # buffer [N*L, 3D] -- 61 GB at BASELINE config 4.  True: always keep it until the next forward;
        # False: never; 'auto' (default): keep it while it is at most AMPCONV_RETAIN_LIMIT_MB (512 MiB:
        # every graph the reference's scripts visualise), drop it above -- reading the attributes then
        # raises instead of pinning tens of GB after backward.
        self.retain_attention = 'auto'
        self._attn_dropped_bytes = 0
        self._attn_token_only = False         # the last call was forward_token (fast path): no per-edge side outputs
        self._attn_param_versions = None
        # how the per-node projections run: 'native' (default: libampconv's own kernels, csrc/proj_gemm.hip -- fp32
        # operands as two fp16 planes of the power-of-two-scaled value, three partial products on the matrix cores
        # (operands of 2^24 elements and more; below that three bf16 planes, six products), fp32 accumulate, error
        # below the fp32 library GEMM's; fp32 storage with embed_dim % 4 == 0 -- tiles are padded inside, so the
        # reference's default 100 is served --, anything else falls to 'fp32') | 'fp32' (library
        # GEMMs, rocBLAS) | 'bf16x3' (hipBLASLt's 3-product split, 8x the error) -- functional.gemm_precision
        self.gemm_precision = os.environ.get('AMPCONV_GEMM', 'native')
        self.num_heads = num_heads
        self.embed_dim = embed_dim
        # parameter container only: same init RNG consumption and state-dict keys as the reference
        self.multi_head_attention = nn.MultiheadAttention(
            embed_dim=embed_dim, num_heads=num_heads, batch_first=True, bias=True)

    # ------------------------------------------------------------------ checks
    def _check_x(self, x, name='x'):
        if x.dim() != 2:
            raise ValueError(f'{name} must be [num_nodes, L*embed_dim], got {tuple(x.shape)}')
        if x.shape[1] % self.embed_dim != 0:
            print("Error, invalid configuration")           # amp_conv.py:32-33
            raise InvalidConfiguration(
                f'{name}.shape[1]={x.shape[1]} is not a multiple of embed_dim={self.embed_dim}')
        if not x.is_cuda:
            raise ValueError('ampnet_amd.AMPConv runs on the GPU only (no CPU fallback): '
                             f'{name} is on {x.device}')
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f'{name} must be float32 (or bfloat16 with a bfloat16 layer), got {x.dtype}')
        p = self.multi_head_attention.in_proj_weight
        if p.device != x.device:
            raise ValueError(f'parameters are on {p.device} but {name} is on {x.device}')

    def _check_linear(self, x):
        if x.dtype != torch.float32:
            raise ValueError('the softmax-free variant runs in float32 only')

    def _params(self):
        m = self.multi_head_attention
        return m.in_proj_weight, m.in_proj_bias, m.out_proj.weight, m.out_proj.bias

    # ------------------------------------------------------------------ forward
    def forward(self, x, edge_index):
        out = self.propagate(edge_index, x=x)
        return out

    def propagate(self, edge_index, size=None, **kwargs):
        """Fused gather -> attention -> mean -> out-projection (one pass, HIP)."""
        x = kwargs['x']
        self._check_x(x)
        _lib.load()
        if edge_index.device != x.device:
            raise ValueError(f'edge_index is on {edge_index.device} but x is on {x.device}')
        csr = graph_cache.get(edge_index, x.size(0))
        # the previous call's projection buffer goes before this call allocates its own (peak memory)
        self._attn_ctx = self._attn_output = self._attn_output_weights = None
        bounds = None
        if self.softmax:
            # (third output of a self-attention call: None, or -- the projections left their kernel in the plane format
            # of the 16-bit edge passes -- the device bounds that read `qkv` back, functional.planes_to_f32)
            y, qkv, bounds = F_.AMPConvFunction.apply(x, x, *self._params(), csr, self.num_heads, True,
                                                      _lib.AMPCONV_F32, self.gemm_precision)
        else:
            self._check_linear(x)
            y, qkv, _ = FL_.LinearAMPConvFunction.apply(x, x, *self._params(), csr, self.num_heads, True,
                                                        self.gemm_precision)
        L = x.size(1) // self.embed_dim
        self._set_attn_ctx(qkv, None, edge_index, L, shared=True, plane_bounds=bounds)
        return y

    def forward_token(self, x, edge_index, token=0):
        """`self.forward(x, edge_index).view(N, L, D)[:, token]`, values and gradients (to x and the four parameters),
        [N, embed_dim]: the layer for a model that reads ONE token of its output (AMPGCN(average_pooling_flag=False)
        reads token 0 of conv2, amp_gcn.py:266-271).  The query rows are x.view(N, L, D)[:, token]; the Q projection, the
        out-projection and their gradients run over N rows instead of N * L, the edge passes are the one-query-token
        family (csrc/edge_token.hip; functional.AMPConvTokenFunction).  Where that family does not serve the shape
        (ampconv_token_supported), for softmax=False layers and under AMPCONV_FORCE_GENERIC=1 this IS the full layer and
        a slice.  The per-edge side outputs (attn_output, attn_output_weights, attention_heatmap) are not available
        after this call: they raise."""
        self._check_x(x)
        D = self.embed_dim
        N, L = x.size(0), x.size(1) // D
        token = int(token)
        if not 0 <= token < L:
            raise ValueError(f'token must be in [0, {L}), got {token}')
        if (not self.softmax or os.environ.get('AMPCONV_FORCE_GENERIC', '0')[:1] == '1'
                or not F_.token_supported(L, D, self.num_heads, x.dtype)):
            return self.forward(x, edge_index).view(N, L, D)[:, token]
        if edge_index.device != x.device:
            raise ValueError(f'edge_index is on {edge_index.device} but x is on {x.device}')
        csr = graph_cache.get(edge_index, N)
        self._attn_ctx = self._attn_output = self._attn_output_weights = None
        self._attn_dropped_bytes = 0
        self._attn_token_only = True
        return F_.AMPConvTokenFunction.apply(x.reshape(N, L, D)[:, token], x, *self._params(), csr, self.num_heads,
                                             self.gemm_precision)

    def message(self, x_i, x_j):
        """Pass messages from nodes x_j to nodes x_i: per-edge cross-attention of the
        pre-gathered pairs, [E, L*D] (amp_conv.py:28-51)."""
        self._check_x(x_i, 'x_i')
        self._check_x(x_j, 'x_j')
        if x_i.shape != x_j.shape:
            raise ValueError(f'x_i {tuple(x_i.shape)} and x_j {tuple(x_j.shape)} differ')
        E = x_i.size(0)
        csr = EdgeCSR.identity(E, x_i.device)
        self._attn_ctx = self._attn_output = self._attn_output_weights = None
        if self.softmax:
            y, q, kv = F_.AMPConvFunction.apply(x_i, x_j, *self._params(), csr, self.num_heads, False,
                                                _lib.AMPCONV_F32, self.gemm_precision)
        else:
            self._check_linear(x_i)
            y, q, kv = FL_.LinearAMPConvFunction.apply(x_i, x_j, *self._params(), csr, self.num_heads, False,
                                                       self.gemm_precision)
        ar = torch.arange(E, dtype=torch.int64, device=x_i.device)
        L = x_i.size(1) // self.embed_dim
        self._set_attn_ctx(q, kv, torch.stack([ar, ar]), L, shared=False)
        self._attn_output = y.view(E, L, self.embed_dim)
        return y

    def aggregate(self, inputs, index, ptr=None, dim_size=None):
        """aggr='mean' scatter of [E, F] messages to dim_size rows (zero rows where
        nothing arrives; testing_message_passing_pyg.py:37-40)."""
        if not inputs.is_cuda:
            raise ValueError('ampnet_amd.AMPConv runs on the GPU only (no CPU fallback)')
        n = int(dim_size) if dim_size is not None else int(index.max().item()) + 1
        ar = torch.arange(index.numel(), dtype=torch.int64, device=index.device)
        csr = EdgeCSR(torch.stack([ar % n, index.to(torch.int64)]), n)
        return F_.segment_mean(inputs.to(torch.float32), csr, index.to(torch.int64))

    # ------------------------------------------------------------------ lazy per-edge outputs
    def _set_attn_ctx(self, q_buf, kv_buf, edge_index, L, shared, plane_bounds=None):
        self._attn_output = None
        self._attn_output_weights = None
        self._attn_ctx = None
        self._attn_dropped_bytes = 0
        self._attn_token_only = False
        nbytes = q_buf.numel() * q_buf.element_size() + (0 if kv_buf is None else kv_buf.numel() * kv_buf.element_size())
        keep = self.retain_attention
        if keep == 'auto':
            keep = nbytes <= (int(os.environ.get('AMPCONV_RETAIN_LIMIT_MB', 512)) << 20)
        if not keep:
            self._attn_dropped_bytes = nbytes
            return
        self._attn_ctx = (q_buf.detach(), None if kv_buf is None else kv_buf.detach(),
                          edge_index, L, shared)
        self._attn_plane_bounds = None if plane_bounds is None else plane_bounds.detach()
        # attn_output is produced lazily with the out-projection parameters: remember which version
        # of them the forward pass saw (an optimizer step in between changes the result)
        m = self.multi_head_attention
        self._attn_param_versions = (m.out_proj.weight._version, m.out_proj.bias._version)

    def _attn_missing(self, name):
        if getattr(self, '_attn_token_only', False):
            raise RuntimeError(f'{name} is not available after forward_token: that call projects ONE query row per node '
                               f'and keeps no [N*L, 3D] projection buffer; run forward() for the per-edge outputs')
        if self._attn_dropped_bytes:
            raise RuntimeError(
                f'{name} was not retained: the projection buffer of the last forward is '
                f'{self._attn_dropped_bytes / 2**30:.1f} GiB (retain_attention={self.retain_attention!r}); set '
                f'layer.retain_attention = True before the forward pass to keep it')
        return None

    def _attn_views(self):
        q_buf, kv_buf, edge_index, L, shared = self._attn_ctx
        if getattr(self, '_attn_plane_bounds', None) is not None:      # plane format -> fp32, once
            with torch.cuda.device(q_buf.device):
                q_buf = F_.planes_to_f32(q_buf, F_.Scalars(bounds=self._attn_plane_bounds).qkv_bound,
                                         self.embed_dim // self.num_heads)
            self._attn_ctx = (q_buf, kv_buf, edge_index, L, shared)
            self._attn_plane_bounds = None
        if q_buf.dtype != torch.float32:              # side outputs are served in fp32
            q_buf = q_buf.float()
            kv_buf = None if kv_buf is None else kv_buf.float()
            self._attn_ctx = (q_buf, kv_buf, edge_index, L, shared)
        D = self.embed_dim
        return *F_._qkv_views(q_buf, kv_buf, L, D, D // self.num_heads), edge_index, L

    @property
    def attn_output_weights(self):
        """[E, L, L]: w[e, row, col] = how much destination token `row` attends to source
        token `col`, mean over heads, original edge order (amp_conv.py:43-47)."""
        if self._attn_output_weights is None and self._attn_ctx is None:
            return self._attn_missing('attn_output_weights')
        if self._attn_output_weights is None:
            Qv, Kv, _, edge_index, L = self._attn_views()
            weights = F_.attention_weights if self.softmax else FL_.attention_scores
            self._attn_output_weights = weights(Qv, Kv, edge_index.contiguous(), L, self.embed_dim,
                                                self.num_heads)
        return self._attn_output_weights

    @attn_output_weights.setter
    def attn_output_weights(self, value):
        self._attn_output_weights = value

    @property
    def attn_output(self):
        """[E, L, D] per-edge attention output after the out-projection (amp_conv.py:39)."""
        if self._attn_output is None and self._attn_ctx is None:
            return self._attn_missing('attn_output')
        if self._attn_output is None:
            m = self.multi_head_attention
            if self._attn_param_versions != (m.out_proj.weight._version, m.out_proj.bias._version):
                warnings.warn('attn_output is computed lazily with the CURRENT out_proj parameters, which changed '
                              'since the forward pass (the reference stores the forward-time value): read it '
                              'before optimizer.step()', RuntimeWarning, stacklevel=2)
            Qv, Kv, Vv, edge_index, L = self._attn_views()
            D, H = self.embed_dim, self.num_heads
            E = edge_index.size(1)
            if not self.softmax:
                self._attn_output = self._linear_attn_output(edge_index, L)
                return self._attn_output
            ident = EdgeCSR.identity(E, edge_index.device)
            ident.col = edge_index[0].to(torch.int32).contiguous()
            qidx = edge_index[1].to(torch.int32).contiguous()
            o = torch.empty(E * L, D, dtype=torch.float32, device=edge_index.device)
            with torch.cuda.device(edge_index.device):
                F_.edge_forward(Qv, Kv, Vv, ident, E, L, D, H, o, qidx=qidx,
                                dtype=_lib.AMPCONV_F32)   # fp32 views (see _attn_views)
            m = self.multi_head_attention
            with torch.no_grad():
                self._attn_output = torch.addmm(m.out_proj.bias.float(), o,
                                                m.out_proj.weight.float().t()).view(E, L, D)
        return self._attn_output

    def attention_heatmap(self, token_features, src_features=None, dst_features=None, *, num_features=None,
                          **selection):
        """[rows, cols] float64 feature-to-feature heatmap of the last forward pass: the mean attention weight between
        tokens of source feature `src_features[r]` and destination feature `dst_features[c]` over the selected edges
        (the reference's calculate_attn_heatmap, visualize_cora_attn_coeffs.py:212-216) -- one
        heatmap.AttentionHeatmap.update followed by .result(); `selection`: edge_mask / node_class, src_class,
        dst_class.  Accumulated on the GPU without forming attn_output_weights."""
        from ..heatmap import AttentionHeatmap
        return AttentionHeatmap(src_features, dst_features, num_features).update(self, token_features,
                                                                                 **selection).result()

    def _linear_attn_output(self, edge_index, L):
        """Per-edge output of the softmax-free variant, [E, L, D]: Q_d (K_s^T V_s) / sqrt(dh), then the
        out-projection (a diagnostic for small graphs, like the reference's E-sized attribute)."""
        q_buf, kv_buf, _, _, shared = self._attn_ctx
        D, H = self.embed_dim, self.num_heads
        dh = D // H
        src, dst = edge_index[0], edge_index[1]
        with torch.no_grad():
            if shared:
                N = q_buf.size(0) // L
                q = q_buf[:, :D].reshape(N, L, H, dh)[dst]
                k = q_buf[:, D:2 * D].reshape(N, L, H, dh)[src]
                v = q_buf[:, 2 * D:].reshape(N, L, H, dh)[src]
            else:
                E = edge_index.size(1)
                q = q_buf.reshape(E, L, H, dh)
                k, v = kv_buf[:, :D].reshape(E, L, H, dh), kv_buf[:, D:].reshape(E, L, H, dh)
            m = torch.einsum('elhi,elhj->ehij', k, v)
            o = torch.einsum('elhi,ehij->elhj', q, m).reshape(-1, D) / (dh ** 0.5)
            mha = self.multi_head_attention
            return torch.addmm(mha.out_proj.bias, o, mha.out_proj.weight.t()).view(-1, L, D)

    @attn_output.setter
    def attn_output(self, value):
        self._attn_output = value
