"""ctypes binding of libampconv.so (C ABI declared in include/ampconv.h).

The product path has no fallback: if the shared library is missing or does not
export a symbol, importing/using the HIP path raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AMPCONV_LIB_PATH', os.path.join(_HERE, 'libampconv.so'))   # override: dev A/B builds

EXPECTED_ABI = 111          # AMPCONV_VERSION of include/ampconv.h this binding was written against

AMPCONV_F32 = 0
AMPCONV_BF16 = 1
DTYPES = {torch.float32: AMPCONV_F32, torch.bfloat16: AMPCONV_BF16}     # storage dtype -> the C ABI's code of it
PASS_FWD, PASS_DST, PASS_SRC = 0, 1, 2                                        # AMPCONV_PASS_*
FAMILY_BF16_MFMA, FAMILY_SMALL, FAMILY_MFMA, FAMILY_BLOCK, FAMILY_GENERIC = range(5)     # AMPCONV_FAMILY_*
HUB_CHUNK = int(os.environ.get('AMPCONV_HUB_CHUNK', 0))    # edges per chunk of a long CSR/CSC segment (include/ampconv.h, long segments); 0 = by size


def hub_chunk(num_edges):
    """Edges per chunk of a long segment.  64 on small graphs (a chunk is walked by ONE wave, so it bounds the launch's
    latency: ~1.5 us per edge), 128 from a million edges up (cfg5: 619 -> 611 ms per step, half the partial-tile
    workspace; 128-256 is a flat optimum once the main pass is XCD-balanced, tools/sweep_hub_chunk.sh)."""
    return HUB_CHUNK if HUB_CHUNK > 0 else (128 if num_edges >= (1 << 20) else 64)
COLSUM_BLOCKS = 1024      # scratch blocks of ampconv_masked_colsum (csrc/node_ops.hip)


class View(ctypes.Structure):
    """ampconv_view_t: element (n, l, h, c) at ptr + n*node + l*row + h*head + c."""
    _fields_ = [('ptr', ctypes.c_void_p), ('node_stride', ctypes.c_int64),
                ('row_stride', ctypes.c_int64), ('head_stride', ctypes.c_int64)]


def ptr(t):
    """Device address of a tensor for a void * argument; None (an optional argument left out) -> NULL."""
    return t.data_ptr() if t is not None else None


_vp, _i64, _i32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t


class WeightImage(ctypes.Structure):
    """ampconv_weight_image_t: one job of ampconv_proj_weight_images."""
    _fields_ = [('W', ctypes.c_void_p), ('stride_n', ctypes.c_int64), ('stride_k', ctypes.c_int64),
                ('N', ctypes.c_int), ('K', ctypes.c_int), ('image', ctypes.c_void_p)]


class AdamTensor(ctypes.Structure):
    """ampconv_adam_tensor_t: one tensor of ampconv_adam_step / ampconv_adam_grad_norm (a HOST array of these)."""
    _fields_ = [('p', ctypes.c_void_p), ('g', ctypes.c_void_p), ('m', ctypes.c_void_p), ('v', ctypes.c_void_p),
                ('numel', ctypes.c_int64), ('step_size', ctypes.c_float), ('inv_bc2_sqrt', ctypes.c_float)]


class AdamMixedTensor(ctypes.Structure):
    """ampconv_adam_mixed_tensor_t: one tensor of ampconv_adam_mixed_step / ampconv_adam_mixed_grad_norm (64 bytes)."""
    _fields_ = [('p', ctypes.c_void_p), ('g', ctypes.c_void_p), ('m', ctypes.c_void_p), ('v', ctypes.c_void_p),
                ('master', ctypes.c_void_p), ('numel', ctypes.c_int64), ('step_size', ctypes.c_float),
                ('inv_bc2_sqrt', ctypes.c_float), ('p_dtype', ctypes.c_int32), ('g_dtype', ctypes.c_int32)]


ADAM_MAX_TENSORS = 24     # AMPCONV_ADAM_MAX_TENSORS: descriptors per launch
ADAM_CHUNK = 1024         # AMPCONV_ADAM_CHUNK: elements per workgroup


class StatsTensor(ctypes.Structure):
    """ampconv_stats_tensor_t: one tensor of the ampconv_stats_* calls (a HOST array of these)."""
    _fields_ = [('x', ctypes.c_void_p), ('numel', ctypes.c_int64), ('dtype', ctypes.c_int)]


STATS_MAX_TENSORS = 24    # AMPCONV_STATS_MAX_TENSORS: descriptors per launch
STATS_CHUNK = 4096        # AMPCONV_STATS_CHUNK: elements one workgroup handles per iteration
STATS_MAX_BINS = 2048     # AMPCONV_STATS_MAX_BINS
STATS_MAX_RANKS = 4       # AMPCONV_STATS_MAX_RANKS: order statistics per call
STATS_RECORD_BYTES = 88   # sizeof(ampconv_stats_record_t)
PCA_RUN, PCA_MAX_W, PCA_MAX_K = 32, 2048, 128    # AMPCONV_PCA_RUN (rows summed in fp32 before the fp64 fold), _MAX_W, _MAX_K
TSNE_MAX_K, TSNE_MAX_N, TSNE_RUN, TSNE_TILE, TSNE_CHUNK, TSNE_PART = 256, 1 << 24, 256, 1024, 4096, 1024    # AMPCONV_TSNE_*
UMAP_MAX_K, UMAP_MAX_M, UMAP_MAX_DIM, UMAP_PART = 256, 1 << 24, 32, 1024      # AMPCONV_UMAP_*
SBM_MAX_K = 256          # AMPCONV_SBM_MAX_K: blocks of a stochastic block model
SPRING_MAX_N, SPRING_RUN, SPRING_TILE, SPRING_CHUNK, SPRING_PART = 1 << 24, 256, 1024, 4096, 1024      # AMPCONV_SPRING_*
GCN_LONG_SEGMENT = 256   # AMPCONV_GCN_LONG_SEGMENT: a CSR/CSC segment from this length on is summed by whole workgroups
GCN_PART = 2048          # AMPCONV_GCN_PART: entries of a long segment that one workgroup sums

# name -> (restype, argtypes); mirrors include/ampconv.h one to one
SIGNATURES = {
    'ampconv_version': (_i32, []),
    'ampconv_error_string': (ctypes.c_char_p, [_i32]),
    'ampconv_csr_workspace_bytes': (_sz, [_i64, _i64]),
    'ampconv_csr_build': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_graph_build': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_csc_positions_from': (_i32, [_vp, _vp, _i64, _vp, _vp]),
    'ampconv_hub_plan_bytes': (_sz, [_i64, _i32]),
    'ampconv_hub_plan': (_i32, [_vp, _i64, _i64, _i32, _vp, _vp]),
    'ampconv_hub_workspace_bytes': (_sz, [_i64, _i32, _i32, _i32]),
    'ampconv_fwd_edge': (_i32, [View, View, View, _vp, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp, _i32, _vp]),
    'ampconv_csc_positions': (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    'ampconv_softmax_stats_bytes': (_sz, [_i64, _i32, _i32, _i32, _i32]),
    'ampconv_bwd_edge_dst': (_i32, [View, View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp,
                                    _vp, _vp, _vp, _i32, _vp]),
    'ampconv_bwd_edge_src': (_i32, [View, View, View, View, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                    View, View, _vp, _i64, _vp, _vp, _vp, _i32, _vp]),
    'ampconv_edge_family': (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, ctypes.POINTER(View), _i32]),
    'ampconv_attn_weights': (_i32, [View, View, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_attn_scores': (_i32, [View, View, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_attn_heatmap': (_i32, [View, View, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64,
                                    _i32, _vp]),
    'ampconv_attn_heatmap_shift': (_i32, []),
    'ampconv_gather_segment_sum': (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _i64, _vp, _vp]),
    'ampconv_linear_outer': (_i32, [View, View, _i64, _i32, _i32, _i32, ctypes.c_float, _vp, _vp]),
    'ampconv_linear_apply': (_i32, [View, _vp, _i32, _i64, _i32, _i32, _i32, ctypes.c_float, View, _vp]),
    'ampconv_saint_random_walk': (_i32, [_vp, _vp, _vp, _i64, _i32, ctypes.c_uint64, _vp, _vp]),
    'ampconv_saint_workspace_bytes': (_sz, [_i64]),
    'ampconv_saint_nodes': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_saint_count_edges': (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_saint_count_edges_bounded': (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_saint_fill_edges': (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'ampconv_saint_add_counts': (_i32, [_vp, _i64, _vp, _vp]),
    'ampconv_saint_norms': (_i32, [_vp, _vp, _vp, _i64, _i64, ctypes.c_float, _vp, _vp, _vp]),
    'ampconv_saint_gather_rows': (_i32, [_vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    'ampconv_feat_zscore_stats': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp]),
    'ampconv_feat_sample_present': (_i32, [_vp, _i64, _i32, _i32, ctypes.c_uint64, _vp, _vp, _vp]),
    'ampconv_feat_build': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    'ampconv_feat_table_grad': (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    'ampconv_feat_build_as': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_feat_table_grad_from': (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_proj_supported': (_i32, [_i32, _i32, _i32]),
    'ampconv_proj_weight_image_bytes': (_sz, [_i32, _i32, _i32]),
    'ampconv_proj_weight_image': (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_proj_weight_images': (_i32, [_i32, _vp, _i32, _vp]),
    'ampconv_proj_rows': (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _vp]),
    'ampconv_proj_wgrad_workspace_bytes': (_sz, [_i64, _i32, _i32, _i32]),
    'ampconv_proj_wgrad': (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp, _i64, _vp, _vp, _i32, _vp]),
    'ampconv_absmax': (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_planes_supported': (_i32, [_i32, _i32, _i32]),
    'ampconv_fwd_edge_planes': (_i32, [View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp, _vp, _vp]),
    'ampconv_bwd_edge_dst_planes': (_i32, [View, View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp,
                                           _vp, _vp, _vp, _vp, _vp]),
    'ampconv_bwd_edge_src_planes': (_i32, [View, View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, View, _vp, _i64,
                                           _vp, _vp, _vp, _vp, _vp]),
    'ampconv_scaled_supported': (_i32, [_i32, _i32, _i32]),
    'ampconv_fwd_edge_scaled': (_i32, [View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp, _vp, _vp]),
    'ampconv_bwd_edge_dst_scaled': (_i32, [View, View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp,
                                           _vp, _vp, _vp, _vp, _vp]),
    'ampconv_bwd_edge_src_scaled': (_i32, [View, View, View, View, _vp, _vp, _vp, _i64, _i32, _i32, _i32, View, View, _vp,
                                           _i64, _vp, _vp, _vp, _vp, _vp]),
    'ampconv_token_supported': (_i32, [_i32, _i32, _i32, _i32]),
    'ampconv_fwd_edge_token': (_i32, [View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp, _i32, _vp]),
    'ampconv_bwd_edge_dst_token': (_i32, [View, View, View, View, _vp, _vp, _i64, _i32, _i32, _i32, View, _vp, _i64, _vp,
                                          _i32, _vp]),
    'ampconv_bwd_edge_src_token': (_i32, [View, View, View, View, _vp, _vp, _vp, _i64, _i32, _i32, _i32, View, View, _vp,
                                          _i64, _vp, _i32, _vp]),
    'ampconv_proj_out_bound': (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    'ampconv_proj_rows_planes': (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp,
                                        _i32, _i32, _vp]),
    'ampconv_planes_to_f32': (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _vp]),
    'ampconv_absmax_stats': (_i32, [_vp, _i64, _i64, _i32, _vp, _vp]),
    'ampconv_active_nodes_workspace_bytes': (_sz, [_i64]),
    'ampconv_active_nodes': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_segment_mean': (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    'ampconv_mask_rows': (_i32, [_vp, _vp, _i64, _i64, _i32, _vp]),
    'ampconv_masked_colsum': (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_act_dropout_fwd': (_i32, [_vp, _i64, _i32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, _vp, _i32, _vp]),
    'ampconv_act_dropout_bwd': (_i32, [_vp, _vp, _i64, _i32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, _vp, _i32, _vp]),
    'ampconv_pool_fwd': (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, _vp, _i32,
                                _vp]),
    'ampconv_pool_bwd': (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float, _vp,
                                _i32, _vp]),
    'ampconv_head_workspace_bytes': (_sz, [_i64, _i32, _i32]),
    'ampconv_head_fwd': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    'ampconv_head_bwd': (_i32, [_vp, _i64, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_head_nll_fwd': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                                    _i32, _vp]),
    'ampconv_head_nll_bwd': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                                    _vp, _sz, _i32, _vp]),
    'ampconv_norm_workspace_bytes': (_sz, [_i64, _i32]),
    'ampconv_norm_fwd': (_i32, [_vp, _i64, _i32, _vp, _vp, ctypes.c_float, _i32, ctypes.c_uint64, ctypes.c_uint32,
                                ctypes.c_float, _vp, _vp, _i32, _vp]),
    'ampconv_norm_bwd': (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_float,
                                _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_norm_pool_fwd': (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, ctypes.c_float, _i32, _i32, ctypes.c_uint64,
                                     ctypes.c_uint32, ctypes.c_float, _vp, _vp, _i32, _vp]),
    'ampconv_norm_pool_bwd': (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _i32, ctypes.c_uint64, ctypes.c_uint32,
                                     ctypes.c_float, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_adam_workspace_bytes': (_sz, [ctypes.POINTER(AdamTensor), _i32]),
    'ampconv_adam_grad_norm': (_i32, [ctypes.POINTER(AdamTensor), _i32, ctypes.c_float, _vp, _vp, _sz, _vp]),
    'ampconv_adam_step': (_i32, [ctypes.POINTER(AdamTensor), _i32, ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                 ctypes.c_float, ctypes.c_float, _i32, ctypes.c_float, _vp, ctypes.c_float, _vp]),
    'ampconv_adam_mixed_workspace_bytes': (_sz, [ctypes.POINTER(AdamMixedTensor), _i32]),
    'ampconv_adam_mixed_grad_norm': (_i32, [ctypes.POINTER(AdamMixedTensor), _i32, ctypes.c_float, _vp, _vp, _sz, _vp]),
    'ampconv_adam_mixed_step': (_i32, [ctypes.POINTER(AdamMixedTensor), _i32, ctypes.c_float, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_float, ctypes.c_float, _i32, ctypes.c_float, _vp, ctypes.c_float, _vp]),
    'ampconv_stats_workspace_bytes': (_sz, [ctypes.POINTER(StatsTensor), _i32]),
    'ampconv_stats_moments': (_i32, [ctypes.POINTER(StatsTensor), _i32, _vp, _vp, _sz, _vp]),
    'ampconv_stats_histogram': (_i32, [ctypes.POINTER(StatsTensor), _i32, _i32, _vp, _vp, _vp, _vp]),
    'ampconv_stats_select': (_i32, [ctypes.POINTER(StatsTensor), _i32, ctypes.POINTER(ctypes.c_double), _i32, _vp, _vp,
                                    _vp, _sz, _vp]),
    'ampconv_gcn_norm': (_i32, [_vp, _vp, _i64, _i32, ctypes.c_float, _vp, _vp]),
    'ampconv_gcn_aggregate_workspace_bytes': (_sz, [_i64, _i64, _i32]),
    'ampconv_gcn_aggregate': (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _i32, ctypes.c_float, _vp, _vp, _i64, _i64, _i64, _vp,
                                     _sz, _vp]),
    'ampconv_gcn_colsum_workspace_bytes': (_sz, [_i64, _i32]),
    'ampconv_gcn_colsum': (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _sz, _vp]),
    'ampconv_gcn_input_workspace_bytes': (_sz, [_i64, _i64, _i32]),
    'ampconv_gcn_input_fwd': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _sz, _vp]),
    'ampconv_gcn_input_bwd': (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_pair_loss_workspace_bytes': (_sz, [_i64, _i64, _i32]),
    'ampconv_pair_loss_fwd': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i32, ctypes.c_float,
                                     ctypes.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_pair_loss_bwd': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i32, ctypes.c_float,
                                     ctypes.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _sz, _i32, _vp]),
    'ampconv_knn_workspace_bytes': (_sz, [_i64, _i64, _i64, _i32, _i32]),
    'ampconv_knn': (_i32, [_vp, _i64, _i32, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_pca_shift_workspace_bytes': (_sz, [_i64, _i32, _i32]),
    'ampconv_pca_shift': (_i32, [_vp, _i64, _i32, _i64, _i32, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_pca_gram_splits': (_i32, [_i64, _i32]),
    'ampconv_pca_gram_workspace_bytes': (_sz, [_i64, _i32]),
    'ampconv_pca_gram': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_pca_project': (_i32, [_vp, _i64, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i32, _vp]),
    'ampconv_tsne_affinities': (_i32, [_vp, _i64, _i32, _i64, ctypes.c_float, _vp, _vp, _vp]),
    'ampconv_tsne_repulsion_workspace_bytes': (_sz, [_i64]),
    'ampconv_tsne_repulsion': (_i32, [_vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_tsne_step_workspace_bytes': (_sz, [_i64, _i64]),
    'ampconv_tsne_step': (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, ctypes.c_float, ctypes.c_float,
                                 ctypes.c_float, ctypes.c_float, _vp, _vp, _sz, _vp]),
    'ampconv_umap_memberships_workspace_bytes': (_sz, [_i64]),
    'ampconv_umap_memberships': (_i32, [_vp, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_umap_coefficients': (_i32, [_vp, _i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp]),
    'ampconv_umap_epoch_workspace_bytes': (_sz, [_i64, _i64, _i32]),
    'ampconv_umap_epoch': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.c_float, ctypes.c_float,
                                  ctypes.c_float, ctypes.c_float, _i32, ctypes.c_uint64, _vp, _sz, _vp]),
    'ampconv_umap_epoch_split': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _vp, ctypes.c_float,
                                        ctypes.c_float, ctypes.c_float, ctypes.c_float, _i32, ctypes.c_uint64, _i32, _vp, _sz,
                                        _vp]),
    'ampconv_spring_start': (_i32, [_vp, _i64, _i32, ctypes.c_uint64, _vp]),
    'ampconv_spring_repulsion_workspace_bytes': (_sz, [_i64, _i32]),
    'ampconv_spring_repulsion': (_i32, [_vp, _i64, _i32, _vp, _vp, _vp, _sz, _vp]),
    'ampconv_spring_step_workspace_bytes': (_sz, [_i64, _i64, _i32]),
    'ampconv_spring_step': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp,
                                   _vp, _sz, _vp]),
    'ampconv_spring_step_split': (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                         _vp, _i32, _vp, _sz, _vp]),
    'ampconv_sbm_count': (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, ctypes.c_uint64, _vp, _vp, _vp]),
    'ampconv_sbm_fill': (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, ctypes.c_uint64, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    'ampconv_mfm_workspace_bytes': (_sz, [_i64, _i32, _i32]),
    'ampconv_mfm_build': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, ctypes.c_uint64, ctypes.c_uint32, _i32,
                                 _vp, _vp, _vp, _vp, _i32, _vp]),
    'ampconv_mfm_token_grad': (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _sz, _i32, _vp]),
    'ampconv_mfm_loss_fwd': (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    'ampconv_mfm_loss_bwd': (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _i32, _vp]),
}

_lib = None


class AmpconvError(RuntimeError):
    pass


def load():
    """Load libampconv.so once; raise (never fall back) if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmpconvError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950). ampnet_amd has no non-HIP fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)           # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    got = lib.ampconv_version()
    if got != EXPECTED_ABI:
        # argument lists differ between ABI versions (101 inserted the statistics pointers): a stale
        # or foreign build would reinterpret pointers as dtype / stream arguments
        raise AmpconvError(f'{LIB_PATH} has ABI version {got}, this binding needs {EXPECTED_ABI}: rebuild it '
                           '(python -c "import __graft_entry__ as g; g.build(force=True)")')
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().ampconv_error_string(rc)
        raise AmpconvError(f'{what} failed: {msg.decode() if msg else rc} (code {rc})')
