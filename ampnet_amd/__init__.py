"""ampnet_amd -- MI355X-native AMPConv (the hot path of HarryL-Git/ampnet).

    from ampnet_amd import AMPConv          # drop-in for src.ampnet.conv.AMPConv

Host side: Python on PyTorch-ROCm (device memory, streams, torch.distributed).
Compute: libampconv.so, hand-written HIP for gfx950 behind the C ABI of
include/ampconv.h.  No CPU fallback.
"""
from .conv import AMPConv, GCNConv, InvalidConfiguration
from .graph import EdgeCSR, graph_cache
from . import distributed
from .module import AMPGCN, GCN, FeatureTokens
from .sampler import GraphSAINTRandomWalkSampler
from .partitioned import NodePartition, PartitionedAMPConv
from .graphed import GraphedAMPConv
from .heatmap import AttentionHeatmap, top_features
from .glue import ActDropout, TokenReadout, act_dropout, act_dropout_pool
from .head import HeadMetrics, classifier_head, saint_nll_loss
from .masked import MaskedMetrics, MaskedValueHead, build_masked_tokens, masked_value_loss
from .norm import NormTokenReadout, TokenLayerNorm, norm_act_dropout, norm_act_dropout_pool
from .optim import FusedAdam
from .stats import TensorStats, tensor_stats
from .gcn import gcn_aggregate, gcn_input_linear, gcn_norm
from .pair_loss import PairLoss, pair_loss, walk_pairs
from .knn import knn, knn_classify, knn_graph
from .pca import PCAResult, pca
from .tsne import TSNEResult, neighbor_preservation, tsne
from .umap import UMAPResult, umap
from .spring import SpringLayout, SpringResult, spring_layout
from .random_graphs import (BlockModelGraph, XorLinkData, gnp_random_graph, random_partition_graph, stochastic_block_model,
                            xor_link_dataset)

__all__ = ['AMPConv', 'InvalidConfiguration', 'EdgeCSR', 'graph_cache', 'distributed', 'AMPGCN', 'FeatureTokens',
           'GraphSAINTRandomWalkSampler', 'NodePartition', 'PartitionedAMPConv', 'GraphedAMPConv', 'AttentionHeatmap', 'top_features',
           'ActDropout', 'TokenReadout', 'act_dropout', 'act_dropout_pool', 'HeadMetrics', 'classifier_head', 'saint_nll_loss',
           'NormTokenReadout', 'TokenLayerNorm', 'norm_act_dropout', 'norm_act_dropout_pool', 'FusedAdam',
           'TensorStats', 'tensor_stats', 'GCNConv', 'GCN', 'gcn_norm', 'gcn_aggregate', 'gcn_input_linear',
           'pair_loss', 'PairLoss', 'walk_pairs', 'knn', 'knn_graph', 'knn_classify', 'pca', 'PCAResult',
           'tsne', 'TSNEResult', 'neighbor_preservation', 'umap', 'UMAPResult',
           'spring_layout', 'SpringResult', 'SpringLayout',
           'stochastic_block_model', 'random_partition_graph', 'gnp_random_graph', 'xor_link_dataset', 'BlockModelGraph',
           'XorLinkData', 'masked_value_loss', 'MaskedValueHead', 'MaskedMetrics', 'build_masked_tokens']
