from .amp_gcn import AMPGCN, FeatureTokens
from .gcn import GCN

__all__ = ['AMPGCN', 'FeatureTokens', 'GCN']
