from .amp_gcn import AMPGCN
from .feature_tokens import FeatureTokens
from .gcn import GCN

__all__ = ['AMPGCN', 'FeatureTokens', 'GCN']
