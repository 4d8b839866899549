from .amp_conv import AMPConv, InvalidConfiguration, MessagePassing
from .gcn_conv import GCNConv

__all__ = ['AMPConv', 'InvalidConfiguration', 'MessagePassing', 'GCNConv']
