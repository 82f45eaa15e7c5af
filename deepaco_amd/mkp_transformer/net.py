"""Net of mkp_transformer/net.py (`from net import TransformerModel`): implemented in deepaco_amd/transformer.py."""
import os
import sys

try:
    from deepaco_amd.transformer import TransformerModel, MLP, ParNet  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from deepaco_amd.transformer import TransformerModel, MLP, ParNet  # noqa: F401
