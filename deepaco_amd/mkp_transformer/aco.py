"""ACO with the class surface of the reference's mkp_transformer/aco.py (`from aco import ACO`), on MI355X.
The implementation lives in deepaco_amd/mkp_vec.py (class ACO)."""
import os
import sys

try:
    from deepaco_amd.mkp_vec import ACO  # noqa: F401
except ImportError:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    from deepaco_amd.mkp_vec import ACO  # noqa: F401
