"""Drop-in counterpart of the reference's mkp_transformer/ directory (aco.py, utils.py)."""
