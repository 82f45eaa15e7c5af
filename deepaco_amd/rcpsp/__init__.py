"""Drop-in counterpart of the reference's rcpsp/ directory (aco.py, rcpsp_inst.py); its heuristic network is not covered."""
