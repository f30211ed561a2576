"""Drop-in import path of the reference (`from bayesian_inference.estimate_MAP import ...`): thin re-exports of
bayesianinferencedl_amd.bayesian_inference.estimate_MAP (repo root on sys.path)."""
from bayesianinferencedl_amd.bayesian_inference.estimate_MAP import (  # noqa: F401
    MLSolverWrapper, ROMMLSolverWrapper, RSolverWrapper, SolverWrapper, estimate_map, objective, starting_points)
