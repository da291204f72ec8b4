"""MI355X-native batched Tetris-piclim environment (Tetris with a prescribed initial configuration, L lines
to clear, at most M moves on a 20x10 board).

The package holds only what the hot path needs: `csrc/` (hand-written HIP kernels for gfx950 + the C ABI of
include/tetris_piclim.h) and `env.py`, the host-side mirror of the reference's `Tetris` interface.
The directory name is not a Python identifier; import it as `import tetris_piclim` (alias module at the repo
root) or with importlib.import_module.
"""
from . import _lib
from ._lib import (LIB_PATH, SYMBOLS, TplError, build_library, carve, forward_generate, generate_configs, pack_policy,
                   shape_info)

__all__ = ["BatchedTetris", "Tetris", "Snapshot", "OBS_DIM", "NUM_ACTIONS", "RUNNING", "WON", "LOST", "TplError",
           "RandomPieceGenerator", "get_tetromino", "piece_translations", "translate", "carve", "build_library", "shape_info", "generate_configs", "forward_generate", "pack_policy", "LIB_PATH", "SYMBOLS", "DQNLearner",
           "ReplayRing", "PrioritizedReplayRing", "LookaheadPolicy", "afterstates", "HeuristicPolicy", "placement_features",
           "evaluate_heuristic", "tune_heuristic", "BeamPolicy", "NTuplePolicy", "NTupleBeamPolicy", "NTupleLearner", "ntuple_table", "ntuple_value",
           "ntuple_is_symmetric", "ntuple_coherence", "ntuple_step_sizes", "ntuple_shape", "NTUPLE_SHAPES", "ntuple_parts", "NTUPLE_SUMS", "NTUPLE_ENTRIES_SUM",
           "NTUPLE_STAGES", "ntuple_stage_map", "ntuple_staged", "ntuple_stages", "ntuple_map", "ntuple_is_staged", "NTUPLE_FEATURE_FORMS",
           "ntuple_feature_bins", "NTUPLE_BUDGET_FORMS", "ntuple_budget", "ntuple_budget_bins", "solve_configs", "prove_configs", "ntuple_prove_configs", "tighten_pool", "CLASSICAL_WEIGHTS", "FEATURE_NAMES",
           "MOVE_FEATURE_NAMES", "DELLACHERIE_WEIGHTS", "move_bound", "config_bound", "config_index", "PoolTally", "resample_pool",
           "curriculum_weights", "PoolCurriculum", "prove_nodes", "label_moves", "label_states", "blunders",
           "NTupleRanker", "LabelSet", "collect_labels", "label_agreement", "window_prove", "ProofPolicy",
           "ntuple_window_prove", "TableProofPolicy", "prove_configs_limited", "ntuple_prove_configs_limited",
           "window_prove_limited", "ntuple_window_prove_limited", "LimitedProofPolicy"]


def __getattr__(name):
    # env.py needs torch; keep `import tetris_piclim` cheap for callers that only build or bind the library
    import importlib
    if name in ("BatchedTetris", "Tetris", "Snapshot", "OBS_DIM", "NUM_ACTIONS", "RUNNING", "WON", "LOST", "env"):
        env = importlib.import_module(__name__ + ".env")
        return env if name == "env" else getattr(env, name)
    if name in ("save_pool", "load_pool", "PoolRefresher", "ForwardGames", "blend"):
        return getattr(importlib.import_module(__name__ + ".pool"), name)
    if name in ("sharding", "actor", "pool"):
        return importlib.import_module(__name__ + "." + name)
    if name in ("RandomPieceGenerator", "get_tetromino", "piece_translations", "translate"):
        return getattr(importlib.import_module(__name__ + ".pieces"), name)
    if name in ("Actor", "PolicyMLP"):
        return getattr(importlib.import_module(__name__ + ".actor"), name)
    if name in ("DQNLearner", "ReplayRing", "PrioritizedReplayRing"):
        # the learner library (libtpl_learn.so) is built and loaded only here, on first use
        return getattr(importlib.import_module(__name__ + ".learn"), name)
    if name in ("LookaheadPolicy", "afterstates"):
        return getattr(importlib.import_module(__name__ + ".lookahead"), name)
    if name in ("HeuristicPolicy", "placement_features", "evaluate_heuristic", "tune_heuristic", "BeamPolicy", "FEATURE_NAMES",
                "MOVE_FEATURE_NAMES", "DELLACHERIE_WEIGHTS", "move_bound"):
        return getattr(importlib.import_module(__name__ + ".heuristic"), name)
    if name in ("NTuplePolicy", "NTupleBeamPolicy", "NTupleLearner", "ntuple_table", "ntuple_value", "ntuple_is_symmetric", "ntuple_coherence",
                "ntuple_step_sizes", "ntuple_shape", "NTUPLE_SHAPES", "ntuple_parts", "NTUPLE_SUMS", "NTUPLE_ENTRIES_SUM",
                "NTUPLE_STAGES", "ntuple_stage_map", "ntuple_staged", "ntuple_stages", "ntuple_map", "ntuple_is_staged", "NTUPLE_FEATURE_FORMS",
                "ntuple_feature_bins", "NTUPLE_BUDGET_FORMS", "ntuple_budget", "ntuple_budget_bins", "NTupleRanker"):
        return getattr(importlib.import_module(__name__ + ".ntuple"), name)
    if name in ("solve_configs", "prove_configs", "ntuple_prove_configs", "tighten_pool", "CLASSICAL_WEIGHTS", "config_bound", "prove_nodes",
                "label_moves", "label_states", "blunders", "LabelSet", "collect_labels", "label_agreement", "window_prove", "ProofPolicy",
                "ntuple_window_prove", "TableProofPolicy", "prove_configs_limited", "ntuple_prove_configs_limited",
                "window_prove_limited", "ntuple_window_prove_limited", "LimitedProofPolicy"):
        return getattr(importlib.import_module(__name__ + ".solve"), name)
    if name in ("config_index", "PoolTally", "resample_pool", "curriculum_weights", "PoolCurriculum"):
        return getattr(importlib.import_module(__name__ + ".curriculum"), name)
    if name in ("learn", "_learn_lib", "lookahead", "heuristic", "ntuple", "solve", "curriculum"):
        return importlib.import_module(__name__ + "." + name)
    raise AttributeError(name)
