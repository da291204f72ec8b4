"""Build and bind the learner's C-ABI library (include/tpl_learn.h) with ctypes: the packed replay ring and the device-side
policy packers (csrc/learn/), and the numpy mirrors of their rules that the tests check the kernels against.

A library of its own (<repo>/lib/libtpl_learn.so), so that the environment library and its measured sources stay as they
are: it includes the environment's device headers read-only and links nothing of libtetris_piclim.so.  Built, stamped and
locked as _lib.build_library builds the environment library; its digest covers its units and every header they include.
Nothing here is loaded by `import tetris_piclim` or by any environment entry point.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np

from . import _lib
from ._lib import TplError, _hipcc

_LEARN_CSRC = os.path.join(_lib._CSRC, "learn")
LEARN_LIB_PATH = os.path.join(_lib._LIBDIR, "libtpl_learn.so")
_UNITS = [os.path.join(_LEARN_CSRC, f) for f in ("replay.hip", "pack.hip", "priority.hip", "afterstates.hip",
                                                      "beam.hip", "solve.hip", "ntuple.hip", "ntuple_beam.hip", "heuristic_move.hip",
                                                      "beam_move.hip", "solve_move.hip", "bound.hip", "beam_bound.hip",
                                                      "solve_bound.hip", "beam_move_bound.hip", "solve_move_bound.hip",
                                                      "exact.hip", "exact_move.hip", "ntuple_exact.hip", "curriculum.hip", "exact_nodes.hip",
                                                      "exact_nodes_move.hip", "exact_window.hip", "exact_window_move.hip",
                                                      "ntuple_window.hip", "ntuple_rank.hip", "exact_limited.hip", "exact_limited_move.hip",
                                                      "exact_window_limited.hip", "exact_window_limited_move.hip",
                                                      "ntuple_exact_limited.hip", "ntuple_window_limited.hip", "heuristic.hip")]

# entry points declared in include/tpl_learn.h (tests check that the .so exports every one of them)
LEARN_SYMBOLS = [
    "tpl_learn_last_error", "tpl_replay_record_bytes", "tpl_replay_push", "tpl_replay_sample", "tpl_replay_index",
    "tpl_learn_image_bytes", "tpl_learn_pack", "tpl_priority_tree_bytes", "tpl_priority_init", "tpl_priority_push",
    "tpl_priority_update", "tpl_replay_sample_prioritized", "tpl_priority_target", "tpl_replay_sample_nstep",
    "tpl_replay_sample_mirror", "tpl_mirror_states", "tpl_afterstates", "tpl_canonical_action", "tpl_placement_features",
    "tpl_placement_act", "tpl_placement_search", "tpl_placement_beam", "tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_update",
    "tpl_ntuple_search", "tpl_ntuple_update_trace", "tpl_ntuple_update_coherent", "tpl_ntuple_entries",
    "tpl_ntuple_value_shaped", "tpl_ntuple_act_shaped", "tpl_ntuple_search_shaped", "tpl_ntuple_update_shaped",
    "tpl_ntuple_update_trace_shaped", "tpl_ntuple_update_coherent_shaped", "tpl_ntuple_beam",
    "tpl_ntuple_value_sum", "tpl_ntuple_act_sum", "tpl_ntuple_search_sum", "tpl_ntuple_beam_sum",
    "tpl_ntuple_value_staged", "tpl_ntuple_act_staged", "tpl_ntuple_search_staged", "tpl_ntuple_beam_staged",
    "tpl_ntuple_update_trace_staged",
    "tpl_ntuple_value_feature", "tpl_ntuple_act_feature", "tpl_ntuple_search_feature", "tpl_ntuple_beam_feature",
    "tpl_ntuple_update_trace_feature", "tpl_ntuple_feature_bins", "tpl_placement_solve",
    "tpl_placement_features_move", "tpl_placement_act_move", "tpl_placement_search_move", "tpl_placement_beam_move",
    "tpl_placement_solve_move",
    "tpl_move_bound", "tpl_move_bound_rows", "tpl_placement_solve_bound", "tpl_placement_solve_move_bound",
    "tpl_placement_beam_bound", "tpl_placement_beam_move_bound",
    "tpl_ntuple_value_budget", "tpl_ntuple_act_budget", "tpl_ntuple_search_budget", "tpl_ntuple_beam_budget",
    "tpl_ntuple_update_trace_budget", "tpl_ntuple_budget_bins",
    "tpl_placement_exact", "tpl_placement_exact_move", "tpl_ntuple_exact",
    "tpl_config_index", "tpl_pool_tally", "tpl_pool_resample",
    "tpl_placement_exact_nodes", "tpl_placement_exact_nodes_move", "tpl_placement_exact_labels", "tpl_placement_exact_labels_move",
    "tpl_ntuple_rank",
    "tpl_placement_window_prove", "tpl_placement_window_prove_move", "tpl_ntuple_window_prove",
    "tpl_placement_exact_limited", "tpl_placement_exact_limited_move", "tpl_placement_window_prove_limited",
    "tpl_placement_window_prove_limited_move", "tpl_ntuple_exact_limited", "tpl_ntuple_window_prove_limited",
]
NSTEP_MAX = 16
BEAM_MAX_DEPTH, BEAM_MAX_WIDTH = 12, 64
NTUPLE_BEAM_MAX_DEPTH = 11                               # one less: the leaf's piece must be a known one
MIRROR_MODES = {False: 0, True: 1, "always": 2}          # sample(mirror=...) -> tpl_mirror_mode

IMAGE_KINDS = {"bf16": 0, "f32": 1, "split": 2}
RECORD_BYTES = 80


def _sources() -> list:
    """The units and, transitively, every quoted #include of theirs (the environment headers among them)."""
    seen, todo = [], list(_UNITS)
    while todo:
        path = os.path.normpath(todo.pop(0))
        if path in seen:
            continue
        seen.append(path)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M):
            todo.append(os.path.join(os.path.dirname(path), inc))
    return sorted(seen)


def _source_digest() -> str:
    import hashlib
    h = hashlib.sha256()
    for path in _sources():
        with open(path, "rb") as f:
            h.update(os.path.relpath(path, _lib._ROOT).encode() + b"\0" + f.read())
    return h.hexdigest()


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> <repo>/lib/libtpl_learn.so; stale by digest, concurrent builders serialise on a lock."""
    stamp = LEARN_LIB_PATH + ".sha256"
    digest = _source_digest()

    def fresh():
        return os.path.exists(LEARN_LIB_PATH) and os.path.exists(stamp) and open(stamp).read().strip() == digest

    if not force and fresh():
        return LEARN_LIB_PATH
    import fcntl
    os.makedirs(_lib._LIBDIR, exist_ok=True)
    with open(LEARN_LIB_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or not fresh():
                tmp = f"{LEARN_LIB_PATH}.{os.getpid()}.tmp"
                cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-o", tmp] + _UNITS
                res = subprocess.run(cmd, capture_output=True, text=True)
                if res.returncode != 0:
                    raise RuntimeError("hipcc failed:\n" + res.stdout + res.stderr)
                os.replace(tmp, LEARN_LIB_PATH)
                with open(stamp + ".tmp", "w") as f:
                    f.write(digest)
                os.replace(stamp + ".tmp", stamp)
                if verbose:
                    print("built", LEARN_LIB_PATH)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LEARN_LIB_PATH


_handle = None


def lib() -> C.CDLL:
    global _handle
    if _handle is not None:
        return _handle
    import torch  # noqa: F401  -- torch's HIP runtime first (_lib.lib() says why)
    L = C.CDLL(build_library())
    vp, i32, i64, u64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t
    L.tpl_learn_last_error.restype = C.c_char_p
    L.tpl_learn_last_error.argtypes = []
    L.tpl_replay_record_bytes.restype = sz
    L.tpl_replay_record_bytes.argtypes = []
    L.tpl_replay_push.argtypes = [vp, i64, i64, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_replay_sample.argtypes = [vp, i64, i64, i64, u64, u64, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_replay_index.restype = i64
    L.tpl_replay_index.argtypes = [u64, u64, i64, i64]
    L.tpl_learn_image_bytes.restype = sz
    L.tpl_learn_image_bytes.argtypes = [i32]
    L.tpl_learn_pack.argtypes = [i32] + [vp] * 12
    f64 = C.c_double
    L.tpl_priority_tree_bytes.restype = sz
    L.tpl_priority_tree_bytes.argtypes = [i64]
    L.tpl_priority_init.argtypes = [vp, i64, vp]
    L.tpl_priority_push.argtypes = [vp, i64, i64, i64, vp]
    L.tpl_priority_update.argtypes = [vp, i64, i64, vp, vp, vp]
    L.tpl_replay_sample_prioritized.argtypes = [vp, vp, i64, i64, i64, u64, u64, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp,
                                                vp]
    L.tpl_priority_target.restype = f64
    L.tpl_priority_target.argtypes = [u64, u64, i64, i64, f64]
    L.tpl_replay_sample_nstep.argtypes = [vp, vp, i64, i64, i64, i64, i32, C.c_float, i64, u64, u64, i32, i32, vp, i32, vp, vp,
                                          vp, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_replay_sample_mirror.argtypes = L.tpl_replay_sample_nstep.argtypes[:-1] + [i32, vp, vp]
    L.tpl_mirror_states.argtypes = [i64, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_afterstates.argtypes = [vp, vp, i64, i32, i32, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_canonical_action.restype = i32
    L.tpl_canonical_action.argtypes = [i32, i32]
    L.tpl_placement_features.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp]
    L.tpl_placement_act.argtypes = [vp, vp, i64, i32, i32, vp, i64, vp, vp, vp]
    L.tpl_placement_search.argtypes = [vp, vp, i64, i32, i32, vp, i64, vp, vp, vp, vp]
    L.tpl_placement_beam.argtypes = [vp, vp, i64, i32, i32, vp, i64, i32, i32, vp, vp, vp, vp]
    L.tpl_placement_solve.argtypes = [vp, vp, i64, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    L.tpl_placement_solve.restype = i32
    for name in ("features", "act", "search", "beam", "solve"):      # the 14-feature form: the twin's arguments
        twin = getattr(L, f"tpl_placement_{name}_move")
        twin.argtypes = getattr(L, f"tpl_placement_{name}").argtypes
        twin.restype = i32
    f32 = C.c_float
    L.tpl_move_bound.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp]
    L.tpl_move_bound_rows.argtypes = [vp, i64, i32, vp, vp]
    L.tpl_move_bound.restype = L.tpl_move_bound_rows.restype = i32
    for form in ("", "_move"):                               # the bounded form: spare_weight behind the width, the solver's two outputs
        beam, solve = getattr(L, f"tpl_placement_beam{form}_bound"), getattr(L, f"tpl_placement_solve{form}_bound")
        beam.argtypes = [vp, vp, i64, i32, i32, vp, i64, i32, i32, f32, vp, vp, vp, vp]
        solve.argtypes = [vp, vp, i64, i32, i32, vp, i32, f32, vp, vp, vp, vp, vp, vp, vp]
        beam.restype = solve.restype = i32
        exact = getattr(L, f"tpl_placement_exact{form}")     # the exact search: a node budget and a flag for a width
        exact.argtypes = [vp, vp, i64, i32, i32, vp, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        exact.restype = i32
        # the search from a node and the labels of its moves: lines, moves, entry and the shared lists for the configuration's own
        nodes, labels = getattr(L, f"tpl_placement_exact_nodes{form}"), getattr(L, f"tpl_placement_exact_labels{form}")
        nodes.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        labels.argtypes = [vp, vp, vp, vp, vp, i64, i64, i32, i32, vp, f32, i32, vp, vp, vp, vp]
        nodes.restype = labels.restype = i32
        # the search over a state's window: the planes, one weight row, the optional skip mask, then the eight outputs
        window = getattr(L, f"tpl_placement_window_prove{form}")
        window.argtypes = [vp, vp, i64, i32, i32, vp, f32, i32, vp] + [vp] * 8 + [vp]
        window.restype = i32
        # the limited searches: first_limit and growth behind max_nodes and shortest, limit behind nodes
        limited = getattr(L, f"tpl_placement_exact_limited{form}")
        limited.argtypes = exact.argtypes[:9] + [i32, i32] + exact.argtypes[9:15] + [vp, vp]
        limited.restype = i32
        limited = getattr(L, f"tpl_placement_window_prove_limited{form}")
        limited.argtypes = window.argtypes[:8] + [i32, i32] + window.argtypes[8:15] + [vp] + window.argtypes[15:]
        limited.restype = i32
    L.tpl_ntuple_value.argtypes = [vp, vp, i64, i32, i32, vp, vp, vp]
    L.tpl_ntuple_act.argtypes = [vp, vp, i64, i32, i32, f32, f32, f32, f32, vp, f32, u64, u64, vp, vp, vp, vp, vp, vp]
    L.tpl_ntuple_update.argtypes = [vp, vp, i64, i32, i32, vp, vp, f32, vp]
    L.tpl_ntuple_search.argtypes = [vp, vp, i64, i32, i32, f32, f32, f32, f32, vp, f32, u64, u64, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_ntuple_update_trace.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, f32, f32, i32, vp]
    L.tpl_ntuple_update_coherent.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, f32, f32, i32, vp]
    L.tpl_ntuple_entries.restype = i64
    L.tpl_ntuple_entries.argtypes = [i32]
    shaped = ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_update", "tpl_ntuple_search", "tpl_ntuple_update_trace",
              "tpl_ntuple_update_coherent")
    for name in shaped:                                      # the twin's arguments with `shape` before `stream`
        twin = getattr(L, name + "_shaped")
        twin.argtypes = getattr(L, name).argtypes[:-1] + [i32, vp]
        twin.restype = i32
    L.tpl_ntuple_beam.argtypes = [vp, vp, i64, i32, i32, f32, f32, f32, f32, vp, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.tpl_ntuple_beam.restype = i32
    for name in ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_search"):      # a sum table: the unshaped twin's arguments
        twin = getattr(L, name + "_sum")
        twin.argtypes = getattr(L, name).argtypes
        twin.restype = i32
    L.tpl_ntuple_beam_sum.argtypes = L.tpl_ntuple_beam.argtypes[:-2] + [vp]      # tpl_ntuple_beam's without `shape`
    L.tpl_ntuple_beam_sum.restype = i32
    for name in ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_search", "tpl_ntuple_update_trace"):   # a staged table: `form` for `shape`
        twin = getattr(L, name + "_staged")
        twin.argtypes = getattr(L, name + "_shaped").argtypes
        twin.restype = i32
    L.tpl_ntuple_beam_staged.argtypes = L.tpl_ntuple_beam.argtypes
    L.tpl_ntuple_beam_staged.restype = i32
    for name in ("tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_search"):      # a feature form: `form` for `shape`
        twin = getattr(L, name + "_feature")
        twin.argtypes = getattr(L, name + "_shaped").argtypes
        twin.restype = i32
    L.tpl_ntuple_beam_feature.argtypes = L.tpl_ntuple_beam.argtypes
    L.tpl_ntuple_beam_feature.restype = i32
    L.tpl_ntuple_update_trace_feature.argtypes = L.tpl_ntuple_update_trace.argtypes
    L.tpl_ntuple_update_trace_feature.restype = i32
    L.tpl_ntuple_feature_bins.argtypes = [vp, vp, i64, vp, vp]
    L.tpl_ntuple_feature_bins.restype = i32
    # the budget table: the _feature twin's arguments without `form`, the policies with `prune` in its place
    L.tpl_ntuple_value_budget.argtypes = L.tpl_ntuple_value.argtypes
    L.tpl_ntuple_act_budget.argtypes = L.tpl_ntuple_act.argtypes[:-1] + [i32, vp]
    L.tpl_ntuple_search_budget.argtypes = L.tpl_ntuple_search.argtypes[:-1] + [i32, vp]
    L.tpl_ntuple_beam_budget.argtypes = L.tpl_ntuple_beam.argtypes
    L.tpl_ntuple_update_trace_budget.argtypes = L.tpl_ntuple_update_trace.argtypes
    L.tpl_ntuple_budget_bins.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    for name in ("value", "act", "search", "beam", "update_trace"):
        getattr(L, f"tpl_ntuple_{name}_budget").restype = i32
    L.tpl_ntuple_budget_bins.restype = i32
    # the table-ordered exact search: the table and its entry count for the weights, the reward and gamma for spare_weight
    L.tpl_ntuple_exact.argtypes = [vp, vp, i64, i32, i32, vp, i64, f32, f32, f32, f32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.tpl_ntuple_exact.restype = i32
    # the table-ordered window search: tpl_placement_window_prove's arguments with tpl_ntuple_exact's table, reward and gamma
    L.tpl_ntuple_window_prove.argtypes = [vp, vp, i64, i32, i32, vp, i64, f32, f32, f32, f32, i32, vp] + [vp] * 8 + [vp]
    L.tpl_ntuple_window_prove.restype = i32
    # their limited forms: first_limit and growth behind max_nodes and shortest, limit behind nodes
    L.tpl_ntuple_exact_limited.argtypes = L.tpl_ntuple_exact.argtypes[:13] + [i32, i32] + L.tpl_ntuple_exact.argtypes[13:19] + [vp, vp]
    L.tpl_ntuple_window_prove_limited.argtypes = (L.tpl_ntuple_window_prove.argtypes[:12] + [i32, i32] +
                                                  L.tpl_ntuple_window_prove.argtypes[12:19] + [vp] +
                                                  L.tpl_ntuple_window_prove.argtypes[19:])
    L.tpl_ntuple_exact_limited.restype = L.tpl_ntuple_window_prove_limited.restype = i32
    # the ranking update's chooser: the planes, the table and its entry count, the label rows, then the eleven outputs
    L.tpl_ntuple_rank.argtypes = [vp, vp, i64, i32, i32, vp, i64, vp, f32, f32, f32, f32, f32, i32] + [vp] * 12
    L.tpl_ntuple_rank.restype = i32
    # per-configuration tallies and the resampled pool (csrc/learn/curriculum.hip)
    L.tpl_config_index.argtypes = [vp, vp, vp, i64, i64, u64, i32, i64, i64, vp, vp, vp]
    L.tpl_pool_tally.argtypes = [vp, vp, vp, i64, i32, i32, vp, i32, i64, u64, i32, i64, i64, vp, vp, vp, vp, vp]
    L.tpl_pool_resample.argtypes = [vp, vp, i64, i32, vp, i64, u64, u64, vp, vp, vp, vp]
    L.tpl_config_index.restype = L.tpl_pool_tally.restype = L.tpl_pool_resample.restype = i32
    for name in ("tpl_replay_push", "tpl_replay_sample", "tpl_learn_pack", "tpl_priority_init", "tpl_priority_push",
                 "tpl_priority_update", "tpl_replay_sample_prioritized", "tpl_replay_sample_nstep", "tpl_replay_sample_mirror",
                 "tpl_mirror_states", "tpl_afterstates", "tpl_placement_features", "tpl_placement_act",
                 "tpl_placement_search", "tpl_placement_beam", "tpl_ntuple_value", "tpl_ntuple_act", "tpl_ntuple_update",
                 "tpl_ntuple_search", "tpl_ntuple_update_trace", "tpl_ntuple_update_coherent"):
        getattr(L, name).restype = i32
    _handle = L
    return L


def check(status: int) -> None:
    if status != 0:
        raise TplError(f"tpl_learn status {status}: {lib().tpl_learn_last_error().decode()}")


# ------------------------------------------------------------------------------------------------ the sampling hash
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M32 = np.uint64(0xFFFFFFFF)


def _mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _draw_hashes(seed: int, update: int, batch: int) -> np.ndarray:
    """h_i, i < batch: position i + 1 of the splitmix64 stream keyed by (seed, update) (uint64 [batch])."""
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(seed % (1 << 64)) + _GOLDEN * np.uint64((update + 1) % (1 << 64)))
        return _mix64(key + _GOLDEN * (np.arange(batch, dtype=np.uint64) + np.uint64(1)))


def replay_indices(seed: int, update: int, batch: int, size: int) -> np.ndarray:
    """The slots tpl_replay_sample draws (int64 [batch]): draw i is position i + 1 of the splitmix64 stream keyed by
    (seed, update), h, mapped to floor(h * size / 2^64) -- computed from 32-bit halves, exact for size < 2^32."""
    if not 1 <= size < (1 << 32):
        raise ValueError("size must be in [1, 2^32)")
    h = _draw_hashes(seed, update, batch)
    with np.errstate(over="ignore"):
        s = np.uint64(size)
        hi, lo = h >> np.uint64(32), h & _M32
        return ((hi * s + ((lo * s) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the priority tree
# A numpy mirror of csrc/learn/priority.hip (layout and rules: include/tpl_learn.h).  A tree is a float64 array of
# tpl_priority_tree_bytes(capacity) / 8 words, the device image word for word; the header's integer words are viewed as int64.
PRIORITY_HEADER_WORDS = 16
PRIORITY_FANOUT = 16
PRIORITY_MIN, PRIORITY_MAX = 1e-12, 1e30


def priority_layout(capacity: int):
    """(offsets, counts, words): where each level starts (in float64 words from the base), its node count, the image size."""
    if not 1 <= capacity < (1 << 32):
        raise ValueError("capacity must be in [1, 2^32)")
    offsets, counts, n, at = [], [], int(capacity), PRIORITY_HEADER_WORDS
    while True:
        offsets.append(at)
        counts.append(n)
        at += -(-n // PRIORITY_FANOUT) * PRIORITY_FANOUT
        if n == 1:
            return offsets, counts, at
        n = -(-n // PRIORITY_FANOUT)


def priority_tree_init(capacity: int) -> np.ndarray:
    """tpl_priority_init: all zero, running maximum 1.0, the capacity and the number of levels in the header."""
    offsets, _, words = priority_layout(capacity)
    tree = np.zeros(words, dtype=np.float64)
    tree[0] = 1.0
    tree.view(np.int64)[1:3] = (capacity, len(offsets))
    return tree


def _leaves(tree):
    capacity = int(tree.view(np.int64)[1])
    return tree[PRIORITY_HEADER_WORDS:PRIORITY_HEADER_WORDS + capacity], capacity


def priority_tree_resum(tree) -> None:
    """Every node := its 16 children added left to right, one rounding per add (the padding children are 0)."""
    offsets, counts, _ = priority_layout(int(tree.view(np.int64)[1]))
    for k in range(1, len(offsets)):
        child = tree[offsets[k - 1]:offsets[k - 1] + PRIORITY_FANOUT * counts[k]].reshape(counts[k], PRIORITY_FANOUT)
        s = child[:, 0].copy()
        for c in range(1, PRIORITY_FANOUT):
            s = s + child[:, c]
        tree[offsets[k]:offsets[k] + counts[k]] = s


def priority_tree_push(tree: np.ndarray, head: int, count: int) -> np.ndarray:
    """tpl_priority_push, in place: slots [head, head + count) mod capacity get the running maximum."""
    leaves, capacity = _leaves(tree)
    if not (0 <= head < capacity and 1 <= count <= capacity):
        raise ValueError("head must be in [0, capacity) and count in [1, capacity]")
    leaves[(head + np.arange(count)) % capacity] = tree[0]
    priority_tree_resum(tree)
    return tree


def clamp_priorities(priority) -> np.ndarray:
    """fmin(fmax(p, 1e-12), 1e30): NaN and everything below 1e-12 -> 1e-12, +inf -> 1e30."""
    return np.fmin(np.fmax(np.asarray(priority, dtype=np.float64), PRIORITY_MIN), PRIORITY_MAX)


def priority_tree_update(tree: np.ndarray, index, priority) -> np.ndarray:
    """tpl_priority_update, in place: the drawn leaves are zeroed, then each takes the largest clamped priority given for it;
    the running maximum takes the batch's.  Indices outside [0, capacity) are ignored."""
    leaves, capacity = _leaves(tree)
    index, priority = np.asarray(index, dtype=np.int64), np.asarray(priority, dtype=np.float64)
    keep = (index >= 0) & (index < capacity)
    index, p = index[keep], clamp_priorities(priority[keep])
    leaves[index] = 0.0
    np.maximum.at(leaves, index, p)
    if p.size:
        tree[0] = max(tree[0], p.max())
    priority_tree_resum(tree)
    return tree


def priority_targets(seed: int, update: int, batch: int, total: float) -> np.ndarray:
    """u_i = ((i + U_i) * total) / batch in float64, U_i = (h_i >> 11) * 2^-53 (tpl_priority_target)."""
    U = (_draw_hashes(seed, update, batch) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return ((np.arange(batch, dtype=np.float64) + U) * np.float64(total)) / np.float64(batch)


def prioritized_draws(tree: np.ndarray, seed: int, update: int, batch: int):
    """The slots tpl_replay_sample_prioritized draws and their prob = float32(leaf / total): (int64 [batch], float32 [batch])."""
    capacity = int(tree.view(np.int64)[1])
    offsets, _, _ = priority_layout(capacity)
    total = tree[offsets[-1]]
    u = priority_targets(seed, update, batch, total)
    j = np.zeros(batch, dtype=np.int64)
    leaf = np.full(batch, tree[offsets[0]])
    lanes = np.arange(PRIORITY_FANOUT)
    for k in range(len(offsets) - 1, 0, -1):
        line = tree[offsets[k - 1] + PRIORITY_FANOUT * j[:, None] + lanes]
        pick, picked = np.full(batch, -1), np.zeros(batch)
        last, last_v = np.zeros(batch, dtype=np.int64), np.zeros(batch)
        for c in range(PRIORITY_FANOUT):
            x = line[:, c]
            open_ = pick < 0
            take = open_ & (u < x)
            pick, picked = np.where(take, c, pick), np.where(take, x, picked)
            u = np.where(open_ & ~take, u - x, u)
            last, last_v = np.where(x > 0, c, last), np.where(x > 0, x, last_v)
        none = pick < 0
        pick, picked = np.where(none, last, pick), np.where(none, last_v, picked)
        j, leaf = j * PRIORITY_FANOUT + pick, picked
    return np.minimum(j, capacity - 1), (leaf / total).astype(np.float32)


# ------------------------------------------------------------------------------------------------ n-step returns
def nstep_targets(records, capacity: int, size: int, head: int, stride: int, slots, n_step: int, gamma: float):
    """The n-step rule of include/tpl_learn.h for drawn `slots` (i64 [B]) of a ring of [capacity, 80] record bytes:
    (R f32, discount f32, done u8, steps u8, s'-source slot i64), each [B], as tpl_replay_sample_nstep writes them.  Float32
    numpy operations, each product and each sum rounded once."""
    capacity, size, head, stride, n_step = int(capacity), int(size), int(head), int(stride), int(n_step)
    if not (1 <= capacity < (1 << 32) and 1 <= size <= capacity and 0 <= head < capacity and 1 <= stride <= capacity
            and 1 <= n_step <= NSTEP_MAX and 0.0 <= gamma <= 1.0 and (size == capacity or head == size)):
        raise ValueError("nstep_targets: arguments outside what tpl_replay_sample_nstep takes")
    rec = np.ascontiguousarray(records, dtype=np.uint8).reshape(capacity, RECORD_BYTES)
    reward = rec[:, 64:68].copy().view(np.float32).reshape(-1)
    dones = rec[:, 69]
    j = np.asarray(slots, dtype=np.int64)
    g32 = np.float32(gamma)
    age = (head - 1 - j) % capacity
    ret, g = reward[j].copy(), np.ones(j.shape, np.float32)
    last = np.zeros(j.shape, np.int64)
    open_ = dones[j] == 0
    for k in range(1, n_step):
        take = open_ & (k * stride <= age)
        sk = (j + k * stride) % capacity
        gk = g * g32
        ret = np.where(take, ret + gk * reward[sk], ret)
        g = np.where(take, gk, g)
        last = np.where(take, k, last)
        open_ = take & (dones[sk] == 0)
    src = (j + last * stride) % capacity
    done = dones[src].copy()
    discount = np.where(done != 0, np.float32(0.0), g * g32).astype(np.float32)
    return ret.astype(np.float32), discount, done, (last + 1).astype(np.uint8), src


# ------------------------------------------------------------------------------------------------ mirror symmetry
# A numpy mirror of csrc/learn/tpl_mirror.h (the rule: include/tpl_learn.h).
PIECE_MIRROR = (0, 2, 1, 3, 5, 4, 6, 7)                  # pi: L <-> J, S <-> Z
# the observation of the mirrored state is obs[:, MIRROR_OBS_PERM] of the state's (an involution)
MIRROR_OBS_PERM = np.array([10 * y + 9 - x for y in range(20) for x in range(10)] + [200 + p for p in PIECE_MIRROR[:7]]
                           + [207 + p for p in PIECE_MIRROR[:7]] + [214, 215, 216], dtype=np.int64)


def mirror_mode(mirror) -> int:
    """sample(mirror=...) -> 0 (False), 1 (True: the coin) or 2 ("always"); ValueError for anything else, 0 and 1 included."""
    if isinstance(mirror, (bool, str)) and mirror in MIRROR_MODES:
        return MIRROR_MODES[mirror]
    raise ValueError('mirror must be False, True (each draw mirrored on its coin) or "always"')


def mirror_states(a, b):
    """The mirror of states given as plane pairs (uint32 / int32 [K, 4] each) -> (A, B) uint32 [K, 4]: column x <-> column
    9 - x, every window entry p -> PIECE_MIRROR[p]; lines, moves, state, slot and the unused bit 31 of B.y stay."""
    A = np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4).astype(np.uint64)
    B = np.ascontiguousarray(b).view(np.uint32).reshape(-1, 4).astype(np.uint64)
    u = np.uint64
    c20, top4 = u(0xFFFFF), u(60)
    # three 20-bit columns and a 4-bit field per 64 bits: (A.x, A.y), (A.z, A.w), (B.x, B.y); then col9 | lines | window[35:32]
    w64 = [A[:, 0] | (A[:, 1] << u(32)), A[:, 2] | (A[:, 3] << u(32)), B[:, 0] | (B[:, 1] << u(32))]
    cols = [(w >> u(20 * k)) & c20 for w in w64 for k in range(3)] + [B[:, 2] & c20]
    cols = cols[::-1]
    out = [cols[3 * j] | (cols[3 * j + 1] << u(20)) | (cols[3 * j + 2] << u(40)) | ((w64[j] >> top4) << top4) for j in range(3)]
    window = B[:, 3] | ((B[:, 2] >> u(28)) << u(32))
    mirrored = np.zeros_like(window)
    pi = np.array(PIECE_MIRROR, dtype=np.uint64)
    for e in range(12):
        mirrored |= pi[((window >> u(3 * e)) & u(7)).astype(np.int64)] << u(3 * e)
    lo, m32 = u(0xFFFFFFFF), u(32)
    bz = cols[9] | (B[:, 2] & u(0x0FF00000)) | ((mirrored >> m32) << u(28))
    A2 = np.stack([out[0] & lo, out[0] >> m32, out[1] & lo, out[1] >> m32], axis=1).astype(np.uint32)
    B2 = np.stack([out[2] & lo, out[2] >> m32, bz, mirrored & lo], axis=1).astype(np.uint32)
    return A2, B2


_widths = None


def shape_widths() -> np.ndarray:
    """int64 [8, 4]: the width of shape table entry [piece][rotations & 3], through the environment library's host shape
    query; row 7 ("none") is the table's own entry for it, O's."""
    global _widths
    if _widths is None:
        w = [[_lib.shape_info(p, r)[1] for r in range(4)] for p in range(7)]
        _widths = np.array(w + [w[6]], dtype=np.int64)
    return _widths


def mirror_actions(action, a, b) -> np.ndarray:
    """The mirror of actions (u8 [K]) taken in the states (a, b) as given: r = (a // 10) & 3, l = a % 10, w the width of
    [cur][r], a' = 10 ((4 - r) & 3) + (10 - w - min(l, 10 - w)) (uint8 [K], always below 40)."""
    act = np.asarray(action, dtype=np.uint8).astype(np.int64).reshape(-1)
    cur = (np.ascontiguousarray(b).view(np.uint32).reshape(-1, 4)[:, 3] & np.uint32(7)).astype(np.int64)
    r, l = (act // 10) & 3, act % 10
    w = shape_widths()[cur, r]
    return (10 * ((4 - r) & 3) + (10 - w - np.minimum(l, 10 - w))).astype(np.uint8)


def mirror_coins(seed: int, update: int, batch: int) -> np.ndarray:
    """Which draws of a minibatch mode 1 mirrors (uint8 [batch]): bit 0 of h_i, the hash word replay_indices maps."""
    return (_draw_hashes(seed, update, batch) & np.uint64(1)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ afterstates
# The canonical-action rule of include/tpl_learn.h in numpy (the device's: csrc/learn/afterstates.hip).
NUM_ACTIONS = 40
PIECE_ROTATIONS = (2, 4, 4, 4, 2, 2, 1, 1)               # nrot: `rotations % len` of each piece id; 7 ("none") reads O's entry


def canonical_actions(cur, action) -> np.ndarray:
    """canonical[a] = 10 (r mod nrot(cur)) + min(l, 10 - w(cur, r)) for a = 10 r + l in 0..39 and current piece cur in 0..7
    (broadcast against each other; uint8).  Two actions with one canonical value are the same placement."""
    cur, act = np.broadcast_arrays(np.asarray(cur, dtype=np.int64), np.asarray(action, dtype=np.int64))
    if cur.size and (cur.min() < 0 or cur.max() > 7 or act.min() < 0 or act.max() >= NUM_ACTIONS):
        raise ValueError("cur must be in 0..7 and action in 0..39")
    r, l = act // 10, act % 10
    w = shape_widths()[cur, r]
    return (10 * (r % np.array(PIECE_ROTATIONS)[cur]) + np.minimum(l, 10 - w)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ placement features
# The feature table of include/tpl_learn.h on the host, counted on the 20 x 10 array of 0 / 1 cells (the device works on column
# words with ctz / popcount: csrc/learn/heuristic.hip -- the two share nothing), and the score rule.
NUM_FEATURES = 12
FEATURE_NAMES = ("cleared", "won", "lost", "holes", "aggregate_height", "max_height", "bumpiness", "row_transitions",
                 "column_transitions", "wells", "rows_with_holes", "hole_depth")
# the 14-feature form: the two features of the move itself behind the twelve of the board it leaves (host_move_features)
NUM_MOVE_FEATURES = 14
MOVE_WEIGHT_STRIDE = 16                                  # floats between two weight rows of the 14-feature kernels
MOVE_FEATURE_NAMES = FEATURE_NAMES + ("landing_height", "eroded_cells")
FEATURE_COUNTS = (NUM_FEATURES, NUM_MOVE_FEATURES)


def entry(name: str, count: int, bound: bool = False):
    """The entry point tpl_placement_<name> of the feature set with `count` features (12 or 14); bound=True: its bounded form
    (beam and solve have one; exact, exact_nodes, exact_labels and window_prove are of the bounded form as they stand and have no
    other)."""
    if count not in FEATURE_COUNTS:
        raise ValueError(f"a weight row has {NUM_FEATURES} or {NUM_MOVE_FEATURES} entries, not {count}")
    return getattr(lib(), f"tpl_placement_{name}" + ("_move" if count == NUM_MOVE_FEATURES else "") + ("_bound" if bound else ""))


def padded_weights(w: np.ndarray) -> np.ndarray:
    """float32 [P, 12] as it is; [P, 14] -> [P, 16], the stride of the 14-feature kernels, zeros in entries 14 and 15."""
    if w.shape[-1] == NUM_FEATURES:
        return w
    out = np.zeros(w.shape[:-1] + (MOVE_WEIGHT_STRIDE,), np.float32)
    out[..., :NUM_MOVE_FEATURES] = w
    return out


def board_features(rows) -> np.ndarray:
    """Features 3..11 of boards given as row masks (uint16 [K, 20] or [20], bit x = column x, row 0 = top) -> int64 [K, 9]:
    holes, aggregate_height, max_height, bumpiness, row_transitions, column_transitions, wells, rows_with_holes, hole_depth.
    Every feature is counted on the 20 x 10 array of 0 / 1 cells as the table words it."""
    rows = np.asarray(rows)
    if rows.ndim == 1:
        rows = rows[None]
    if rows.ndim != 2 or rows.shape[1] != 20:
        raise ValueError("rows must be [K, 20] row masks")
    k = rows.shape[0]
    cell = (rows.astype(np.int64)[:, :, None] // (2 ** np.arange(10))[None, None, :]) % 2          # [K, 20, 10], 1 = filled
    above = np.cumsum(cell, axis=1) - cell                     # filled cells of the column strictly above each cell
    hole = (cell == 0) & (above > 0)
    occupied = cell.any(axis=1)
    height = np.where(occupied, 20 - cell.argmax(axis=1), 0)   # argmax: the first (top-most) filled row
    bump = np.abs(height[:, 1:] - height[:, :-1]).sum(axis=1)
    wall = np.ones((k, 20, 1), dtype=np.int64)
    line = np.concatenate([wall, cell, wall], axis=2)          # wall, x = 0..9, wall
    row_trans = (line[:, :, 1:] != line[:, :, :-1]).sum(axis=(1, 2))
    col_trans = (cell[:, 1:, :] != cell[:, :-1, :]).sum(axis=(1, 2)) + (cell[:, 19, :] == 0).sum(axis=1)
    beside = np.concatenate([np.full((k, 1), 20), height, np.full((k, 1), 20)], axis=1)           # h_{-1} = h_10 = 20
    d = np.maximum(0, np.minimum(beside[:, :-2], beside[:, 2:]) - height)
    wells = (d * (d + 1) // 2).sum(axis=1)
    first_hole = hole.argmax(axis=1)                           # the top-most hole of each column, where it has one
    above_it = np.take_along_axis(above, first_hole[:, None, :], axis=1)[:, 0, :]
    depth = np.where(hole.any(axis=1), above_it, 0).sum(axis=1)
    return np.stack([hole.sum(axis=(1, 2)), height.sum(axis=1), height.max(axis=1), bump, row_trans, col_trans, wells,
                     hole.any(axis=2).sum(axis=1), depth], axis=1).astype(np.int64)


def move_bound_cells(rows, lines_left) -> np.ndarray:
    """The move bound's `cells` (include/tpl_learn.h) of boards given as row masks (uint16 [K, 20] or [20], bit x = column x) with
    `lines_left` rows still owed ([K] or one number, each >= 0) -> int64 [K]: the sum of the lines_left smallest row costs, a row with
    f < 10 filled cells costing 10 - f and a full row 10, the twenty costs extended by 10s.  Counted on the 0 / 1 cells, row by row
    (the device adds the ten column words bit-sliced: csrc/learn/tpl_placement.h -- the two share nothing)."""
    rows = np.asarray(rows)
    if rows.ndim == 1:
        rows = rows[None]
    if rows.ndim != 2 or rows.shape[1] != 20:
        raise ValueError("rows must be [K, 20] row masks")
    k = rows.shape[0]
    left = np.broadcast_to(np.asarray(lines_left, dtype=np.int64), (k,))
    if left.size and left.min() < 0:
        raise ValueError("lines_left must not be negative")
    cell = (rows.astype(np.int64)[:, :, None] // (2 ** np.arange(10))[None, None, :]) % 2          # [K, 20, 10], 1 = filled
    fill = cell.sum(axis=2)
    cost = np.sort(np.where(fill < 10, 10 - fill, 10), axis=1)
    upto = np.concatenate([np.zeros((k, 1), np.int64), np.cumsum(cost, axis=1)], axis=1)          # upto[:, j] = the j cheapest
    return upto[np.arange(k), np.minimum(left, 20)] + 10 * np.maximum(left - 20, 0)


def move_bound(rows, L: int, M: int, lines, moves, state) -> dict:
    """The move bound of boards in row form under the game's L and M (include/tpl_learn.h): cells and spare = 4 (M - moves) - cells
    for a running board (a running board whose lines have reached L owes nothing), both 0 for a finished one; need =
    ceil(cells / 4); dead = spare < 0.  int64 [K] each, dead bool."""
    rows = np.asarray(rows)
    rows = rows[None] if rows.ndim == 1 else rows
    k = rows.shape[0]
    lines, moves, state = (np.broadcast_to(np.asarray(x, dtype=np.int64), (k,)) for x in (lines, moves, state))
    running = state == STATE_RUNNING
    cells = np.where(running, move_bound_cells(rows, np.maximum(int(L) - lines, 0)), 0)
    spare = np.where(running, 4 * (int(M) - moves) - cells, 0)
    return dict(cells=cells, spare=spare, need=(cells + 3) // 4, dead=spare < 0)


def placement_score(features, weights) -> np.ndarray:
    """score = w_0 phi_0 + w_1 phi_1 + ... + w_11 phi_11 from left to right in float32, every product and every sum rounded
    once (numpy float32 operations; nothing fused): features [..., 12] integers, weights [12] or broadcastable [..., 12].
    The 14-feature form: both end in 14 and the sum runs two terms further."""
    f = np.asarray(features)
    w = np.asarray(weights, dtype=np.float32)
    count = f.shape[-1]
    if count not in FEATURE_COUNTS or w.shape[-1] != count:
        raise ValueError("features and weights must both end in 12 or both in 14")
    f = f.astype(np.float32)                                  # exact: every feature is a small integer
    s = w[..., 0] * f[..., 0]
    for k in range(1, count):
        s = s + w[..., k] * f[..., k]
    return np.asarray(s, dtype=np.float32)


NO_SECOND = 255


def search_choice(phi1, done1, distinct1, phi2, distinct2, weights):
    """The two-ply rule of include/tpl_learn.h (tpl_placement_search) on features that are given: phi1 [K, 40, 12] the one-ply
    features of every first placement a, done1 [K, 40] where the first move ends the game (every a of a finished board),
    distinct1 [K, 40] where a is a distinct placement of the current piece, phi2 [K, 40, 40, 12] = psi(a, b) (read only where
    done1 is not set), distinct2 [K, 40] or [K, 40, 40] where b is a distinct placement of the next piece; weights [12], or one
    row per board [K, 12].  Returns (action u8 [K], second u8 [K] -- 255 where the chosen first move ends the game --, score
    f32 [K]): V(a) = the one-ply score where done1, else the maximum over the distinct b of placement_score, the lowest index
    at each maximum (-0 and +0 tie).  The 14-feature form: phi1, phi2 and weights end in 14, phi2 holding the landing and eroded
    sums of both moves."""
    phi1, phi2 = np.asarray(phi1), np.asarray(phi2)
    k, count = phi1.shape[0], phi1.shape[-1]
    if count not in FEATURE_COUNTS or phi1.shape != (k, NUM_ACTIONS, count) or phi2.shape != (k, NUM_ACTIONS, NUM_ACTIONS, count):
        raise ValueError("phi1 must be [K, 40, 12] and phi2 [K, 40, 40, 12], or both end in 14")
    done1, distinct1, distinct2 = (np.asarray(x).astype(bool) for x in (done1, distinct1, distinct2))
    if distinct2.ndim == 2:
        distinct2 = distinct2[:, None, :]
    if done1.shape != (k, NUM_ACTIONS) or distinct1.shape != (k, NUM_ACTIONS) or distinct2.shape[::2] != (k, NUM_ACTIONS):
        raise ValueError("done1 and distinct1 must be [K, 40] and distinct2 [K, 40] or [K, 40, 40]")
    w = np.asarray(weights, dtype=np.float32)
    if w.shape[-1] != count:
        raise ValueError(f"weights must end in {count}, as the features do")
    w = w.reshape(-1, count)
    if w.shape[0] not in (1, k):
        raise ValueError(f"weights must be [{count}] or one row per board")
    rows = np.arange(k)[:, None]
    first = np.arange(NUM_ACTIONS)[None, :]
    score2 = np.where(distinct2, placement_score(phi2, w[:, None, None, :]), -np.inf)
    second = np.argmax(score2 == score2.max(axis=2, keepdims=True), axis=2)       # the lowest b at the maximum
    value = np.where(done1, placement_score(phi1, w[:, None, :]), score2[rows, first, second]).astype(np.float32)
    second = np.where(done1, NO_SECOND, second)
    masked = np.where(distinct1, value, -np.inf)
    action = np.argmax(masked == masked.max(axis=1, keepdims=True), axis=1)
    at = np.arange(k)
    return action.astype(np.uint8), second[at, action].astype(np.uint8), value[at, action]


def beam_select(values, width: int) -> np.ndarray:
    """The one non-obvious step of the beam rule of include/tpl_learn.h (tpl_placement_beam): of candidates with float32
    `values` [count], listed in candidate order, the indices of the min(width, count) best under (value descending, index
    ascending; -0 and +0 tie), IN CANDIDATE ORDER (int64, ascending) -- a stable compaction, not a sort."""
    v = np.asarray(values, dtype=np.float32)
    if v.ndim != 1 or v.size < 1:
        raise ValueError("values must be a non-empty vector")
    if isinstance(width, bool) or int(width) != width or not 1 <= int(width) <= BEAM_MAX_WIDTH:
        raise ValueError(f"width must be an integer in [1, {BEAM_MAX_WIDTH}]")
    order = np.argsort(-(v + np.float32(0.0)), kind="stable")  # x + 0 makes -0 a +0; stable: the lower index first among equals
    return np.sort(order[:int(width)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the whole-game solver
# The rule of tpl_placement_solve (include/tpl_learn.h) on the host, from the ROW form of a board: a move on row masks out of the
# shape query's row patterns, board_features, placement_score and the order of beam_select.  The device works on column words
# (csrc/learn/solve.hip, csrc/tpl_device.h) -- the two share nothing.
SOLVE_MAX_MOVES = 254
STATE_RUNNING, STATE_WON, STATE_LOST_LIMIT, STATE_LOST_TOPOUT = 0, 1, 2, 3
_shape_tables = None


def _solve_shape_tables():
    """(height [8, 4], width [8, 4], row pattern [8, 4, 4], lowest cell of each piece column [8, 4, 4]) of shape table entry
    [piece][rotations & 3], through the environment library's host shape query; row 7 ("none") is O's."""
    global _shape_tables
    if _shape_tables is None:
        h, w = np.zeros((8, 4), np.int64), np.zeros((8, 4), np.int64)
        mask, low = np.zeros((8, 4, 4), np.int64), np.zeros((8, 4, 4), np.int64)
        for p in range(8):
            for r in range(4):
                hh, ww, masks, topo = _lib.shape_info(min(p, 6), r)
                h[p, r], w[p, r] = hh, ww
                mask[p, r, :hh], low[p, r, :ww] = masks, topo
        _shape_tables = (h, w, mask, low)
    return _shape_tables


def host_moves(rows, piece, rotations, location, L: int, M: int, lines, moves):
    """host_moves_traced without the trace."""
    return host_moves_traced(rows, piece, rotations, location, L, M, lines, moves)[:5]


def host_move_features(rows, piece, rotations, location, L: int, M: int, lines, moves):
    """Features 12 and 13 of include/tpl_learn.h for `piece` played on K running boards (host_moves' arguments): returns
    (drop int64 [K], cleared_rows bool [K, 20], landing_height int64 [K], eroded_cells int64 [K]).  drop is the row of the piece's
    top-most mask row after the fall (negative on a top-out), cleared_rows the rows that were full after the lock, in the
    coordinates of the board BEFORE the compaction; landing_height = 39 - 2 drop - h and eroded_cells = (rows cleared) x (the
    piece's cells in cleared rows), both 0 on a top-out."""
    return host_moves_traced(rows, piece, rotations, location, L, M, lines, moves)[5:]


def host_moves_traced(rows, piece, rotations, location, L: int, M: int, lines, moves):
    """Tetris.move(rotations, location) with `piece` on K running boards in row form (uint16 [K, 20], bit x = column x, row 0 = top;
    the rest [K]): the right clamp, the drop from the column tops under the piece, the top-out (board and moves stay), the lock, the
    full-row test over the piece's rows, the compaction, then won (rows were cleared and lines >= L) before the move limit
    (moves >= M).  Returns (rows uint16 [K, 20], cleared, lines, moves, state) -- state 0 running, 1 won, 2 lost at the limit,
    3 topped out -- and behind them host_move_features' four."""
    H, W_, MASK, LOW = _solve_shape_tables()
    rows = np.array(rows, dtype=np.uint16).reshape(-1, 20).astype(np.int64)
    k = rows.shape[0]
    piece, rot = np.broadcast_to(np.asarray(piece, np.int64) & 7, (k,)), np.broadcast_to(np.asarray(rotations, np.int64) & 3, (k,))
    lines, moves = np.broadcast_to(np.asarray(lines, np.int64), (k,)).copy(), np.broadcast_to(np.asarray(moves, np.int64), (k,)).copy()
    h, w = H[piece, rot], W_[piece, rot]
    loc = np.minimum(np.broadcast_to(np.asarray(location, np.int64), (k,)), 10 - w)
    at = np.arange(k)
    cell = (rows[:, :, None] >> np.arange(10)) & 1
    top = np.where(cell.any(axis=1), cell.argmax(axis=1), 20)                       # [K, 10]: the top-most filled row, 20 if none
    delta = np.full(k, 1 << 20, np.int64)
    for c in range(4):
        d = top[at, np.minimum(loc + c, 9)] - LOW[piece, rot, c]
        delta = np.where(c < w, np.minimum(delta, d), delta)
    drop = delta - 1
    ok = drop >= 0
    cleared_row = np.zeros((k, 20), bool)
    for i in range(4):
        put = ok & (i < h)
        r = np.where(put, drop + i, 0)
        rows[at, r] |= np.where(put, MASK[piece, rot, i] << loc, 0)
    for i in range(4):
        put = ok & (i < h)
        r = np.where(put, drop + i, 0)
        full = put & (rows[at, r] == 0x3FF)
        cleared_row[at[full], r[full]] = True
    n = cleared_row.sum(axis=1)
    # the move's own features: the piece's cells row by row, counted where the row was cleared
    in_cleared = np.zeros(k, np.int64)
    for i in range(4):
        put = ok & (i < h)
        cells = np.array([bin(m).count("1") for m in range(16)])[MASK[piece, rot, i]]
        in_cleared += np.where(put & cleared_row[at, np.where(put, drop + i, 0)], cells, 0)
    landing = np.where(ok, 39 - 2 * drop - h, 0)
    eroded = n * in_cleared
    trace = (drop, cleared_row.copy(), landing, eroded)
    order = np.argsort(~cleared_row, axis=1, kind="stable")                        # the cleared rows first, the others in order
    rows = np.take_along_axis(rows, order, axis=1)
    rows[np.arange(20)[None, :] < n[:, None]] = 0
    moves += ok
    lines += n
    won = ok & (n > 0) & (lines >= L)
    limit = ok & ~won & (moves >= M)
    state = np.where(~ok, STATE_LOST_TOPOUT, np.where(won, STATE_WON, np.where(limit, STATE_LOST_LIMIT, STATE_RUNNING)))
    return (rows.astype(np.uint16), n, lines, moves, state) + trace


def _first_in_order(values) -> int:
    """The index of the candidate that comes first under (value descending, index ascending; -0 and +0 tie)."""
    v = np.asarray(values, dtype=np.float32) + np.float32(0.0)
    return int(np.argmax(v == v.max()))


def placement_solve(rows, pieces, L: int, M: int, weights, width: int, max_width: int = BEAM_MAX_WIDTH, chunk: int = 1 << 14,
                    bound: bool = False, spare_weight: float = 0.0):
    """The rule of tpl_placement_solve (include/tpl_learn.h) for n configurations: rows uint16 [n, 20] (bit x = column x), pieces
    [n, M + 1] (masked to three bits), one weight row [12] -- or [14], the 14-feature form, in which a node also carries the landing
    and eroded sums of its path --, a width in [1, max_width].  The placement beam run through the whole
    piece list: ply j plays pieces[:, j - 1]; the search ends at the first ply at which ANY candidate is won, before the cut, with the
    path of the won candidate that comes first in the rule's order, or unsolved once no node of the beam runs.  Returns
    (solved uint8 [n], solution_len int32 [n], actions uint8 [n, M] padded with 255, best_value float32 [n, M], +0 beyond the
    plies run) in the C layout.  solved = 0 means that this beam found no win, not that there is none.
    bound=True is the bounded form (tpl_placement_solve_bound): a child that is left running and dead (move_bound) becomes lost at
    the limit before psi is built, spare_weight * float32(spare) is added to the score last, in float32, and two more arrays are
    returned behind the four: bound int32 [n] = need(root), and complete uint8 [n], 1 iff no cut dropped a running candidate -- under
    which solved = 0 is a proof that there is no win and solved = 1 that solution_len is the shortest.  A spare_weight other than 0
    needs bound=True.
    `max_width` is for the test that compares a beam wide enough to keep everything with an exhaustive search; the kernel's limit
    is BEAM_MAX_WIDTH.  `chunk` bounds how many candidates are moved and counted at once."""
    L, M = int(L), int(M)
    if not (1 <= L <= 250 and 1 <= M <= SOLVE_MAX_MOVES):
        raise ValueError(f"L and M must be in [1, 250] and [1, {SOLVE_MAX_MOVES}]")
    if isinstance(width, bool) or int(width) != width or not 1 <= int(width) <= int(max_width):
        raise ValueError(f"width must be an integer in [1, {int(max_width)}]")
    width = int(width)
    rows = np.asarray(rows)
    rows = (rows.view(np.uint16) if rows.dtype == np.int16 else rows.astype(np.uint16)).reshape(-1, 20)
    n = rows.shape[0]
    pieces = np.asarray(pieces).astype(np.int64) & 7
    if n < 1 or pieces.shape != (n, M + 1):
        raise ValueError(f"rows must be [n, 20] and pieces [n, {M + 1}] with n >= 1")
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    if w.shape not in ((NUM_FEATURES,), (NUM_MOVE_FEATURES,)):
        raise ValueError("weights must be one row of 12 or of 14")
    move = w.shape[0] == NUM_MOVE_FEATURES
    if not isinstance(bound, (bool, np.bool_)):
        raise ValueError("bound must be True or False")
    with np.errstate(over="ignore"):
        spare_weight = np.float32(spare_weight)
    if not np.isfinite(spare_weight):
        raise ValueError("spare_weight must be finite (in float32)")
    if spare_weight != 0 and not bound:
        raise ValueError("spare_weight belongs to the bounded form: give bound=True")
    root_need = move_bound(rows, L, M, 0, 0, STATE_RUNNING)["need"].astype(np.int32)
    complete = np.ones(n, np.uint8)
    placements = [np.flatnonzero(canonical_actions(p, np.arange(NUM_ACTIONS)) == np.arange(NUM_ACTIONS)) for p in range(8)]
    solved, length = np.zeros(n, np.uint8), np.zeros(n, np.int32)
    actions, best_value = np.full((n, M), NO_SECOND, np.uint8), np.zeros((n, M), np.float32)
    # a beam: the nodes' rows, lines, moves, state and value in stored order; tape[j] = (parent's place, placement) of Beam_{j+1}
    beams = [dict(rows=rows[s:s + 1].copy(), lines=np.zeros(1, np.int64), moves=np.zeros(1, np.int64),
                  state=np.zeros(1, np.int64), value=np.zeros(1, np.float32), sums=np.zeros((1, 2), np.int64), tape=[])
             for s in range(n)]
    active = list(range(n))
    for ply in range(M):
        # every child of every running node of every configuration still searched, in one batch
        cfg, place, first, p_rows, p_lines, p_moves, p_sums, total = [], [], {}, [], [], [], [], 0
        for s in active:                                        # every active configuration has a running node
            run = np.flatnonzero(beams[s]["state"] == STATE_RUNNING)
            b = placements[pieces[s, ply]]
            node = np.repeat(run, b.size)                       # node by node, ascending b: the candidates' order
            first[s] = total
            total += node.size
            cfg.append(np.full(node.size, s)), place.append(np.tile(b, run.size))
            p_rows.append(beams[s]["rows"][node]), p_lines.append(beams[s]["lines"][node]), p_moves.append(beams[s]["moves"][node])
            p_sums.append(beams[s]["sums"][node])
        cfg, place = np.concatenate(cfg), np.concatenate(place)
        p_rows, p_lines, p_moves = np.concatenate(p_rows), np.concatenate(p_lines), np.concatenate(p_moves)
        p_sums, c_sums = np.concatenate(p_sums), np.zeros((total, 2), np.int64)
        c_rows, c_lines, c_moves = np.zeros((total, 20), np.uint16), np.zeros(total, np.int64), np.zeros(total, np.int64)
        c_state, c_value = np.zeros(total, np.int64), np.zeros(total, np.float32)
        for lo in range(0, total, chunk):
            hi = min(total, lo + chunk)
            r2, _, l2, m2, s2, _, _, land, erod = host_moves_traced(p_rows[lo:hi], pieces[cfg[lo:hi], ply], place[lo:hi] // 10,
                                                                    place[lo:hi] % 10, L, M, p_lines[lo:hi], p_moves[lo:hi])
            c_sums[lo:hi] = p_sums[lo:hi] + np.stack([land, erod], axis=1)
            spare = np.zeros(hi - lo, np.int64)
            if bound:                                           # the one place where the bounded form parts from its twin
                mb = move_bound(r2, L, M, l2, m2, s2)
                s2 = np.where(mb["dead"], STATE_LOST_LIMIT, s2)
                spare = np.where(mb["dead"], 0, mb["spare"])
            psi = np.concatenate([np.stack([l2, s2 == STATE_WON, s2 >= STATE_LOST_LIMIT], axis=1).astype(np.int64),
                                  board_features(r2)] + ([c_sums[lo:hi]] if move else []), axis=1)
            c_rows[lo:hi], c_lines[lo:hi], c_moves[lo:hi], c_state[lo:hi] = r2, l2, m2, s2
            c_value[lo:hi] = placement_score(psi, w)
            if bound:                                           # one rounded multiply, one rounded add, made last
                c_value[lo:hi] = c_value[lo:hi] + spare_weight * spare.astype(np.float32)
        still = []
        for s in active:
            beam = beams[s]
            run = beam["state"] == STATE_RUNNING
            count = placements[pieces[s, ply]].size
            sizes = np.where(run, count, 1)
            cand = int(sizes.sum())
            # the candidates in order: a finished node gives itself (child -1), a running node its children in ascending b
            parent = np.repeat(np.arange(run.size), sizes)
            child = np.full(cand, -1, np.int64)
            mine = first[s] + np.arange(int(run.sum()) * count)
            child[run[parent]] = mine
            value = np.where(child >= 0, c_value[np.maximum(child, 0)], beam["value"][parent]).astype(np.float32)
            best_value[s, ply] = value[_first_in_order(value)]
            won = np.flatnonzero((child >= 0) & (c_state[np.maximum(child, 0)] == STATE_WON))
            if won.size:                                        # the stop, before the cut
                at = won[_first_in_order(value[won])]
                path, q = [int(place[child[at]])], int(parent[at])
                for back in reversed(beam["tape"]):
                    path.append(int(back[1][q]))
                    q = int(back[0][q])
                solved[s], length[s] = 1, ply + 1
                actions[s, :ply + 1] = path[::-1]
                continue
            order = np.argsort(-(value + np.float32(0.0)), kind="stable")       # beam_select's order, for any width
            keep = np.sort(order[:width])
            cut = order[width:]
            if (c_state[child[cut][child[cut] >= 0]] == STATE_RUNNING).any():
                complete[s] = 0                                 # the cut dropped a running candidate
            kc, kp = child[keep], parent[keep]
            moved = kc >= 0
            kc0 = np.maximum(kc, 0)
            beam["tape"].append((kp, np.where(moved, place[kc0], NO_SECOND)))
            beams[s] = dict(rows=np.where(moved[:, None], c_rows[kc0], beam["rows"][kp]),
                            lines=np.where(moved, c_lines[kc0], beam["lines"][kp]),
                            moves=np.where(moved, c_moves[kc0], beam["moves"][kp]),
                            state=np.where(moved, c_state[kc0], beam["state"][kp]),
                            sums=np.where(moved[:, None], c_sums[kc0], beam["sums"][kp]),
                            value=value[keep], tape=beam["tape"])
            if (beams[s]["state"] == STATE_RUNNING).any():
                still.append(s)
        active = still
        if not active:
            break
    if bound:
        return solved, length, actions, best_value, root_need, complete
    return solved, length, actions, best_value


# ------------------------------------------------------------------------------------------------ the exact search
# The rule of tpl_placement_exact (include/tpl_learn.h) on the host, from the ROW form of a board again: host_moves_traced,
# move_bound, board_features and placement_score.  The device keeps a stack of packed boards in LDS and ranks keys across a wave
# (csrc/learn/exact.hip) -- the two share nothing.
EXACT_MAX_NODES = 1 << 24


def _exact_arrays(rows, pieces, L: int, M: int, max_nodes, shortest):
    """What placement_exact and ntuple_exact refuse alike, and their arrays: (L, M, max_nodes, rows uint16 [n, 20], pieces int64
    [n, M + 1] masked to three bits)."""
    L, M = int(L), int(M)
    if not (1 <= L <= 250 and 1 <= M <= SOLVE_MAX_MOVES):
        raise ValueError(f"L and M must be in [1, 250] and [1, {SOLVE_MAX_MOVES}]")
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or not 1 <= int(max_nodes) <= EXACT_MAX_NODES:
        raise ValueError(f"max_nodes must be an integer in [1, {EXACT_MAX_NODES}]")
    if not isinstance(shortest, (bool, np.bool_)):
        raise ValueError("shortest must be True or False")
    rows = np.asarray(rows)
    rows = (rows.view(np.uint16) if rows.dtype == np.int16 else rows.astype(np.uint16)).reshape(-1, 20)
    pieces = np.asarray(pieces).astype(np.int64) & 7
    if rows.shape[0] < 1 or pieces.shape != (rows.shape[0], M + 1):
        raise ValueError(f"rows must be [n, 20] and pieces [n, {M + 1}] with n >= 1")
    return L, M, int(max_nodes), rows, pieces


LIMIT_TOP = 65535                                        # the clamp of a discrepancy limit K, and first_limit's largest value
LIMIT_NEVER_CUTS = 8382                                  # a K from here on never cuts: 253 nodes above the one expanded, ranks <= 33
DISCREPANCY_GROWTH = {"add": 0, "double": 1}             # discrepancy= of the Python surface -> the C `growth`


def _limit_arguments(first_limit, growth) -> None:
    """What every limited mirror refuses of its two arguments (first_limit None is the plain rule and takes any growth of the two)."""
    if first_limit is not None and (isinstance(first_limit, bool) or not isinstance(first_limit, (int, np.integer))
                                    or not 0 <= int(first_limit) <= LIMIT_TOP):
        raise ValueError(f"first_limit must be None or an integer in [0, {LIMIT_TOP}]")
    if isinstance(growth, bool) or not isinstance(growth, (int, np.integer)) or int(growth) not in (0, 1):
        raise ValueError("growth must be 0 (add) or 1 (double)")


def _exact_search(rows, pieces, L: int, M: int, max_nodes: int, shortest: bool, children, first_limit=None, growth: int = 0):
    """The depth-first search of placement_exact and ntuple_exact on checked arguments: the budgets, the cap, the stop at the first won
    child in the order (value descending, placement ascending; -0 and +0 tie), the descent and the return.  What a node's children are
    worth is the caller's: children(tops, piece, nxt, b, L, B) takes a batch of children of the game (L, B), one a row -- tops holds
    the parent's rows, lines, moves and extra (None where no parent has any: a root carries nothing), piece the piece placed, nxt the
    one behind it in the list, b the placement -- and returns their (value, state, rows, lines, moves, extra), extra being whatever
    the order keeps along a path, or None.  Returns placement_exact's six arrays.
    first_limit None is the plain rule.  An integer is the LIMITED rule of tpl_placement_exact_limited: an iteration is (B, K), K from
    first_limit; a node holds rem, what is left of K on its path; of its running children those of rank <= rem are kept, the one of
    rank j with rem - j, and a dropped child sets the iteration's cut; a budget searched out with cut set starts again from a fresh
    root under K + 1 (growth 0) or max(1, 2 K) (growth 1), clamped at 65,535, and only one that cut nothing ends the budget.  Then a
    seventh array is returned: limit int32 [n], the K of the last iteration begun.
    The configurations are searched in step, one expansion each a round, so that every round moves and counts the children of all of
    them in one batch per budget."""
    n = rows.shape[0]
    bound = move_bound(rows, L, M, 0, 0, STATE_RUNNING)["need"].astype(np.int32)
    placements = [np.flatnonzero(canonical_actions(p, np.arange(NUM_ACTIONS)) == np.arange(NUM_ACTIONS)) for p in range(8)]
    solved, proved, length = np.zeros(n, np.uint8), np.ones(n, np.uint8), np.zeros(n, np.int32)
    actions, nodes = np.full((n, M), NO_SECOND, np.uint8), np.zeros(n, np.uint32)

    limited = first_limit is not None
    limit, cut = np.zeros(n, np.int32), np.zeros(n, bool)

    def root(s):
        return dict(rows=rows[s], lines=0, moves=0, extra=None, kids=None, at=0, rem=int(limit[s]))

    # a stack per configuration still searched, its last frame the node to expand next; a frame's kids are its running children in
    # the order of the descent -- (placement, rows, lines, moves, extra) each --, `at` the next of them
    budget = {s: int(bound[s]) if shortest else M for s in range(n) if bound[s] <= M}
    if limited:
        limit[sorted(budget)] = int(first_limit)
    stacks = {s: [root(s)] for s in budget}
    while stacks:
        for s in [s for s in stacks if nodes[s] == max_nodes]:  # the cap: nothing is proved, nothing is reported
            proved[s] = 0
            del stacks[s]
        if not stacks:
            break
        todo = sorted(stacks)
        nodes[todo] += 1
        found = {}
        for B in sorted({budget[s] for s in todo}):             # the game (L, B): one batch per budget
            group = [s for s in todo if budget[s] == B]
            tops = [stacks[s][-1] for s in group]
            depth = [len(stacks[s]) - 1 for s in group]
            place = [placements[pieces[s, d]] for s, d in zip(group, depth)]
            sizes = [b.size for b in place]
            rep = lambda per_top: np.repeat(np.array(per_top), sizes, axis=0)
            carried = next((t["extra"] for t in tops if t["extra"] is not None), None)
            batch = dict(rows=rep([t["rows"] for t in tops]), lines=rep([t["lines"] for t in tops]), moves=rep([t["moves"] for t in tops]),
                         extra=None if carried is None else rep([np.zeros_like(carried) if t["extra"] is None else t["extra"] for t in tops]))
            out = children(batch, rep([pieces[s, d] for s, d in zip(group, depth)]), rep([pieces[s, d + 1] for s, d in zip(group, depth)]),
                           np.concatenate(place), L, B)
            lo = 0
            for s, b, size in zip(group, place, sizes):
                found[s] = (b,) + tuple(None if x is None else x[lo:lo + size] for x in out)
                lo += size
        for s in todo:
            b, value, state, c_rows, c_lines, c_moves, c_extra = found[s]
            stack = stacks[s]
            order = np.argsort(-(value + np.float32(0.0)), kind="stable")
            won = order[state[order] == STATE_WON]
            if won.size:                                        # a win at this depth + 1: the path to here, then the won child
                path = [f["kids"][f["at"] - 1][0] for f in stack[:-1]] + [int(b[won[0]])]
                solved[s], length[s] = 1, len(path)
                actions[s, :len(path)] = path
                del stacks[s]
                continue
            run = order[state[order] == STATE_RUNNING]
            if limited and run.size > stack[-1]["rem"] + 1:     # the children of rank <= rem are kept; a dropped one is a cut
                run, cut[s] = run[:stack[-1]["rem"] + 1], True
            stack[-1]["kids"] = [(int(b[k]), c_rows[k], int(c_lines[k]), int(c_moves[k]), None if c_extra is None else c_extra[k]) for k in run]
            while stack and stack[-1]["at"] == len(stack[-1]["kids"]):
                stack.pop()                                     # used up: back to the parent
            if stack:
                top = stack[-1]
                _, k_rows, k_lines, k_moves, k_extra = top["kids"][top["at"]]
                stack.append(dict(rows=k_rows, lines=k_lines, moves=k_moves, extra=k_extra, kids=None, at=0, rem=top["rem"] - top["at"]))
                top["at"] += 1
            elif cut[s]:                                        # something was dropped: the same budget under the next limit
                limit[s], cut[s] = min(max(1, 2 * int(limit[s])) if growth else int(limit[s]) + 1, LIMIT_TOP), False
                stack.append(root(s))
            elif shortest and budget[s] < M:                    # searched out at this budget: the next one
                budget[s] += 1
                if limited:
                    limit[s] = int(first_limit)
                stack.append(root(s))
            else:                                               # searched out: no sequence of placements wins within M moves
                del stacks[s]
    return (solved, proved, length, actions, bound, nodes) + ((limit,) if limited else ())


def placement_exact(rows, pieces, L: int, M: int, weights, max_nodes: int, shortest: bool = True, spare_weight: float = 0.0):
    """The rule of tpl_placement_exact (include/tpl_learn.h) for n configurations: rows uint16 [n, 20] (bit x = column x), pieces
    [n, M + 1] (masked to three bits), one weight row [12] or [14], max_nodes in [1, 2^24], shortest True or False, one finite
    spare_weight.  A depth-first search of the game (L, B) in the bounded form -- a child that the move bound proves lost under B is
    lost --, children ordered by (value descending, placement ascending; -0 and +0 tie), the first won child of a node ending the
    iteration; B runs over need(root) .. M (shortest) or is M alone; `nodes` counts the expansions of all iterations and the search
    gives up, proving nothing, when it would pass max_nodes.  Returns (solved uint8 [n], proved uint8 [n], solution_len int32 [n],
    actions uint8 [n, M] padded with 255, bound int32 [n], nodes uint32 [n]) in the C layout (_exact_search)."""
    return _placement_exact(rows, pieces, L, M, weights, max_nodes, shortest, spare_weight, None, 0)


def placement_exact_limited(rows, pieces, L: int, M: int, weights, max_nodes: int, first_limit: int = 0, growth: int = 0,
                            shortest: bool = True, spare_weight: float = 0.0):
    """The rule of tpl_placement_exact_limited (include/tpl_learn.h): placement_exact in limited-discrepancy order, with first_limit an
    integer in [0, 65535] and growth 0 ("add") or 1 ("double") (_exact_search says what they do).  Under proved the verdicts are
    placement_exact's; first_limit >= 8,382 gives its outputs byte for byte.  Returns its six arrays and limit int32 [n], the K of the
    last iteration begun.  first_limit None is placement_exact itself, six arrays."""
    return _placement_exact(rows, pieces, L, M, weights, max_nodes, shortest, spare_weight, first_limit, growth)


def _placement_exact(rows, pieces, L, M, weights, max_nodes, shortest, spare_weight, first_limit, growth):
    L, M, max_nodes, rows, pieces = _exact_arrays(rows, pieces, L, M, max_nodes, shortest)
    _limit_arguments(first_limit, growth)
    w = np.asarray(weights, dtype=np.float32).reshape(-1)
    if w.shape not in ((NUM_FEATURES,), (NUM_MOVE_FEATURES,)):
        raise ValueError("weights must be one row of 12 or of 14")
    move = w.shape[0] == NUM_MOVE_FEATURES
    with np.errstate(over="ignore"):
        spare_weight = np.float32(spare_weight)
    if not np.isfinite(spare_weight):
        raise ValueError("spare_weight must be finite (in float32)")

    def children(tops, piece, nxt, b, L, B):                    # the linear order; extra: the path's landing and eroded sums
        r2, _, l2, m2, s2, _, _, land, erod = host_moves_traced(tops["rows"], piece, b // 10, b % 10, L, B, tops["lines"], tops["moves"])
        sums = np.stack([land, erod], axis=1) + (0 if tops["extra"] is None else tops["extra"])
        mb = move_bound(r2, L, B, l2, m2, s2)
        s2 = np.where(mb["dead"], STATE_LOST_LIMIT, s2)
        spare = np.where(mb["dead"], 0, mb["spare"])
        psi = np.concatenate([np.stack([l2, s2 == STATE_WON, s2 >= STATE_LOST_LIMIT], axis=1).astype(np.int64),
                              board_features(r2)] + ([sums] if move else []), axis=1)
        value = placement_score(psi, w)
        return value + spare_weight * spare.astype(np.float32), s2, r2, l2, m2, sums

    return _exact_search(rows, pieces, L, M, max_nodes, bool(shortest), children, first_limit, int(growth))


# ------------------------------------------------------------------------------------------------ the exact search from a node
# The rules of tpl_placement_exact_nodes and tpl_placement_exact_labels (include/tpl_learn.h) on the host, from the ROW form: the
# nodes are grouped by (lines, moves), each group is handed to placement_exact as configurations of its SHIFTED game, and the one
# move of a label is host_moves_traced and move_bound under the game's own (L, M).  The device shifts per wave and runs its own
# copy of the search (csrc/learn/exact_nodes.hip) -- the two share nothing.
LABEL_NONE, LABEL_WIN, LABEL_LOSS, LABEL_OPEN = 0, 1, 2, 3


def _node_arrays(rows, lines, moves, entry, pieces, L: int, M: int):
    """The node arguments of both mirrors, checked: rows uint16 [n, 20], lines / moves / entry int64 [n], pieces int64 [n_cfg, M + 1]
    masked to three bits, and `live` [n], False where the kernel treats the node as finished."""
    L, M = int(L), int(M)
    if not (1 <= L <= 250 and 1 <= M <= SOLVE_MAX_MOVES):
        raise ValueError(f"L and M must be in [1, 250] and [1, {SOLVE_MAX_MOVES}]")
    rows = np.asarray(rows)
    rows = (rows.view(np.uint16) if rows.dtype == np.int16 else rows.astype(np.uint16)).reshape(-1, 20)
    n = rows.shape[0]
    pieces = np.asarray(pieces)
    if pieces.ndim != 2 or pieces.shape[0] < 1 or pieces.shape[1] != M + 1:
        raise ValueError(f"pieces must be [n_cfg, {M + 1}] with n_cfg >= 1")
    pieces = pieces.astype(np.int64) & 7
    out = []
    for name, x, top in (("lines", lines, 255), ("moves", moves, 255), ("entry", entry, (1 << 32) - 1)):
        x = np.asarray(x)
        if x.shape != (n,) or not np.issubdtype(x.dtype, np.integer):
            raise ValueError(f"{name} must be {n} integers, one per node")
        x = x.astype(np.int64)
        if n and (x.min() < 0 or x.max() > top):
            raise ValueError(f"{name} must be in [0, {top}]")
        out.append(x)
    if n < 1:
        raise ValueError("rows must be [n, 20] with n >= 1")
    lines, moves, entry = out
    live = (lines < L) & (moves < M) & (entry < pieces.shape[0])
    return rows, lines, moves, entry, pieces, live


def _exact_arguments(weights, max_nodes, shortest, spare_weight) -> None:
    """What placement_exact refuses of the arguments that are no arrays of nodes, for a call that may search nothing."""
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or not 1 <= int(max_nodes) <= EXACT_MAX_NODES:
        raise ValueError(f"max_nodes must be an integer in [1, {EXACT_MAX_NODES}]")
    if not isinstance(shortest, (bool, np.bool_)):
        raise ValueError("shortest must be True or False")
    if np.asarray(weights, dtype=np.float32).reshape(-1).shape not in ((NUM_FEATURES,), (NUM_MOVE_FEATURES,)):
        raise ValueError("weights must be one row of 12 or of 14")
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(spare_weight)):
            raise ValueError("spare_weight must be finite (in float32)")


def placement_exact_nodes(rows, lines, moves, entry, pieces, L: int, M: int, weights, max_nodes: int, shortest: bool = True,
                          spare_weight: float = 0.0):
    """The rule of tpl_placement_exact_nodes (include/tpl_learn.h) for n nodes of the game (L, M): rows uint16 [n, 20], lines, moves and
    entry integers [n], pieces [n_cfg, M + 1] shared by the nodes, the rest placement_exact's.  Node i is searched as the configuration
    (rows[i], pieces[entry[i], moves[i]:]) of the game (L - lines[i], M - moves[i]).  Returns placement_exact's six arrays with
    solution_len and actions counted from the node, actions uint8 [n, M] padded with 255; a node with lines >= L, moves >= M or
    entry >= n_cfg is finished: solved = 0, proved = 1, bound = 0, nodes = 0."""
    rows, lines, moves, entry, pieces, live = _node_arrays(rows, lines, moves, entry, pieces, L, M)
    L, M, n = int(L), int(M), rows.shape[0]
    _exact_arguments(weights, max_nodes, shortest, spare_weight)
    solved, proved, length = np.zeros(n, np.uint8), np.ones(n, np.uint8), np.zeros(n, np.int32)
    actions, bound, nodes = np.full((n, M), NO_SECOND, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    for at_lines, at_moves in sorted({(int(a), int(b)) for a, b in zip(lines[live], moves[live])}):
        idx = np.flatnonzero(live & (lines == at_lines) & (moves == at_moves))
        got = placement_exact(rows[idx], pieces[entry[idx], at_moves:], L - at_lines, M - at_moves, weights, max_nodes, shortest,
                              spare_weight)
        solved[idx], proved[idx], length[idx], bound[idx], nodes[idx] = got[0], got[1], got[2], got[4], got[5]
        actions[idx, :M - at_moves] = got[3]
    return solved, proved, length, actions, bound, nodes


def placement_exact_labels(rows, lines, moves, entry, pieces, L: int, M: int, weights, max_nodes: int, spare_weight: float = 0.0):
    """The rule of tpl_placement_exact_labels (include/tpl_learn.h) for n nodes (placement_exact_nodes' arguments without `shortest`):
    every distinct placement b of a node's piece is played under (L, M) from the node's lines and moves, a dead child turned lost; a won
    child is LABEL_WIN at length 1, a lost one LABEL_LOSS, and a running one is what placement_exact_nodes (shortest, max_nodes for
    the child alone) says of it: solved -> LABEL_WIN at 1 + solution_len, proved without a win -> LABEL_LOSS, stopped -> LABEL_OPEN,
    which proves nothing.  Returns (label uint8 [n, 40], length int32 [n, 40], nodes uint32 [n, 40]); LABEL_NONE, 0, 0 where b is no
    distinct placement and for every b of a finished node."""
    rows, lines, moves, entry, pieces, live = _node_arrays(rows, lines, moves, entry, pieces, L, M)
    L, M, n = int(L), int(M), rows.shape[0]
    label, length = np.zeros((n, NUM_ACTIONS), np.uint8), np.zeros((n, NUM_ACTIONS), np.int32)
    nodes = np.zeros((n, NUM_ACTIONS), np.uint32)
    placements = [np.flatnonzero(canonical_actions(p, np.arange(NUM_ACTIONS)) == np.arange(NUM_ACTIONS)) for p in range(8)]
    at = np.flatnonzero(live)
    _exact_arguments(weights, max_nodes, True, spare_weight)
    if at.size == 0:
        return label, length, nodes
    cur = pieces[entry[at], moves[at]]
    sizes = [placements[p].size for p in cur]
    node = np.repeat(at, sizes)
    b = np.concatenate([placements[p] for p in cur])
    r2, _, l2, m2, s2 = host_moves(rows[node], np.repeat(cur, sizes), b // 10, b % 10, L, M, lines[node], moves[node])
    s2 = np.where(move_bound(r2, L, M, l2, m2, s2)["dead"], STATE_LOST_LIMIT, s2)
    label[node, b] = np.where(s2 == STATE_WON, LABEL_WIN, np.where(s2 == STATE_RUNNING, LABEL_OPEN, LABEL_LOSS))
    length[node, b] = s2 == STATE_WON
    run = np.flatnonzero(s2 == STATE_RUNNING)
    if run.size:
        solved, proved, sol_len, _, _, count = placement_exact_nodes(r2[run], l2[run], m2[run], entry[node[run]], pieces, L, M, weights,
                                                                     max_nodes, True, spare_weight)
        label[node[run], b[run]] = np.where(solved == 1, LABEL_WIN, np.where(proved == 1, LABEL_LOSS, LABEL_OPEN))
        length[node[run], b[run]] = np.where(solved == 1, 1 + sol_len, 0)
        nodes[node[run], b[run]] = count
    return label, length, nodes


def best_labelled_move(label, length) -> np.ndarray:
    """The lowest placement among the proved-winning ones of least length, uint8 [n]; 255 where no move is proved winning."""
    label, length = np.asarray(label), np.asarray(length).astype(np.int64)
    win = label == LABEL_WIN
    key = np.where(win, length, np.iinfo(np.int64).max)
    return np.where(win.any(axis=1), key.argmin(axis=1), NO_SECOND).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the exact search over a window
# The rule of tpl_placement_window_prove (include/tpl_learn.h) on the host, from the ROW form: the window is decoded, the boards are
# grouped by (lines, H), and each group is handed to placement_exact as configurations of the SHIFTED game (L - lines, H) whose lists
# are the window's first H entries; the verdict is derived from what comes back.  The device unpacks the planes and runs its own copy
# of the search (csrc/learn/exact_window.hip) -- the two share nothing.
WINDOW_PLAN = 12                                         # the plan's width: the window's twelve entries
WINDOW_NONE, WINDOW_WIN, WINDOW_LOSS, WINDOW_OPEN = 0, 1, 2, 3


def window_entries(window) -> np.ndarray:
    """The twelve 3-bit entries of 36-bit piece windows (window | window_hi << 32, entry j at bits 3 j): int64 [n, 12]."""
    window = np.asarray(window).astype(np.uint64).reshape(-1)
    return ((window[:, None] >> (np.uint64(3) * np.arange(WINDOW_PLAN, dtype=np.uint64))) & np.uint64(7)).astype(np.int64)


def _window_frame(rows, lines, moves, state, window, L: int, M: int, skip, search) -> dict:
    """The framing the two window mirrors share: the fields checked, live / known / rem / H, the dict in the C layout, the boards grouped
    by (lines, H), and the verdicts.  search(rows [k, 20], lists [k, H + 1], L - lines, H) -> the six arrays of an exact mirror for the
    group's configurations, shortest -- or the seven of a limited one, and then the dict holds limit int32 [n], 0 where nothing was
    searched."""
    rows = np.asarray(rows)
    rows = (rows.view(np.uint16) if rows.dtype == np.int16 else rows.astype(np.uint16)).reshape(-1, 20)
    n = rows.shape[0]
    if n < 1:
        raise ValueError("rows must be [n, 20] with n >= 1")
    fields = []
    for name, x, top in (("lines", lines, 255), ("moves", moves, 255), ("state", state, 3), ("window", window, (1 << 36) - 1)):
        x = np.asarray(x)
        if x.shape != (n,) or not np.issubdtype(x.dtype, np.integer):
            raise ValueError(f"{name} must be {n} integers, one per state")
        if x.min() < 0 or int(x.max()) > top:
            raise ValueError(f"{name} must be in [0, {top}]")
        fields.append(x.astype(np.uint64 if name == "window" else np.int64))
    lines, moves, state, window = fields
    if skip is None:
        skip = np.zeros(n, bool)
    else:
        skip = np.asarray(skip)
        if skip.shape != (n,):
            raise ValueError(f"skip must be None or {n} flags, one per state")
        skip = skip != 0
    q = window_entries(window)
    live = (state == STATE_RUNNING) & (lines < L) & (moves < M)
    known = (WINDOW_PLAN - moves % 10).astype(np.int64)
    rem = np.where(live, M - moves, 0)
    H = np.minimum(known, rem)
    out = dict(solved=np.zeros(n, np.uint8), proved=np.where(skip, 0, 1).astype(np.uint8), solution_len=np.zeros(n, np.int32),
               plan=np.full((n, WINDOW_PLAN), NO_SECOND, np.uint8), bound=np.zeros(n, np.int32), nodes=np.zeros(n, np.uint32),
               horizon=H.astype(np.uint8), verdict=np.zeros(n, np.uint8), known=known.astype(np.uint8))
    if live.any():
        at = np.flatnonzero(live)
        out["bound"][at] = move_bound(rows[at], L, M, lines[at], 0, STATE_RUNNING)["need"]
    todo = live & ~skip
    for at_lines, at_H in sorted({(int(a), int(b)) for a, b in zip(lines[todo], H[todo])}):
        idx = np.flatnonzero(todo & (lines == at_lines) & (H == at_H))
        lists = np.concatenate([q[idx, :at_H], np.zeros((idx.size, 1), np.int64)], axis=1)      # [k, H + 1]: the last is never placed
        solved, proved, length, actions, _, nodes, *limit = search(rows[idx], lists, L - at_lines, at_H)
        if limit:
            out.setdefault("limit", np.zeros(n, np.int32))[idx] = limit[0]
        out["solved"][idx], out["proved"][idx], out["solution_len"][idx], out["nodes"][idx] = solved, proved, length, nodes
        out["plan"][idx, :at_H] = actions
        out["verdict"][idx] = np.where(solved == 1, WINDOW_WIN,
                                       np.where((proved == 1) & (at_H == rem[idx]), WINDOW_LOSS, WINDOW_OPEN))
    return out


def placement_window_prove(rows, lines, moves, state, window, L: int, M: int, weights, max_nodes: int, spare_weight: float = 0.0,
                           skip=None) -> dict:
    """The rule of tpl_placement_window_prove (include/tpl_learn.h) for n states of the game (L, M) given by their fields: rows uint16
    [n, 20] (bit x = column x), lines, moves and state integers [n] (state 0 = running), window uint64 [n] (36 bits); one weight row
    [12] or [14], max_nodes in [1, 2^24], one finite spare_weight, skip None or [n] (nonzero: not searched).
    A running board with lines < L and moves < M has known = 12 - moves % 10, rem = M - moves and the horizon H = min(known, rem), and is
    searched as the configuration (rows, window entries 0 .. H - 1) of the game (L - lines, H), shortest; anything else is finished.
    Returns a dict in the C layout: solved, proved uint8 [n], solution_len int32 [n], plan uint8 [n, 12] padded with 255, bound int32
    [n], nodes uint32 [n], horizon uint8 [n], verdict uint8 [n] (WINDOW_NONE / WIN / LOSS / OPEN), and known uint8 [n]."""
    return _placement_window_prove(rows, lines, moves, state, window, L, M, weights, max_nodes, spare_weight, skip, None, 0)


def placement_window_prove_limited(rows, lines, moves, state, window, L: int, M: int, weights, max_nodes: int, first_limit: int = 0,
                                   growth: int = 0, spare_weight: float = 0.0, skip=None) -> dict:
    """The rule of tpl_placement_window_prove_limited (include/tpl_learn.h): placement_window_prove with the search of every board
    placement_exact_limited's.  Returns its dict with limit int32 [n], 0 where nothing was searched."""
    return _placement_window_prove(rows, lines, moves, state, window, L, M, weights, max_nodes, spare_weight, skip, first_limit, growth)


def _placement_window_prove(rows, lines, moves, state, window, L, M, weights, max_nodes, spare_weight, skip, first_limit, growth) -> dict:
    L, M = int(L), int(M)
    if not (1 <= L <= 250 and 1 <= M <= SOLVE_MAX_MOVES):
        raise ValueError(f"L and M must be in [1, 250] and [1, {SOLVE_MAX_MOVES}]")
    _exact_arguments(weights, max_nodes, True, spare_weight)
    _limit_arguments(first_limit, growth)
    out = _window_frame(rows, lines, moves, state, window, L, M, skip,
                        lambda r, p, game_L, H: _placement_exact(r, p, game_L, H, weights, max_nodes, True, spare_weight, first_limit,
                                                                 growth))
    if first_limit is not None:
        out.setdefault("limit", np.zeros(out["solved"].shape[0], np.int32))
    return out


# ------------------------------------------------------------------------------------------------ the n-tuple value function
# The table layout, the value and the update of include/tpl_learn.h on the host, from the ROW form of a board (uint16 [20], bit x =
# column x): the device works on column words with two shifts and a mask (csrc/learn/ntuple.hip) -- the two share nothing.
NTUPLE_PIECES, NTUPLE_TUPLES, NTUPLE_PATTERNS, NTUPLE_COUNTERS = 8, 153, 256, 1024
NTUPLE_COUNTER_BASE = NTUPLE_PIECES * NTUPLE_TUPLES * NTUPLE_PATTERNS                   # 313,344
NTUPLE_ENTRIES = NTUPLE_COUNTER_BASE + NTUPLE_COUNTERS                                   # 314,368
# the table shapes of include/tpl_learn.h: name -> (tuples, patterns, entries); NTUPLE_SHAPE_IDS gives the C `shape` of a name
NTUPLE_SHAPES = {"2x4": (153, 256, 314368), "3x3": (144, 512, 590848)}
NTUPLE_SHAPE_IDS = {"2x4": 0, "3x3": 1}
_WINDOWS = {"2x4": (2, 4), "3x3": (3, 3)}                  # (columns, rows) of a window
# the sums of shapes in one value: name -> the shapes of its parts, whose tables lie one behind the other in a SUM TABLE; a sum is
# no `shape` of the C interface (NTUPLE_SHAPE_IDS has none for it): the _sum entries read it, the updates take it part by part
NTUPLE_SUMS = {"2x4+3x3": ("2x4", "3x3")}
NTUPLE_ENTRIES_SUM = NTUPLE_SHAPES["2x4"][2] + NTUPLE_SHAPES["3x3"][2]                     # 905,216
NTUPLE_STEP_MAX = 1 << 24                                                               # |d| of one update is clamped to it
PIECE_PLACEMENTS = (17, 34, 34, 34, 17, 17, 9, 9)        # S: the distinct placements of each piece id (7 reads O's entry)


# Feature tuples (include/tpl_learn.h): tables indexed by the nine board features, alone or behind a 3 x 3 table.  A registry of their
# own -- name -> the C `form` of the _feature entries --, beside the shapes and sums above, which stay as they are
NTUPLE_FEATURE_FORMS = {"feat": 0, "3x3+feat": 1}
NTUPLE_FEATURES, NTUPLE_FEATURE_BINS = 9, 256
NTUPLE_ENTRIES_FEAT = NTUPLE_PIECES * NTUPLE_FEATURES * NTUPLE_FEATURE_BINS + NTUPLE_COUNTERS    # 19,456
_FEATURE_PARTS = {"feat": ("feat",), "3x3+feat": ("3x3", "feat")}
_PART_ENTRIES = {"2x4": NTUPLE_SHAPES["2x4"][2], "3x3": NTUPLE_SHAPES["3x3"][2], "feat": NTUPLE_ENTRIES_FEAT}
_PART_COLUMNS = {"2x4": 154, "3x3": 145, "feat": NTUPLE_FEATURES + 1}      # the columns of ntuple_indices, the counter's included
NTUPLE_ENTRIES_3X3_FEAT = _PART_ENTRIES["3x3"] + NTUPLE_ENTRIES_FEAT                             # 610,304

# The budget table (include/tpl_learn.h): a feature table with a tenth row per piece, read at the spare cells of the move bound.  A
# registry of its own again -- name -> the one form the _budget entries read --, beside the three above, which stay as they are
NTUPLE_BUDGET_FORMS = {"feat+spare": 0}
BUDGET = "feat+spare"
NTUPLE_BUDGET_ROWS = NTUPLE_FEATURES + 1                                                         # the nine feature rows, then spare
NTUPLE_ENTRIES_BUDGET = NTUPLE_PIECES * NTUPLE_BUDGET_ROWS * NTUPLE_FEATURE_BINS + NTUPLE_COUNTERS   # 21,504
_PART_ENTRIES[BUDGET] = NTUPLE_ENTRIES_BUDGET
_PART_COLUMNS[BUDGET] = NTUPLE_BUDGET_ROWS + 1


def _ntuple_shape(shape) -> str:
    known = (NTUPLE_SHAPES, NTUPLE_SUMS, NTUPLE_FEATURE_FORMS, NTUPLE_BUDGET_FORMS)
    if not isinstance(shape, str) or not any(shape in names for names in known):
        raise ValueError(f"shape must be one of {sum((sorted(names) for names in known), [])}, got {shape!r}")
    return shape


def _ntuple_feature_counts() -> dict:
    """Entry count -> name, for the feature forms."""
    return {ntuple_entries_of(name): name for name in NTUPLE_FEATURE_FORMS}


def _ntuple_budget_counts() -> dict:
    """Entry count -> name, for the budget table."""
    return {ntuple_entries_of(name): name for name in NTUPLE_BUDGET_FORMS}


def ntuple_parts_of(shape: str) -> tuple:
    """The shapes whose tables a table of `shape` consists of, in the order they lie in it: the shape itself, or a sum's parts."""
    if _ntuple_shape(shape) in NTUPLE_FEATURE_FORMS:
        return _FEATURE_PARTS[shape]
    return NTUPLE_SUMS.get(shape, (shape,))


def spare_bins(rows, L: int, M: int, lines, moves, state=0) -> np.ndarray:
    """sbin of K boards in row form (int64 [K]), the bin row 9 of a budget table is read at: 0 where the board is dead, else
    min(spare + 1, 255), dead and spare being move_bound's -- from the board's own lines and moves under the game's L and M.  A finished
    board has spare 0 and is not dead: bin 1."""
    bound = move_bound(rows, L, M, lines, moves, state)
    return np.where(bound["dead"], 0, np.minimum(bound["spare"] + 1, NTUPLE_FEATURE_BINS - 1)).astype(np.int64)


def ntuple_budget_bins(rows, L: int, M: int, lines, moves, state) -> np.ndarray:
    """tpl_ntuple_budget_bins on the host (uint8 [K, 10]): min(phi_j, 255) of board_features, then spare_bins, of K states, running or
    not."""
    rows = np.asarray(rows)
    rows = rows[None] if rows.ndim == 1 else rows
    phi = np.minimum(board_features(rows), NTUPLE_FEATURE_BINS - 1)
    return np.concatenate([phi, spare_bins(rows, L, M, lines, moves, state)[:, None]], axis=1).astype(np.uint8)


def ntuple_entries_of(shape: str) -> int:
    """The entries of a table of `shape`: a sum table holds its parts' tables whole, one behind the other."""
    return sum(_PART_ENTRIES[part] for part in ntuple_parts_of(shape))


def _ntuple_counts() -> dict:
    """Entry count -> name, for every shape and every sum."""
    return {ntuple_entries_of(name): name for name in list(NTUPLE_SHAPES) + list(NTUPLE_SUMS)}


def ntuple_shape_of(entries: int) -> str:
    """The shape (or sum of shapes) whose table has `entries` entries; anything else is refused."""
    counts = _ntuple_counts()
    if entries in counts:
        return counts[entries]
    if entries in _ntuple_feature_counts():
        return _ntuple_feature_counts()[entries]
    if entries in _ntuple_budget_counts():
        return _ntuple_budget_counts()[entries]
    counts = {**counts, **_ntuple_feature_counts(), **_ntuple_budget_counts()}
    raise ValueError(f"no table shape has {entries} entries: {({v: k for k, v in counts.items()})}")


def _counter_columns(shape: str) -> list:
    """The columns of ntuple_indices(shape=...) that hold a counter entry: the last one of every part."""
    columns, at = [], 0
    for part in ntuple_parts_of(shape):
        at += _PART_COLUMNS[part]
        columns.append(at - 1)
    return columns


# Staged tables (include/tpl_learn.h): NTUPLE_STAGES whole tables of a form -- a shape or a sum, NTUPLE_FORM_IDS gives the C `form` of
# a name -- one behind the other, then the stage map, an int32 per counter index; the stage of a state is map[k] & 7
NTUPLE_STAGES = 8
NTUPLE_FORM_IDS = {"2x4": 0, "3x3": 1, "2x4+3x3": 2}


def ntuple_staged_entries_of(shape: str) -> int:
    """The entries of a staged table of the form `shape`: eight tables and the 1,024 entries of the map."""
    return NTUPLE_STAGES * ntuple_entries_of(shape) + NTUPLE_COUNTERS


def _ntuple_staged_counts() -> dict:
    """Entry count -> the form's name, for the staged table of every shape and every sum."""
    return {ntuple_staged_entries_of(name): name for name in list(NTUPLE_SHAPES) + list(NTUPLE_SUMS)}


def ntuple_form_of(entries: int) -> tuple:
    """(the form's name, whether the table is staged) of a table of `entries` entries; anything else is refused."""
    staged = _ntuple_staged_counts()
    return (staged[entries], True) if entries in staged else (ntuple_shape_of(entries), False)


def ntuple_counter_index(L: int, M: int, lines, moves) -> np.ndarray:
    """k = 64 min(max(L - lines, 0), 15) + min(max(M - moves, 0), 63) (int64, the shape of lines against moves)."""
    lines, moves = np.asarray(lines, dtype=np.int64), np.asarray(moves, dtype=np.int64)
    return 64 * np.clip(int(L) - lines, 0, 15) + np.clip(int(M) - moves, 0, 63)


def ntuple_stage_map(L: int, M: int, lines: int = 1, moves: int = 4) -> np.ndarray:
    """A stage map (int32 [1,024]) that cuts (lines left, moves left) into a grid of `lines` x `moves` <= 8 buckets of equal width:
    entry k = 64 l + m, l < 16 and m < 64 the clamped counters, holds bl * moves + bm with bm = m * moves // (min(M, 63) + 1) and
    bl = l * lines // (min(L, 15) + 1).  Counters above min(L, 15) or min(M, 63), which no state of the game has, fall in the top
    bucket."""
    for name, v in (("L", L), ("M", M), ("lines", lines), ("moves", moves)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"{name} must be a positive integer, got {v!r}")
    if lines * moves > NTUPLE_STAGES:
        raise ValueError(f"lines * moves must be at most {NTUPLE_STAGES} stages, got {lines} x {moves}")
    l, m = np.divmod(np.arange(NTUPLE_COUNTERS, dtype=np.int64), 64)
    bl = np.minimum(l * lines // (min(int(L), 15) + 1), lines - 1)
    bm = np.minimum(m * moves // (min(int(M), 63) + 1), moves - 1)
    return (bl * moves + bm).astype(np.int32)


def ntuple_stages_of(table, L: int, M: int, lines, moves) -> np.ndarray:
    """The stage of K states under a staged table (or under a map of 1,024 entries alone): map[k] & 7 (int64 [K])."""
    table = np.asarray(table)
    stage_map = table[-NTUPLE_COUNTERS:]
    return (stage_map[ntuple_counter_index(L, M, lines, moves)].astype(np.int64) & (NTUPLE_STAGES - 1)).reshape(-1)


def ntuple_indices(rows, piece, L: int, M: int, lines, moves, shape: str = "2x4"):
    """Where the value of K boards lives in the table: (index int64 [K, 154], used bool [K, 154]).  Column t < 153 is tuple
    t = 17 x + y -- cell (row y + j, column x) is bit j and cell (row y + j, column x + 1) bit 4 + j of its pattern q, j < 4 --
    at index (piece * 153 + t) * 256 + q, used where q != 0; column 153 is the counter entry 313,344 + 64 min(max(L - lines, 0),
    15) + min(max(M - moves, 0), 63), always used.  rows: uint16 [K, 20] or [20] row masks (bit x = column x, row 0 = top).
    shape="3x3": [K, 145]; column t < 144 is tuple t = 18 x + y, x < 8 and y < 18 -- cell (row y + j, column x + i) is bit 3 i + j
    of q, i and j < 3 -- at index (piece * 144 + t) * 512 + q; column 144 is the counter entry 589,824 + the same k.
    shape="2x4+3x3", a sum table: [K, 154 + 145] -- the 2 x 4 columns, then the 3 x 3 columns with 314,368, the entry where the second
    part starts, added to every index; `used` likewise.  Both parts' counter columns are used.
    shape="feat", a feature table: [K, 10]; column j < 9 is feature j of board_features(rows) -- holes .. hole_depth -- at index
    (piece * 9 + j) * 256 + min(phi_j, 255); column 9 is the counter entry 18,432 + the same k; ALL ten are used.
    shape="3x3+feat": [K, 145 + 10] -- the 3 x 3 columns, then the feature columns with 590,848 added to every index.
    shape="feat+spare", a budget table: [K, 11]; column j < 9 is feature j at index (piece * 10 + j) * 256 + min(phi_j, 255), column 9
    the spare row at (piece * 10 + 9) * 256 + spare_bins(rows, L, M, lines, moves) -- of the board as a running one --, column 10 the
    counter entry 20,480 + the same k; ALL eleven are used."""
    if _ntuple_shape(shape) in NTUPLE_SUMS or shape == "3x3+feat":
        index, used, at = [], [], 0
        for part in ntuple_parts_of(shape):
            i, u = ntuple_indices(rows, piece, L, M, lines, moves, part)
            index.append(i + at)
            used.append(u)
            at += _PART_ENTRIES[part]
        return np.concatenate(index, axis=1), np.concatenate(used, axis=1)
    if shape == BUDGET:                                       # written from the row form: board_features and the move bound's mirror
        rows = np.asarray(rows)
        if rows.ndim == 1:
            rows = rows[None]
        phi = board_features(rows)
        k = rows.shape[0]
        piece, lines, moves = (np.broadcast_to(np.asarray(v, dtype=np.int64), (k,)) for v in (piece, lines, moves))
        if k and (piece.min() < 0 or piece.max() >= NTUPLE_PIECES):
            raise ValueError("piece must be in 0..7")
        bins = np.concatenate([np.minimum(phi, NTUPLE_FEATURE_BINS - 1), spare_bins(rows, L, M, lines, moves)[:, None]], axis=1)
        index = np.zeros((k, NTUPLE_BUDGET_ROWS + 1), dtype=np.int64)
        index[:, :NTUPLE_BUDGET_ROWS] = ((piece[:, None] * NTUPLE_BUDGET_ROWS + np.arange(NTUPLE_BUDGET_ROWS)[None, :]) * NTUPLE_FEATURE_BINS
                                         + bins)
        index[:, NTUPLE_BUDGET_ROWS] = NTUPLE_ENTRIES_BUDGET - NTUPLE_COUNTERS + ntuple_counter_index(L, M, lines, moves)
        return index, np.ones(index.shape, dtype=bool)
    if shape == "feat":
        rows = np.asarray(rows)
        if rows.ndim == 1:
            rows = rows[None]
        phi = board_features(rows)
        k = rows.shape[0]
        piece, lines, moves = (np.broadcast_to(np.asarray(v, dtype=np.int64), (k,)) for v in (piece, lines, moves))
        if k and (piece.min() < 0 or piece.max() >= NTUPLE_PIECES):
            raise ValueError("piece must be in 0..7")
        index = np.zeros((k, NTUPLE_FEATURES + 1), dtype=np.int64)
        index[:, :NTUPLE_FEATURES] = ((piece[:, None] * NTUPLE_FEATURES + np.arange(NTUPLE_FEATURES)[None, :]) * NTUPLE_FEATURE_BINS
                                      + np.minimum(phi, NTUPLE_FEATURE_BINS - 1))
        index[:, NTUPLE_FEATURES] = (NTUPLE_ENTRIES_FEAT - NTUPLE_COUNTERS + 64 * np.clip(int(L) - lines, 0, 15)
                                     + np.clip(int(M) - moves, 0, 63))
        return index, np.ones(index.shape, dtype=bool)
    tuples, patterns, entries = NTUPLE_SHAPES[shape]
    wide, high = _WINDOWS[shape]
    rows = np.asarray(rows)
    if rows.ndim == 1:
        rows = rows[None]
    if rows.ndim != 2 or rows.shape[1] != 20:
        raise ValueError("rows must be [K, 20] row masks")
    k = rows.shape[0]
    piece, lines, moves = (np.broadcast_to(np.asarray(v, dtype=np.int64), (k,)) for v in (piece, lines, moves))
    if k and (piece.min() < 0 or piece.max() >= NTUPLE_PIECES):
        raise ValueError("piece must be in 0..7")
    cell = (rows.astype(np.int64)[:, :, None] >> np.arange(10)[None, None, :]) & 1              # [K, 20, 10]
    index = np.zeros((k, tuples + 1), dtype=np.int64)
    used = np.ones((k, tuples + 1), dtype=bool)
    ys = 20 - high + 1
    for x in range(10 - wide + 1):
        for y in range(ys):
            q = np.zeros(k, dtype=np.int64)
            for i in range(wide):
                for j in range(high):
                    q |= cell[:, y + j, x + i] << (high * i + j)
            t = ys * x + y
            index[:, t] = (piece * tuples + t) * patterns + q
            used[:, t] = q != 0
    index[:, tuples] = (entries - NTUPLE_COUNTERS + 64 * np.clip(int(L) - lines, 0, 15) + np.clip(int(M) - moves, 0, 63))
    return index, used


def _ntuple_table(table, staged: bool = True) -> np.ndarray:
    """A table of a known entry count; staged=False: a plain one, for what has no staged form."""
    if (not isinstance(table, np.ndarray) or table.dtype != np.int32 or table.ndim != 1
            or (table.shape[0] not in _ntuple_counts() and table.shape[0] not in _ntuple_feature_counts()
                and table.shape[0] not in _ntuple_budget_counts()
                and not (staged and table.shape[0] in _ntuple_staged_counts()))):
        raise ValueError(f"table must be an int32 array of {NTUPLE_ENTRIES} entries (3x3: {NTUPLE_SHAPES['3x3'][2]}, "
                         f"2x4+3x3: {NTUPLE_ENTRIES_SUM}, feat: {NTUPLE_ENTRIES_FEAT}, 3x3+feat: {NTUPLE_ENTRIES_3X3_FEAT}, feat+spare: {NTUPLE_ENTRIES_BUDGET}" + (f"; staged: {list(_ntuple_staged_counts())})" if staged else
                                                             "); a staged table has no coherent update"))
    return table


def _table_shape(table) -> str:
    """The shape of a PLAIN table."""
    return ntuple_shape_of(_ntuple_table(table, staged=False).shape[0])


def _table_indices(table, rows, piece, L: int, M: int, lines, moves):
    """(index, used, the form's name) of K boards in `table`, plain or staged: ntuple_indices of the form, and under a staged table
    every index of a board moved into the block of its stage, stage * (the form's entries) further on."""
    shape, staged = ntuple_form_of(_ntuple_table(table).shape[0])
    index, used = ntuple_indices(rows, piece, L, M, lines, moves, shape)
    if staged:
        stage = np.broadcast_to(ntuple_stages_of(table, L, M, lines, moves), index.shape[:1])
        index = index + (stage * ntuple_entries_of(shape))[:, None]
    return index, used, shape


def ntuple_value(table, rows, piece, L: int, M: int, lines, moves, state) -> np.ndarray:
    """V of K states (float32 [K]): 0 where state != 0, else the entries ntuple_indices names summed exactly (int64), rounded
    once to float32 and scaled by 2^-16.  Under a sum table the entries of both parts are in that one sum: one rounding.  Under a
    staged table: the same sum over the block of the state's stage, map[k] & 7."""
    index, used, _ = _table_indices(table, rows, piece, L, M, lines, moves)
    total = np.where(used, table[index].astype(np.int64), 0).sum(axis=1)
    running = np.broadcast_to(np.asarray(state), total.shape) == 0
    return np.where(running, total.astype(np.float32) * np.float32(2.0 ** -16), np.float32(0.0)).astype(np.float32)


# The rule of tpl_ntuple_exact (include/tpl_learn.h) on the host: placement_exact's search with the children valued by a table, from
# the ROW form -- host_moves, move_bound and ntuple_value above.  The device ranks keys across a wave over packed boards in LDS and
# gathers from column words (csrc/learn/ntuple_exact.hip) -- the two share nothing.
NTUPLE_EXACT_FORMS = ("2x4", "3x3", "feat", "feat+spare")


def _ntuple_exact_table(table) -> np.ndarray:
    """A table of one of the four plain forms tpl_ntuple_exact reads; a sum or a staged table, or anything else, is refused."""
    counts = {ntuple_entries_of(name): name for name in NTUPLE_EXACT_FORMS}
    if not isinstance(table, np.ndarray) or table.dtype != np.int32 or table.ndim != 1 or table.shape[0] not in counts:
        sizes = ", ".join(f"{k} ({v!r})" for k, v in counts.items())
        raise ValueError(f"table must be an int32 array of {sizes} entries, one of the four plain forms: a sum or a staged table orders "
                         "no search")
    return table


def ntuple_exact(rows, pieces, L: int, M: int, table, max_nodes: int, shortest: bool = True, gamma: float = 1.0,
                 reward=(1.0, 0.0, 0.0)):
    """The rule of tpl_ntuple_exact (include/tpl_learn.h) for n configurations: placement_exact's arguments with a table (int32, one of
    NTUPLE_EXACT_FORMS by its entry count) for the weights and a finite gamma and reward = (r_line, r_win, r_lose) for spare_weight.  The
    search is placement_exact's (_exact_search); the child made at depth d is worth reward, or reward + gamma * V where it runs, V being
    ntuple_value of its board with pieces[d + 1] as the falling piece in the game (L, B) of the iteration -- float32 operations, each
    rounded once.  Returns placement_exact's six arrays."""
    return _ntuple_exact(rows, pieces, L, M, table, max_nodes, shortest, gamma, reward, None, 0)


def ntuple_exact_limited(rows, pieces, L: int, M: int, table, max_nodes: int, first_limit: int = 0, growth: int = 0,
                         shortest: bool = True, gamma: float = 1.0, reward=(1.0, 0.0, 0.0)):
    """The rule of tpl_ntuple_exact_limited (include/tpl_learn.h): ntuple_exact in limited-discrepancy order, first_limit and growth
    placement_exact_limited's.  Returns its seven arrays."""
    return _ntuple_exact(rows, pieces, L, M, table, max_nodes, shortest, gamma, reward, first_limit, growth)


def _ntuple_exact(rows, pieces, L, M, table, max_nodes, shortest, gamma, reward, first_limit, growth):
    L, M, max_nodes, rows, pieces = _exact_arrays(rows, pieces, L, M, max_nodes, shortest)
    _limit_arguments(first_limit, growth)
    table = _ntuple_exact_table(table)
    try:
        with np.errstate(over="ignore"):
            g = np.float32(gamma)
            r_line, r_win, r_lose = (np.float32(v) for v in reward)
    except (TypeError, ValueError):
        raise ValueError("gamma must be a number and reward three numbers (r_line, r_win, r_lose)") from None
    if not all(np.isfinite(v) for v in (g, r_line, r_win, r_lose)):
        raise ValueError("gamma and reward must be finite (in float32)")

    def children(tops, piece, nxt, b, L, B):                    # the table's order; nothing is kept along a path
        r2, cleared, l2, m2, s2 = host_moves(tops["rows"], piece, b // 10, b % 10, L, B, tops["lines"], tops["moves"])
        s2 = np.where(move_bound(r2, L, B, l2, m2, s2)["dead"], STATE_LOST_LIMIT, s2)
        with np.errstate(over="ignore", invalid="ignore"):
            r = r_line * cleared.astype(np.float32)
            r = np.where(s2 == STATE_WON, r + r_win, r)
            r = np.where(s2 >= STATE_LOST_LIMIT, r + r_lose, r).astype(np.float32)
            v = ntuple_value(table, r2, nxt, L, B, l2, m2, s2)
            value = np.where(s2 == STATE_RUNNING, r + g * v, r).astype(np.float32)
        return value, s2, r2, l2, m2, None

    return _exact_search(rows, pieces, L, M, max_nodes, bool(shortest), children, first_limit, int(growth))


# The rule of tpl_ntuple_window_prove (include/tpl_learn.h) on the host: placement_window_prove's framing (_window_frame, shared) with
# ntuple_exact for placement_exact, from the ROW form.  The device unpacks the planes and runs its own copy of the search
# (csrc/learn/ntuple_window.hip) -- the two share nothing.
def ntuple_window_prove(rows, lines, moves, state, window, L: int, M: int, table, max_nodes: int, gamma: float = 1.0,
                        reward=(1.0, 0.0, 0.0), skip=None) -> dict:
    """The rule of tpl_ntuple_window_prove (include/tpl_learn.h) for n states of the game (L, M): placement_window_prove's fields and
    skip mask, with ntuple_exact's table (int32, one of NTUPLE_EXACT_FORMS by its entry count), gamma and reward = (r_line, r_win,
    r_lose) for the weights and spare_weight.  A running board with lines < L and moves < M is searched as the configuration (rows,
    [window entries 0 .. H - 1, 0]) of the game (L - lines, H) by ntuple_exact, shortest; anything else is finished.
    Returns placement_window_prove's dict, `known` included."""
    return _ntuple_window_prove(rows, lines, moves, state, window, L, M, table, max_nodes, gamma, reward, skip, None, 0)


def ntuple_window_prove_limited(rows, lines, moves, state, window, L: int, M: int, table, max_nodes: int, first_limit: int = 0,
                                growth: int = 0, gamma: float = 1.0, reward=(1.0, 0.0, 0.0), skip=None) -> dict:
    """The rule of tpl_ntuple_window_prove_limited (include/tpl_learn.h): ntuple_window_prove with the search of every board
    ntuple_exact_limited's.  Returns its dict with limit int32 [n], 0 where nothing was searched."""
    return _ntuple_window_prove(rows, lines, moves, state, window, L, M, table, max_nodes, gamma, reward, skip, first_limit, growth)


def _ntuple_window_prove(rows, lines, moves, state, window, L, M, table, max_nodes, gamma, reward, skip, first_limit, growth) -> dict:
    L, M = int(L), int(M)
    if not (1 <= L <= 250 and 1 <= M <= SOLVE_MAX_MOVES):
        raise ValueError(f"L and M must be in [1, 250] and [1, {SOLVE_MAX_MOVES}]")
    if isinstance(max_nodes, bool) or not isinstance(max_nodes, (int, np.integer)) or not 1 <= int(max_nodes) <= EXACT_MAX_NODES:
        raise ValueError(f"max_nodes must be an integer in [1, {EXACT_MAX_NODES}]")
    max_nodes = int(max_nodes)
    table = _ntuple_exact_table(table)
    try:
        with np.errstate(over="ignore"):
            values = [np.float32(gamma)] + [np.float32(v) for v in reward]
    except (TypeError, ValueError):
        raise ValueError("gamma must be a number and reward three numbers (r_line, r_win, r_lose)") from None
    if len(values) != 4 or not all(np.isfinite(v) for v in values):
        raise ValueError("gamma and reward = (r_line, r_win, r_lose) must be finite (in float32)")
    _limit_arguments(first_limit, growth)
    out = _window_frame(rows, lines, moves, state, window, L, M, skip,
                        lambda r, p, game_L, H: _ntuple_exact(r, p, game_L, H, table, max_nodes, True, gamma, reward, first_limit, growth))
    if first_limit is not None:
        out.setdefault("limit", np.zeros(out["solved"].shape[0], np.int32))
    return out


def ntuple_steps(error, rate) -> np.ndarray:
    """d = (int32) rint(rate * e): the float32 product rounded once, clamped to +-2^24, 0 for a NaN (int64 [K])."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.float32(rate) * np.asarray(error, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0.0), np.clip(x, -float(NTUPLE_STEP_MAX), float(NTUPLE_STEP_MAX)))
    return np.rint(x).astype(np.int64)


def ntuple_update(table, rows, piece, L: int, M: int, lines, moves, state, error, rate) -> np.ndarray:
    """tpl_ntuple_update, in place: every running state adds its d to the entries ntuple_indices names; the adds wrap.  A sum
    table takes d on the entries of both parts: tpl_ntuple_update_shaped once per part with the same errors.  A staged table
    takes d in the block of the state's stage (tpl_ntuple_update_trace_staged on a ring of one slot); its map is only read."""
    index, used, _ = _table_indices(table, rows, piece, L, M, lines, moves)
    d = np.where(np.broadcast_to(np.asarray(state), index.shape[:1]) == 0, ntuple_steps(error, rate), 0)
    used = used & (d != 0)[:, None]
    np.add.at(_ntuple_table(table).view(np.uint32), index[used], np.broadcast_to(d[:, None], used.shape)[used].astype(np.uint32))
    return table


NTUPLE_TRACE_MAX = 16                                    # the horizon of tpl_ntuple_update_trace is at most this


def _reflected_rows(rows) -> np.ndarray:
    """Row masks with their ten columns reversed: bit x -> bit 9 - x."""
    rows = np.asarray(rows).astype(np.int64)
    out = np.zeros_like(rows)
    for x in range(10):
        out |= ((rows >> x) & 1) << (9 - x)
    return out.astype(np.uint16)


_sigma_of = {}                                          # ntuple_mirror_permutation's results, one per shape


def ntuple_mirror_permutation(shape: str = "2x4") -> np.ndarray:
    """shape="2x4+3x3": each part's sigma, the second offset by where its part starts.  Otherwise:
    sigma (int64 [entries of the shape]): the index of tuple[p][17 x + y][q] -> that of tuple[pi(p)][17 (8 - x) + y][swap(q)],
    with pi = PIECE_MIRROR and swap(q) = (q >> 4) | ((q & 15) << 4) (3x3: 18 (7 - x) + y, and swap exchanges bits 0..2 with bits
    6..8); the counter indices stay.  A table is mirror-symmetric when table[sigma] == table.
    Built from its definition, not from that closed form: every tuple entry (p, t, q) is put on a board as the cells of its
    window, and its image is the index ntuple_indices gives the reflected rows under pi(p) at the reflected window.
    shape="feat" (and the feature part of "3x3+feat") IS a closed form: feature[p][j][q] -> feature[pi(p)][j][q], the counters stay.
    An entry of a feature table is no set of cells that could be laid on a board and reflected; that the image keeps j and q rests
    on the nine features being invariant under reflection, which the tests check on the 8,192 boards of random_moves.npz, and the
    closed form is held to the definition by the symmetric update, which goes through the reflected rows and not through sigma.
    shape="feat+spare": the same closed form over ten rows a piece -- a row's fill, and with it spare, does not change under reflection."""
    if _ntuple_shape(shape) in NTUPLE_SUMS or shape == "3x3+feat":
        parts, at = [], 0
        for part in ntuple_parts_of(shape):
            parts.append(ntuple_mirror_permutation(part) + at)
            at += _PART_ENTRIES[part]
        return np.concatenate(parts)
    if shape in ("feat", BUDGET):                             # the features, and spare, are reflection-invariant: only the piece moves
        sigma = np.arange(_PART_ENTRIES[shape], dtype=np.int64)
        stride = (_PART_COLUMNS[shape] - 1) * NTUPLE_FEATURE_BINS
        for p in range(NTUPLE_PIECES):
            sigma[p * stride:(p + 1) * stride] = PIECE_MIRROR[p] * stride + np.arange(stride)
        return sigma
    tuples, patterns, entries = NTUPLE_SHAPES[shape]
    if shape in _sigma_of:
        return _sigma_of[shape].copy()
    wide, high = _WINDOWS[shape]
    xs, ys = 10 - wide + 1, 20 - high + 1
    sigma = np.arange(entries, dtype=np.int64)
    q = np.arange(patterns, dtype=np.int64)
    pi = np.array(PIECE_MIRROR)
    for x in range(xs):
        rows = np.zeros((ys, patterns, 20), dtype=np.int64)              # pattern q laid out in window (x, y) of an empty board
        for y in range(ys):
            for i in range(wide):
                for j in range(high):
                    rows[y, :, y + j] |= ((q >> (high * i + j)) & 1) << (x + i)
        image, _ = ntuple_indices(_reflected_rows(rows.reshape(-1, 20)), 0, 1, 1, 0, 0, shape)
        for y in range(ys):
            t, image_t = ys * x + y, ys * (xs - 1 - x) + y
            image_q = image[y * patterns:(y + 1) * patterns, image_t] - image_t * patterns    # piece 0: the tuple's row, then q
            for p in range(NTUPLE_PIECES):
                sigma[(p * tuples + t) * patterns + q] = (pi[p] * tuples + image_t) * patterns + image_q
    _sigma_of[shape] = sigma.copy()
    return sigma


def ntuple_update_trace(table, ages, L: int, M: int, error, rate, decay, symmetric) -> np.ndarray:
    """tpl_ntuple_update_trace, in place.  `ages`: a list, newest first, of (rows, piece, lines, moves, state) -- the decoded
    fields ntuple_update takes, K states each.  Board i takes d_k = ntuple_steps(e_i, float32(rate) * w_k), w_0 = 1 and w_k =
    float32(w_{k-1} * decay), at age k as long as that state and every younger one run.  symmetric: the same d_k goes to the tuple
    entries of the REFLECTED rows (columns reversed, piece through PIECE_MIRROR) as well -- not through sigma --; the counter is
    added once.  A staged table (tpl_ntuple_update_trace_staged): every add of a state, the reflected board's included, goes to the
    block of THAT state's stage; the map is read as it stands and never written."""
    tab, shape = _ntuple_table(table).view(np.uint32), ntuple_form_of(table.shape[0])[0]
    counters = _counter_columns(shape)
    e = np.asarray(error, dtype=np.float32).reshape(-1)
    open_ = np.ones(e.shape, dtype=bool)
    w, decay = np.float32(1.0), np.float32(decay)
    for age, (rows, piece, lines, moves, state) in enumerate(ages):
        if age:
            w = np.float32(w * decay)
        open_ = open_ & (np.broadcast_to(np.asarray(state), e.shape) == 0)
        d = np.where(open_, ntuple_steps(e, np.float32(rate) * w), 0)
        index, used, _ = _table_indices(table, rows, piece, L, M, lines, moves)
        used = used & (d != 0)[:, None]
        np.add.at(tab, index[used], np.broadcast_to(d[:, None], used.shape)[used].astype(np.uint32))
        if symmetric:
            piece = np.broadcast_to(np.asarray(piece, dtype=np.int64), e.shape)
            index, used, _ = _table_indices(table, _reflected_rows(rows), np.array(PIECE_MIRROR)[piece], L, M, lines, moves)
            used = used & (d != 0)[:, None]
            used[:, counters] = False             # the counter (of a sum table: each part's) was added above, once
            np.add.at(tab, index[used], np.broadcast_to(d[:, None], used.shape)[used].astype(np.uint32))
    return table


def _ntuple_coherence(coherence, entries=None) -> np.ndarray:
    """An int64 [entries, 2] buffer of a shape's entry count -- of `entries`, where a table says which."""
    if (not isinstance(coherence, np.ndarray) or coherence.dtype != np.int64 or coherence.ndim != 2 or coherence.shape[1] != 2
            or coherence.shape[0] not in (list(_ntuple_counts()) if entries is None else [entries])):
        raise ValueError(f"coherence must be an int64 array of shape ({NTUPLE_ENTRIES if entries is None else entries}, 2)")
    return coherence


def ntuple_step_sizes(coherence) -> np.ndarray:
    """alpha of every entry (float32 [the buffer's entries]) from its pair (E, A): 1 where A <= 0, else min(float32(|E|) / float32(A), 1)
    -- |E| as an unsigned 64-bit value, both conversions to nearest even, the float32 quotient rounded once."""
    c = _ntuple_coherence(coherence)
    e, a = c[:, 0], c[:, 1]
    mag = np.where(e < 0, np.uint64(0) - e.view(np.uint64), e.view(np.uint64)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.minimum(mag / a.astype(np.float32), np.float32(1.0))
    return np.where(a <= 0, np.float32(1.0), ratio).astype(np.float32)


def ntuple_coherent_steps(error, rate, alpha) -> np.ndarray:
    """s = (int32) rint((rate * alpha) * e) (int64, the shape of alpha against e): ntuple_steps with rate * alpha, a float32 product
    rounded once, as its rate."""
    with np.errstate(over="ignore", invalid="ignore"):
        x = (np.float32(rate) * np.asarray(alpha, dtype=np.float32)) * np.asarray(error, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0.0), np.clip(x, -float(NTUPLE_STEP_MAX), float(NTUPLE_STEP_MAX)))
    return np.rint(x).astype(np.int64)


def ntuple_update_coherent(table, coherence, ages, L: int, M: int, error, rate, decay, symmetric):
    """tpl_ntuple_update_coherent, in place on both buffers: (table, coherence).  `ages` as ntuple_update_trace takes them.  Every
    alpha is read from `coherence` as it stands at the call; entry j of a board at age k whose trace is open and whose d_k is not 0
    takes s = ntuple_coherent_steps(e, float32(rate) * w_k, alpha_j) on the table, d_k on E_j and |d_k| on A_j, all wrapping."""
    tab, shape = _ntuple_table(table).view(np.uint32), _table_shape(table)
    counters = _counter_columns(shape)
    sums = _ntuple_coherence(coherence, table.shape[0]).view(np.uint64)
    alpha = ntuple_step_sizes(coherence)                 # before any add of this call
    e = np.asarray(error, dtype=np.float32).reshape(-1)
    open_ = np.ones(e.shape, dtype=bool)
    w, decay = np.float32(1.0), np.float32(decay)
    for age, (rows, piece, lines, moves, state) in enumerate(ages):
        if age:
            w = np.float32(w * decay)
        open_ = open_ & (np.broadcast_to(np.asarray(state), e.shape) == 0)
        r = np.float32(rate) * w
        d = np.where(open_, ntuple_steps(e, r), 0)
        piece = np.broadcast_to(np.asarray(piece, dtype=np.int64), e.shape)
        forms = [(rows, piece, True)] + ([(_reflected_rows(rows), np.array(PIECE_MIRROR)[piece], False)] if symmetric else [])
        for form_rows, form_piece, counter in forms:
            index, used = ntuple_indices(form_rows, form_piece, L, M, lines, moves, shape)
            used = used & (d != 0)[:, None]
            used[:, counters] &= counter          # the counter (each part's) is taken once, with the state's own entries
            j = index[used]
            d_j = np.broadcast_to(d[:, None], used.shape)[used]
            s_j = ntuple_coherent_steps(np.broadcast_to(e[:, None], used.shape)[used], r, alpha[j])
            np.add.at(tab, j, s_j.astype(np.uint32))
            np.add.at(sums[:, 0], j, d_j.astype(np.uint64))
            np.add.at(sums[:, 1], j, np.abs(d_j).astype(np.uint64))
    return table, coherence


def ntuple_explore(seed: int, step: int, n: int, epsilon: float, placements):
    """The exploration draw of tpl_ntuple_act for boards 0 .. n - 1: (explores bool [n], j int64 [n]) -- a RUNNING board i explores
    iff (h_i >> 40) < (uint32)(epsilon * 2^24) and then plays the j-th of its `placements` (S, int [n] or a number) distinct
    placements in ascending order, j = ((h_i & 0xFFFFFFFF) * S) >> 32; h = _draw_hashes(seed, step, n)."""
    h = _draw_hashes(seed, step, n)
    below = np.uint64(int(np.float32(epsilon) * np.float32(2.0 ** 24)))
    s = np.broadcast_to(np.asarray(placements, dtype=np.uint64), (n,))
    return (h >> np.uint64(40)) < below, (((h & _M32) * s) >> np.uint64(32)).astype(np.int64)


def _lowest_at_max(x, axis):
    """(the entry at the lowest index that holds the maximum along `axis` -- its own bits: -0 and +0 tie --, that index); -inf
    marks what does not take part."""
    x = np.asarray(x, dtype=np.float32)
    at = np.argmax(x == x.max(axis=axis, keepdims=True), axis=axis)            # == : -0 and +0 are equal
    return np.take_along_axis(x, np.expand_dims(at, axis), axis=axis).squeeze(axis), at


# The rule of tpl_ntuple_rank (include/tpl_learn.h) on the host, from the ROW form: host_moves, canonical_actions, move_bound and
# ntuple_value above, the arg-max by _lowest_at_max.  The device scores a (board, action) pair a lane and takes three 64-bit maxima in
# LDS (csrc/learn/ntuple_rank.hip) -- the two share nothing.
NTUPLE_RANK_FORMS = NTUPLE_EXACT_FORMS
RANK_UNDECIDED = 255
RANK_OUTPUTS = ("win", "loss", "greedy", "violated", "gap", "err_win", "err_loss", "win_rows", "win_fields", "loss_rows", "loss_fields")


def _rank_table(table) -> np.ndarray:
    """A table of one of the four plain forms tpl_ntuple_rank reads; a sum or a staged table, or anything else, is refused."""
    counts = {ntuple_entries_of(name): name for name in NTUPLE_RANK_FORMS}
    if not isinstance(table, np.ndarray) or table.dtype != np.int32 or table.ndim != 1 or table.shape[0] not in counts:
        sizes = ", ".join(f"{k} ({v!r})" for k, v in counts.items())
        raise ValueError(f"table must be an int32 array of {sizes} entries, one of the four plain forms: a sum or a staged table is "
                         "taught no ranking")
    return table


def _rank_numbers(gamma, reward, margin, prune, table):
    try:
        with np.errstate(over="ignore"):
            g, m = np.float32(gamma), np.float32(margin)
            r_line, r_win, r_lose = (np.float32(v) for v in reward)
    except (TypeError, ValueError):
        raise ValueError("gamma and margin must be numbers and reward three numbers (r_line, r_win, r_lose)") from None
    if not all(np.isfinite(v) for v in (g, m, r_line, r_win, r_lose)):
        raise ValueError("gamma, margin and reward must be finite (in float32)")
    if not isinstance(prune, (bool, np.bool_)):
        raise ValueError("prune must be True or False")
    if prune and table.shape[0] != NTUPLE_ENTRIES_BUDGET:
        raise ValueError('prune=True is the dead-board prune of a budget table ("feat+spare") alone')
    return g, m, (r_line, r_win, r_lose)


def ntuple_rank(table, rows, piece, L: int, M: int, lines, moves, state, label, gamma, reward, margin, prune) -> dict:
    """The rule of tpl_ntuple_rank (include/tpl_learn.h) for K states in row form: rows uint16 [K, 20], piece int [K, 2] -- the falling
    piece and the one behind it, window entries 0 and 1 --, lines, moves and state [K], label uint8 [K, 40]; table an int32 array of one
    of NTUPLE_RANK_FORMS; gamma, margin and reward = (r_line, r_win, r_lose) finite; prune a bool, True under a "feat+spare" table only.
    Returns a dict of RANK_OUTPUTS: win, loss, greedy, violated uint8 [K]; gap, err_win, err_loss float32 [K]; and the two afterstates
    in row form, win_rows / loss_rows uint16 [K, 20] and win_fields / loss_fields int64 [K, 3] = (lines, moves, state) -- the state itself
    where the node is undecided; the falling piece of a decided afterstate is piece[:, 1]."""
    table = _rank_table(table)
    L, M = int(L), int(M)
    if not (1 <= L <= 250 and 1 <= M <= 254):
        raise ValueError("L and M must be in [1, 250] and [1, 254]")
    g, margin, (r_line, r_win, r_lose) = _rank_numbers(gamma, reward, margin, prune, table)
    rows = np.asarray(rows)
    rows = (rows.view(np.uint16) if rows.dtype == np.int16 else rows.astype(np.uint16)).reshape(-1, 20)
    k = rows.shape[0]
    piece = np.asarray(piece).astype(np.int64) & 7
    label = np.asarray(label)
    if k < 1 or piece.shape != (k, 2) or label.shape != (k, NUM_ACTIONS) or label.dtype != np.uint8:
        raise ValueError("rows must be [K, 20], piece [K, 2] and label uint8 [K, 40] with K >= 1")
    lines, moves, state = (np.broadcast_to(np.asarray(x).astype(np.int64), (k,)) for x in (lines, moves, state))
    running = state == STATE_RUNNING
    acts = np.arange(NUM_ACTIONS)
    distinct = canonical_actions(piece[:, :1], acts[None, :]) == acts[None, :]
    # every distinct placement of every running board, played once
    node, a = np.nonzero(distinct & running[:, None])
    score = np.zeros((k, NUM_ACTIONS), np.float32)                          # a finished board scores 0
    valued = np.zeros((k, NUM_ACTIONS), bool)
    child_rows = np.repeat(rows[:, None, :], NUM_ACTIONS, axis=1)
    child = np.repeat(np.stack([lines, moves, state], axis=1)[:, None, :], NUM_ACTIONS, axis=1)
    if node.size:
        r2, cleared, l2, m2, s2 = host_moves(rows[node], piece[node, 0], a // 10, a % 10, L, M, lines[node], moves[node])
        scored = np.where(move_bound(r2, L, M, l2, m2, s2)["dead"], STATE_LOST_LIMIT, s2) if prune else s2
        with np.errstate(over="ignore", invalid="ignore"):
            r = r_line * cleared.astype(np.float32)
            r = np.where(scored == STATE_WON, r + r_win, r)
            r = np.where(scored >= STATE_LOST_LIMIT, r + r_lose, r).astype(np.float32)
            v = ntuple_value(table, r2, piece[node, 1], L, M, l2, m2, scored)
            score[node, a] = np.where(scored == STATE_RUNNING, r + g * v, r).astype(np.float32)
        valued[node, a] = scored == STATE_RUNNING
        child_rows[node, a] = r2
        child[node, a] = np.stack([l2, m2, s2], axis=1)                     # the true board, also under the prune
    wins = distinct & running[:, None] & (label == 1)
    losses = distinct & running[:, None] & (label == 2)
    decided = wins.any(axis=1) & losses.any(axis=1)
    at = np.arange(k)
    masked = lambda m: np.where(m, score, -np.inf).astype(np.float32)
    _, greedy = _lowest_at_max(masked(distinct), 1)
    s_win, win = _lowest_at_max(masked(wins), 1)
    s_loss, loss = _lowest_at_max(masked(losses), 1)
    with np.errstate(invalid="ignore", over="ignore"):
        zero = np.float32(0.0)
        gap = (np.where(decided, s_win, zero).astype(np.float32) - np.where(decided, s_loss, zero).astype(np.float32)).astype(np.float32)
        violated = decided & (gap <= margin)
    out = dict(win=np.where(decided, win, RANK_UNDECIDED).astype(np.uint8), loss=np.where(decided, loss, RANK_UNDECIDED).astype(np.uint8),
               greedy=greedy.astype(np.uint8), violated=violated.astype(np.uint8), gap=gap,
               err_win=np.where(violated & valued[at, win], np.float32(1.0), np.float32(0.0)).astype(np.float32),
               err_loss=np.where(violated & valued[at, loss], np.float32(-1.0), np.float32(0.0)).astype(np.float32))
    own = np.stack([lines, moves, state], axis=1)
    for side, b in (("win", win), ("loss", loss)):
        out[side + "_rows"] = np.where(decided[:, None], child_rows[at, b], rows).astype(np.uint16)
        out[side + "_fields"] = np.where(decided[:, None], child[at, b], own).astype(np.int64)
    return out


def ntuple_rank_step(table, rows, piece, L: int, M: int, lines, moves, state, label, gamma, reward, margin, prune, rate,
                     symmetric: bool = False) -> dict:
    """One teaching step, in place on `table`: ntuple_rank, then ntuple_update_trace twice on a ring of one slot -- the win afterstates
    with err_win, then the loss afterstates with err_loss, each adding rint(rate * err) to its entries (symmetric: to the reflected
    board's as well).  Returns ntuple_rank's dict, taken BEFORE the adds."""
    out = ntuple_rank(table, rows, piece, L, M, lines, moves, state, label, gamma, reward, margin, prune)
    piece = np.asarray(piece).astype(np.int64) & 7
    falling = np.where(out["win"] == RANK_UNDECIDED, piece[:, 0], piece[:, 1])      # an undecided node's afterstate is the state itself
    for side in ("win", "loss"):
        f = out[side + "_fields"]
        ntuple_update_trace(table, [(out[side + "_rows"], falling, f[:, 0], f[:, 1], f[:, 2])], L, M, out["err_" + side], rate, 1.0,
                            symmetric)
    return out


def rank_fit_order(count: int, epochs: int, seed: int) -> np.ndarray:
    """The order in which `fit` visits `count` nodes: int64 [epochs, count], one permutation an epoch from numpy's default generator
    seeded with `seed` -- the one order of NTupleRanker.fit and of its mirror below."""
    gen = np.random.default_rng(int(seed))
    return np.stack([gen.permutation(int(count)) for _ in range(int(epochs))]).astype(np.int64).reshape(int(epochs), int(count))


def ntuple_rank_fit(table, rows, piece, L: int, M: int, lines, moves, state, label, gamma, reward, margin, prune, rate,
                    symmetric: bool, epochs: int, batch: int, seed: int = 0) -> list:
    """NTupleRanker.fit on the host, in place on `table`: every epoch walks the nodes in rank_fit_order's permutation, `batch` at a time
    (the last minibatch may be short), one ntuple_rank_step each; returns the violated count of every epoch -- each node counted when
    its minibatch was ranked, before that minibatch's adds."""
    rows, piece, label = np.asarray(rows), np.asarray(piece), np.asarray(label)
    lines, moves, state = (np.asarray(x) for x in (lines, moves, state))
    counts = []
    for order in rank_fit_order(rows.shape[0], epochs, seed):
        total = 0
        for lo in range(0, order.size, int(batch)):
            pick = order[lo:lo + int(batch)]
            out = ntuple_rank_step(table, rows[pick], piece[pick], L, M, lines[pick], moves[pick], state[pick], label[pick], gamma, reward,
                                   margin, prune, rate, symmetric)
            total += int(out["violated"].sum())
        counts.append(total)
    return counts


def ntuple_search_choice(reward1, done1, distinct1, reward2, done2, value2, distinct2, gamma, running=None):
    """The two-ply rule of include/tpl_learn.h (tpl_ntuple_search) on rewards and values that are given: reward1 f32 [K, 40] and
    done1 [K, 40] of every first placement a; reward2 f32, done2 and value2 f32 [K, 40, 40] of every (a, b) -- read only where
    done1 is not set; value2 = V(s_ab), read only where done2 is not set --; distinct1 [K, 40] where a is a distinct placement of
    the current piece, distinct2 [K, 40] or [K, 40, 40] where b is one of the next piece; running [K] (default: all) where the
    state is in play.  Returns (action u8 [K], second u8 [K], score f32 [K], Q f32 [K, 40], second of every a u8 [K, 40]):
    q(a, b) = r2, or r2 + gamma * V where the game goes on; W(a) = the maximum over the distinct b, second(a) the lowest b at
    it; Q(a) = r1 where done1 (second 255), else r1 + gamma * W(a); action = the lowest distinct a at the maximum of Q; a state
    that is not running gets action 0, second 255, score 0 and Q = 0.  Float32 numpy operations: every product and every sum
    rounded once; -0 and +0 tie."""
    reward1, reward2, value2 = (np.asarray(x, dtype=np.float32) for x in (reward1, reward2, value2))
    k = reward1.shape[0]
    done1, distinct1, done2, distinct2 = (np.asarray(x).astype(bool) for x in (done1, distinct1, done2, distinct2))
    if distinct2.ndim == 2:
        distinct2 = np.broadcast_to(distinct2[:, None, :], (k, NUM_ACTIONS, NUM_ACTIONS))
    pairs = (k, NUM_ACTIONS)
    if reward1.shape != pairs or done1.shape != pairs or distinct1.shape != pairs:
        raise ValueError("reward1, done1 and distinct1 must be [K, 40]")
    if any(x.shape != pairs + (NUM_ACTIONS,) for x in (reward2, done2, value2, distinct2)):
        raise ValueError("reward2, done2 and value2 must be [K, 40, 40] and distinct2 [K, 40] or [K, 40, 40]")
    running = np.ones(k, dtype=bool) if running is None else np.asarray(running).astype(bool).reshape(k)
    g = np.float32(gamma)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.where(done2, reward2, reward2 + g * value2)
        w, second = _lowest_at_max(np.where(distinct2, q, -np.inf), axis=2)
        w = np.where(done1, np.float32(0.0), w)                # not read there; keeps -inf out of the product
        Q = np.where(done1, reward1, reward1 + g * w)
    Q = np.where(running[:, None], Q, np.float32(0.0)).astype(np.float32)
    second = np.where(done1 | ~running[:, None], NO_SECOND, second).astype(np.uint8)
    score, action = _lowest_at_max(np.where(distinct1, Q, -np.inf), axis=1)
    action = np.where(running, action, 0)
    at = np.arange(k)
    return action.astype(np.uint8), second[at, action], Q[at, action], Q, second


def ntuple_beam_values(rewards, ended, leaf_value, gamma) -> np.ndarray:
    """The fold of include/tpl_learn.h (tpl_ntuple_beam) for K children at ply j: rewards f32 [K, j] = r_1 .. r_j of each path,
    ended [K] where the child does not run, leaf_value f32 [K] = V(child), read only where it runs.  tail_j = r_j, or
    r_j + gamma * V where the child runs; tail_k = r_k + gamma * tail_{k+1} for k = j - 1 .. 1; returns tail_1 (float32 [K]).
    Float32 numpy operations from the leaf inwards: every product and every sum rounded once."""
    r = np.asarray(rewards, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] < 1:
        raise ValueError("rewards must be [K, j] with j >= 1")
    ended = np.asarray(ended).astype(bool).reshape(r.shape[0])
    v = np.asarray(leaf_value, dtype=np.float32).reshape(r.shape[0])
    g = np.float32(gamma)
    with np.errstate(invalid="ignore", over="ignore"):
        tail = np.where(ended, r[:, -1], r[:, -1] + g * np.where(ended, np.float32(0.0), v)).astype(np.float32)
        for k in range(r.shape[1] - 2, -1, -1):
            tail = (r[:, k] + g * tail).astype(np.float32)
    return tail


def ntuple_beam_ply(node_value, node_running, child_value, distinct, width: int):
    """The choice of one ply of the beam rule (tpl_placement_beam's candidates, tpl_ntuple_beam's values) on top of beam_select:
    node_value f32 [Q] and node_running [Q] of the nodes of Beam_{j-1} in their stored order, child_value f32 [Q, 40] the folded
    value of every placement of every running node, distinct [Q, 40] or [40] where a placement is a distinct one.  A node that does
    not run is ONE candidate, itself, with its value unchanged; a running node gives its distinct placements in ascending b.
    Returns (node int64 [kept], placement int64 [kept] -- 255 for a node carried --, value f32 [kept]) of Beam_j, in candidate
    order; every value keeps its own bits."""
    nv = np.asarray(node_value, dtype=np.float32).reshape(-1)
    run = np.asarray(node_running).astype(bool).reshape(nv.shape[0])
    cv = np.asarray(child_value, dtype=np.float32).reshape(nv.shape[0], NUM_ACTIONS)
    d = np.broadcast_to(np.asarray(distinct).astype(bool), cv.shape)
    cand = np.where(run[:, None], d, np.arange(NUM_ACTIONS)[None, :] == 0)
    value = np.where(run[:, None], cv, nv[:, None])
    at = np.flatnonzero(cand.reshape(-1))
    keep = at[beam_select(value.reshape(-1)[at], width)]
    q, b = keep // NUM_ACTIONS, keep % NUM_ACTIONS
    return q, np.where(run[q], b, NO_SECOND), value[q, b]


def ntuple_beam_choice(children, gamma, depth: int, width: int, running: bool = True):
    """The rule of tpl_ntuple_beam for ONE state whose moves are given by a function: children(path) -> (reward f32 [40], ended
    [40], value f32 [40], distinct [40]) of the node reached by the tuple of placements `path` -- the reward of every placement,
    whether it ends the game, V of the child where it does not, and which placements are distinct.  `depth` is the EFFECTIVE depth.
    Returns (action, plan -- a list of `depth` placements padded with 255 --, score f32).  A state that is not running: (0, all
    255, 0)."""
    if isinstance(depth, bool) or int(depth) != depth or not 1 <= int(depth) <= NTUPLE_BEAM_MAX_DEPTH:
        raise ValueError(f"depth must be an integer in [1, {NTUPLE_BEAM_MAX_DEPTH}]")
    if not running:
        return 0, [NO_SECOND] * int(depth), np.float32(0.0)
    nodes = [dict(path=(), rewards=[], value=np.float32(0.0), running=True)]
    for _ in range(int(depth)):
        child_value = np.zeros((len(nodes), NUM_ACTIONS), np.float32)
        distinct = np.zeros((len(nodes), NUM_ACTIONS), bool)
        made = {}
        for q, node in enumerate(nodes):
            if not node["running"]:
                continue
            reward, ended, value, distinct[q] = children(node["path"])
            reward = np.asarray(reward, dtype=np.float32)
            made[q] = (reward, np.asarray(ended).astype(bool))
            before = np.broadcast_to(np.asarray(node["rewards"], np.float32), (NUM_ACTIONS, len(node["rewards"])))
            child_value[q] = ntuple_beam_values(np.concatenate([before, reward[:, None]], axis=1), ended, value, gamma)
        qs, bs, vs = ntuple_beam_ply([x["value"] for x in nodes], [x["running"] for x in nodes], child_value, distinct, width)
        nodes = [nodes[q] if b == NO_SECOND else dict(path=nodes[q]["path"] + (int(b),), rewards=nodes[q]["rewards"] + [made[q][0][b]],
                                                      value=v, running=not made[q][1][b]) for q, b, v in zip(qs, bs, vs)]
    best = nodes[beam_select(np.array([x["value"] for x in nodes], np.float32), 1)[0]]
    plan = list(best["path"]) + [NO_SECOND] * (int(depth) - len(best["path"]))
    return plan[0], plan, np.float32(best["value"])


# ------------------------------------------------------------------------------------------------ device packing
def policy_tensors(model) -> list:
    """The ten float32 parameter tensors of a PolicyMLP, contiguous, in tpl_learn_pack's argument order."""
    return [t.detach().contiguous() for layer in (model.layer1, model.layer2, model.layer3, model.layer4, model.layer5)
            for t in (layer.weight, layer.bias)]


_SHAPES = [(128, 217), (128,), (128, 128), (128,), (128, 128), (128,), (128, 128), (128,), (14, 128), (14,)]


def pack_policy_device(params, kind: str = "split", out=None):
    """tpl_learn_pack: ten float32 device tensors (w1, b1, ..., w5, b5; torch layout) -> the policy image of `kind`
    ("bf16", "f32" or "split") as a uint8 device tensor, byte-identical to _lib.pack_policy's.  Enqueued on the current
    stream; no host sync."""
    import torch
    if kind not in IMAGE_KINDS:
        raise ValueError(f"kind must be one of {sorted(IMAGE_KINDS)}")
    params = list(params)
    if len(params) != 10:
        raise ValueError("pack_policy_device takes the ten parameter tensors of Model(217, 14)")
    dev = params[0].device
    for t, shape in zip(params, _SHAPES):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape or t.device != dev
                or dev.type != "cuda" or not t.is_contiguous()):
            raise ValueError(f"policy parameters must be contiguous float32 {_SHAPES} on one GPU")
    L = lib()
    nbytes = L.tpl_learn_image_bytes(IMAGE_KINDS[kind])
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or tuple(out.shape) != (nbytes,) or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of {nbytes} bytes on {dev}")
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    check(L.tpl_learn_pack(IMAGE_KINDS[kind], *[t.data_ptr() for t in params], out.data_ptr(), stream))
    return out


# ------------------------------------------------------------------------------------------------ tallies and the resampled pool
# numpy mirrors of csrc/learn/curriculum.hip, written from include/tpl_learn.h's rule ("Per-configuration tallies and the resampled
# pool") and the interchange form of a pool (rows [n_cfg, 20], pieces [n_cfg, M + 1]).
def _mulhi64(a, b):
    """floor(a * b / 2^64) of uint64 arrays, from 32-bit halves (exact)."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    s32 = np.uint64(32)
    with np.errstate(over="ignore"):
        a_hi, a_lo, b_hi, b_lo = a >> s32, a & _M32, b >> s32, b & _M32
        mid = a_hi * b_lo + ((a_lo * b_lo) >> s32)              # below 2^64: (2^32 - 1)^2 + 2^32 - 1
        mid2 = a_lo * b_hi + (mid & _M32)
        return a_hi * b_hi + (mid >> s32) + (mid2 >> s32)


def _fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & _M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def assign_entries(boards, births, seed: int, global_offset: int, n_cfg: int, mode: int) -> np.ndarray:
    """The pool entry of the episode of board `boards[k]` (local index; global index global_offset + board) that begins at step
    `births[k]`, in a buffer of n_cfg entries: int64, broadcast over the two arrays.  mode 0 = hash, 1 = sequential."""
    if mode not in (0, 1):
        raise ValueError("mode must be 0 (hash) or 1 (sequential)")
    if not 1 <= int(n_cfg) < (1 << 32):
        raise ValueError("n_cfg must be in [1, 2^32)")
    if global_offset < 0:
        raise ValueError("global_offset must not be negative")
    g = np.asarray(boards, dtype=np.uint64) + np.uint64(global_offset)
    birth = np.asarray(births, dtype=np.uint64)
    n = np.uint64(n_cfg)
    if mode == 1:
        return ((g % n + (birth & _M32) % n) % n).astype(np.int64)
    m24 = np.uint64(0xFFFFFF)
    with np.errstate(over="ignore"):
        seed_mix = _mix64(np.uint64(seed % (1 << 64)) + _GOLDEN) >> np.uint64(32)          # splitmix64(seed) >> 32
        x = ((g & _M32) + (birth & _M32) * np.uint64(0x9E3779B1)) & _M32
        x = x ^ ((((g >> np.uint64(32)) & m24) * np.uint64(0x85EBCB)) & _M32)
        x = x ^ ((((birth >> np.uint64(32)) & m24) * np.uint64(0xC2B2AF)) & _M32) ^ seed_mix
        return ((_fmix32(x) * n) >> np.uint64(32)).astype(np.int64)


def check_pool_weights(weights) -> int:
    """The total of int64 weights [n_cfg] that tpl_pool_resample's prefix sums may be made of: all non-negative, total in [1, 2^62)."""
    w = np.asarray(weights)
    if w.dtype != np.int64 or w.ndim != 1 or w.shape[0] < 1:
        raise ValueError("weights must be int64 [n_cfg], n_cfg >= 1")
    if int(w.min()) < 0:
        raise ValueError("weights must not be negative")
    total = int(w.astype(object).sum())                      # Python integers: the sum of int64 values may not fit one
    if not 1 <= total < (1 << 62):
        raise ValueError(f"the weights' total must be in [1, 2^62), got {total}")
    return total


def curriculum_weights(episodes, wins, floor: int = 1, gain: int = 8) -> np.ndarray:
    """floor + gain * (episodes - wins) as int64: the losses so far, and a floor that keeps every configuration alive."""
    for name, v in (("floor", floor), ("gain", gain)):
        if isinstance(v, bool) or int(v) != v or int(v) < 0:
            raise ValueError(f"{name} must be a non-negative integer, got {v!r}")
    e, w = np.asarray(episodes), np.asarray(wins)
    if e.shape != w.shape or e.ndim != 1 or e.dtype.kind not in "iu" or w.dtype.kind not in "iu":
        raise ValueError("episodes and wins must be integer arrays of one shape [n_cfg]")
    return np.int64(floor) + np.int64(gain) * (e.astype(np.int64) - w.astype(np.int64))


def pool_resample(rows, pieces, weights, count: int, seed: int = 0, round: int = 0):
    """tpl_pool_resample on the host: (rows' [count, 20], pieces' [count, M + 1], source int32 [count]).  Draw j takes the target
    t_j = floor(h_j * total / 2^64), h = _draw_hashes(seed, round, count), and the first entry whose inclusive prefix sum is above it."""
    rows, pieces = np.asarray(rows), np.asarray(pieces)
    total = check_pool_weights(weights)
    n_cfg = np.asarray(weights).shape[0]
    if rows.ndim != 2 or rows.shape != (n_cfg, 20) or rows.dtype.itemsize != 2 or rows.dtype.kind not in "iu":
        raise ValueError(f"rows must be 16-bit integers [{n_cfg}, 20]")
    if pieces.ndim != 2 or pieces.shape[0] != n_cfg or pieces.dtype != np.uint8 or not 2 <= pieces.shape[1] <= 255:
        raise ValueError(f"pieces must be uint8 [{n_cfg}, M + 1]")
    if isinstance(count, bool) or int(count) != count or not 1 <= int(count) < (1 << 31):
        raise ValueError("count must be in [1, 2^31)")
    prefix = np.cumsum(np.asarray(weights, dtype=np.int64)).astype(np.uint64)
    target = _mulhi64(_draw_hashes(seed, round, int(count)), np.uint64(total))
    source = np.searchsorted(prefix, target, side="right").astype(np.int32)
    return rows[source].copy(), pieces[source].copy(), source
