"""Outcomes per configuration and a curriculum pool resampled on the device (the rule: include/tpl_learn.h, "Per-configuration
tallies and the resampled pool"; the kernels: csrc/learn/curriculum.hip).

    config_index(env)             which pool entry every board is playing: the environment's own assignment rule, from the side
    PoolTally(env).observe(a)     called just before env.step(a): episodes and wins per pool entry, int32 on the device, one launch
    resample_pool(rows, pieces, weights, count)
                                  a pool of `count` entries drawn in proportion to int64 weights: search and gather in one launch
    curriculum_weights(e, w)      floor + gain * (episodes - wins): a plain default for the weights
    PoolCurriculum(env, rows, pieces)
                                  a tally over the loaded pool folded into one over the BASE configurations, and refresh(): reweight,
                                  resample, load_configs -- all on the device

Nothing here writes to the environment except load_configs() in PoolCurriculum.refresh().
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _learn_lib
from ._learn_lib import check
from .lookahead import _state_ptrs

__all__ = ["config_index", "PoolTally", "resample_pool", "curriculum_weights", "PoolCurriculum"]

_ASSIGN = {"hash": 0, "sequential": 1}
_ACTION_CODES = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}      # tpl_int_dtype
UNKNOWN = -1                                                           # config_index of a frozen board on a fresh buffer (0xFFFFFFFF)


def _nonneg_int(name: str, v, least: int = 0) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < least:
        raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")
    return int(v)


def _assignment(env):
    """What the assignment rule reads of `env`: (plane_a, plane_b, clock, n, global_offset, seed, mode, n_cfg of slot 0, of slot 1)."""
    info = env.pool_info()
    if info["n_configs"] == 0:
        raise ValueError("the environment has no configuration pool (load_configs first)")
    n_cfg = [0, 0]
    n_cfg[info["current_slot"]], n_cfg[info["current_slot"] ^ 1] = info["n_configs"], info["n_configs_other"]
    pa, pb = _state_ptrs(env)
    return (pa, pb, env._clocks().data_ptr(), env.num_envs, env.global_offset, env.seed % (1 << 64), _ASSIGN[env.assign], *n_cfg), info


def config_index(env, out: Optional[torch.Tensor] = None, slot: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The pool entry of every board's current episode, int32 [N] on the device (the uint32 of tpl_config_index; pools have fewer than
    2^31 entries here), by the environment's own rule: assign(global board index, clock - moves_used, seed) in the buffer whose bit
    the board carries.  `slot` (uint8 [N], optional) receives that bit.  A FINISHED board of an environment without auto-reset has no
    recoverable birth (its clock runs on, its moves_used does not): its entry of `out` is left as it is, so one buffer passed before
    every step keeps the entry each board finished with; a fresh buffer (out=None) holds UNKNOWN (-1) there."""
    args, _ = _assignment(env)
    if out is None:
        out = torch.full((env.num_envs,), UNKNOWN, dtype=torch.int32, device=env.device)
    env._own(out, torch.int32, "out")
    if slot is not None:
        env._own(slot, torch.uint8, "slot")
    stream = torch._C._cuda_getCurrentRawStream(env.device.index)
    check(_learn_lib.lib().tpl_config_index(*args, out.data_ptr(), None if slot is None else slot.data_ptr(), stream))
    return out


class PoolTally:
    """episodes and wins per entry of the pool `env` has loaded: int32 [n_cfg] device tensors, added to by observe().

        tally.observe(action); env.step(action)      # every step: one launch that reads the planes, the clocks and the actions

    observe() makes every running board's move in registers and, where it ends the episode, adds to the entry the board was dealt
    (frozen boards add nothing; the environment is not written).  After env.load_configs(...) call swap(): the tallies become
    `previous_episodes` / `previous_wins`, which boards still finishing on the old buffer keep adding to, and fresh zeroed ones
    take the new pool.  A full env.reset() is the caller's cue to zero()."""

    def __init__(self, env):
        self.env = env
        info = env.pool_info()
        if info["n_configs"] == 0:
            raise ValueError("PoolTally needs an environment with a configuration pool (load_configs first)")
        self._slot = info["current_slot"]
        self.episodes, self.wins = self._fresh(info["n_configs"])
        self.previous_episodes = self.previous_wins = None

    def _fresh(self, n_cfg: int):
        return tuple(torch.zeros(n_cfg, dtype=torch.int32, device=self.env.device) for _ in range(2))

    def zero(self) -> None:
        """Start over (after a full reset): the current tallies are zeroed, the previous buffer's are dropped."""
        self.episodes.zero_()
        self.wins.zero_()
        self.previous_episodes = self.previous_wins = None

    def swap(self) -> None:
        """After env.load_configs(...): current becomes previous, zeroed tallies of the new pool's size become current."""
        info = self.env.pool_info()
        if info["current_slot"] == self._slot:
            raise ValueError("swap() follows a load_configs() on a live environment: the current pool buffer has not changed")
        self.previous_episodes, self.previous_wins = self.episodes, self.wins
        self._slot = info["current_slot"]
        self.episodes, self.wins = self._fresh(info["n_configs"])

    def observe(self, action: torch.Tensor) -> None:
        """Count the episodes that env.step(action) is about to end.  `action`: the uint8 / int32 / int64 tensor the step takes."""
        env = self.env
        env._own(action, _ACTION_CODES, "action")
        args, info = _assignment(env)
        if info["current_slot"] != self._slot or info["n_configs"] != self.episodes.shape[0]:
            raise ValueError("the environment's pool changed under this tally: call swap() after load_configs()")
        pairs = [(None, None), (None, None)]
        pairs[self._slot] = (self.episodes.data_ptr(), self.wins.data_ptr())
        if self.previous_episodes is not None and info["n_configs_other"] == self.previous_episodes.shape[0]:
            pairs[self._slot ^ 1] = (self.previous_episodes.data_ptr(), self.previous_wins.data_ptr())
        stream = torch._C._cuda_getCurrentRawStream(env.device.index)
        pa, pb, clock, n = args[:4]
        check(_learn_lib.lib().tpl_pool_tally(pa, pb, clock, n, env.L, env.M, action.data_ptr(), _ACTION_CODES[action.dtype], *args[4:],
                                              *pairs[0], *pairs[1], stream))


def _weights_total(weights: torch.Tensor) -> int:
    """The exact total of non-negative int64 weights (one host sync); ValueError for a negative weight or a total outside [1, 2^62)."""
    hi, lo = weights >> 31, weights & 0x7FFFFFFF                         # both sums fit int64 for fewer than 2^31 weights
    least, s_hi, s_lo = torch.stack((weights.min(), hi.sum(), lo.sum())).tolist()
    if least < 0:
        raise ValueError("weights must not be negative")
    total = (s_hi << 31) + s_lo
    if not 1 <= total < (1 << 62):
        raise ValueError(f"the weights' total must be in [1, 2^62), got {total}")
    return total


def _pool_tensors(rows, pieces, what: str = "rows / pieces"):
    if not isinstance(rows, torch.Tensor) or not isinstance(pieces, torch.Tensor):
        raise ValueError(f"{what} must be torch tensors")
    if rows.dtype not in (torch.int16, torch.uint16) or rows.dim() != 2 or rows.shape[1] != 20 or rows.shape[0] < 1:
        raise ValueError("rows must be int16 [n_cfg, 20]")
    if pieces.dtype != torch.uint8 or pieces.dim() != 2 or pieces.shape[0] != rows.shape[0] or not 2 <= pieces.shape[1] <= 255:
        raise ValueError(f"pieces must be uint8 [{rows.shape[0]}, M + 1]")
    if rows.device != pieces.device:
        raise ValueError("rows and pieces must be on one device")
    return rows.shape[0], pieces.shape[1] - 1


def resample_pool(rows: torch.Tensor, pieces: torch.Tensor, weights: torch.Tensor, count: int, seed: int = 0, round: int = 0):
    """A pool of `count` configurations drawn from (rows int16 [n_cfg, 20], pieces uint8 [n_cfg, M + 1]) in proportion to `weights`
    (int64 [n_cfg], non-negative, total in [1, 2^62)): returns (rows', pieces', source int32 [count]) on the device, entry j a copy of
    configuration source[j].  Draw j is position j + 1 of the splitmix64 stream keyed by (seed, round) (the replay samplers' draw),
    multiplied high with the total and looked up in the inclusive prefix sums (torch.cumsum on int64: exact); the search and the
    gather are one launch.  A configuration of weight 0 is never drawn.  One host sync, for the check of the weights."""
    n_cfg, M = _pool_tensors(rows, pieces)
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.int64 or tuple(weights.shape) != (n_cfg,):
        raise ValueError(f"weights must be an int64 tensor [{n_cfg}]")
    count = _nonneg_int("count", count, 1)
    if count >= (1 << 31):
        raise ValueError("count must be below 2^31")
    seed, round = _nonneg_int("seed", seed) % (1 << 64), _nonneg_int("round", round) % (1 << 64)
    if weights.device != rows.device:
        raise ValueError("weights must be on the pool's device")
    _weights_total(weights)
    d = rows.device
    if d.type != "cuda":
        raise ValueError("resample_pool runs on a GPU only (the numpy form is _learn_lib.pool_resample)")
    rows, pieces = rows.contiguous(), pieces.contiguous()
    prefix = torch.cumsum(weights, 0)
    rows_out = torch.empty((count, 20), dtype=rows.dtype, device=d)
    pieces_out = torch.empty((count, M + 1), dtype=torch.uint8, device=d)
    source = torch.empty(count, dtype=torch.int32, device=d)
    with torch.cuda.device(d):
        stream = torch._C._cuda_getCurrentRawStream(d.index)
        check(_learn_lib.lib().tpl_pool_resample(rows.data_ptr(), pieces.data_ptr(), n_cfg, M, prefix.data_ptr(), count, seed, round,
                                                 rows_out.data_ptr(), pieces_out.data_ptr(), source.data_ptr(), stream))
    return rows_out, pieces_out, source


def curriculum_weights(episodes: torch.Tensor, wins: torch.Tensor, floor: int = 1, gain: int = 8) -> torch.Tensor:
    """floor + gain * (episodes - wins) as int64: the losses so far plus a floor that keeps every configuration alive.  A plain
    default; resample_pool and PoolCurriculum.refresh(weights=...) take any other non-negative int64 weights."""
    floor, gain = _nonneg_int("floor", floor), _nonneg_int("gain", gain)
    for t in (episodes, wins):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError("episodes and wins must be int32 / int64 tensors [n_cfg]")
    if episodes.shape != wins.shape:
        raise ValueError("episodes and wins must have one shape")
    return floor + gain * (episodes.to(torch.int64) - wins.to(torch.int64))


class PoolCurriculum:
    """Prioritized level replay over a BASE pool (rows int16 [n_base, 20], pieces uint8 [n_base, M + 1], on env's device).

    The first pool is the base pool itself (loaded here unless `env` already holds it: pass loaded=True), source = arange.
    observe(action) goes before every env.step(action).  refresh() folds the loaded pool's tallies into `base_episodes` /
    `base_wins` (int64 [n_base]) through `source` (index_add_, exact) and zeroes them, computes curriculum_weights(floor, gain) of
    the base tallies, resamples `count` entries (default n_base; draw `round` = the number of refreshes so far) and loads them with
    env.load_configs(..., validate=False) -- everything on the device but the weights' one check.  While the environment's other pool
    buffer is still in use (pool_info()["steps_until_swap"] > 0) refresh() returns False and changes nothing.  Boards that finish on
    the buffer a refresh replaced keep counting: the next refresh folds them in through the source they were drawn with."""

    def __init__(self, env, rows: torch.Tensor, pieces: torch.Tensor, count: Optional[int] = None, seed: int = 0, floor: int = 1,
                 gain: int = 8, loaded: bool = False):
        n_base, M = _pool_tensors(rows, pieces)
        if M != env.M or rows.device != env.device:
            raise ValueError(f"the base pool must be [n, 20] / [n, {env.M + 1}] on {env.device}")
        self.env, self.rows, self.pieces = env, rows.contiguous(), pieces.contiguous()
        self.count = n_base if count is None else _nonneg_int("count", count, 1)
        self.seed, self.floor, self.gain = _nonneg_int("seed", seed), _nonneg_int("floor", floor), _nonneg_int("gain", gain)
        if not loaded:
            env.load_configs(self.rows, self.pieces, validate=False)
        elif env.n_configs != n_base:
            raise ValueError("loaded=True: the environment's pool is not the base pool")
        self.tally = PoolTally(env)
        self.source = torch.arange(n_base, dtype=torch.int32, device=env.device)
        self._previous_source = None
        self.base_episodes = torch.zeros(n_base, dtype=torch.int64, device=env.device)
        self.base_wins = torch.zeros(n_base, dtype=torch.int64, device=env.device)
        self.refreshes = 0

    def observe(self, action: torch.Tensor) -> None:
        self.tally.observe(action)

    def _fold(self, source, episodes, wins) -> None:
        if episodes is None:
            return
        self.base_episodes.index_add_(0, source, episodes.to(torch.int64))
        self.base_wins.index_add_(0, source, wins.to(torch.int64))
        episodes.zero_()
        wins.zero_()

    def fold(self) -> None:
        """Move what the tallies hold into the base tallies (refresh() does; also the way to read them up to date)."""
        t = self.tally
        if self._previous_source is not None:
            self._fold(self._previous_source, t.previous_episodes, t.previous_wins)
        self._fold(self.source, t.episodes, t.wins)

    def weights(self) -> torch.Tensor:
        return curriculum_weights(self.base_episodes, self.base_wins, self.floor, self.gain)

    def refresh(self, weights: Optional[torch.Tensor] = None) -> bool:
        env = self.env
        if env.pool_info()["steps_until_swap"] > 0:
            return False
        self.fold()
        w = self.weights() if weights is None else weights
        rows, pieces, source = resample_pool(self.rows, self.pieces, w, self.count, self.seed, self.refreshes)
        env.load_configs(rows, pieces, validate=False)
        self.tally.swap()
        self._previous_source, self.source = self.source, source
        self.refreshes += 1
        return True

    def base_win_rate(self) -> torch.Tensor:
        """wins / max(episodes, 1) per base configuration, float64 on the device, of what has been folded so far."""
        return self.base_wins.to(torch.float64) / self.base_episodes.clamp(min=1).to(torch.float64)
