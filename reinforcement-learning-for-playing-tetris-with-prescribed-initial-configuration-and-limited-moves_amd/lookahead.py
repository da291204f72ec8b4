"""Afterstates on the device and a one-ply lookahead policy on top of them (the rule: include/tpl_learn.h; the kernel:
csrc/learn/afterstates.hip).

    afterstates(env)          the 40 successors of every resident board: planes, reward, done, rows cleared, canonical action
    LookaheadPolicy(env, image, gamma).act()
                              argmax over the DISTINCT placements a of  r(s, a) + gamma * (1 - done) * V(s'_a),
                              V = max(logits[0:4]) + max(logits[4:14]) of `image` on the afterstate -- one enumeration and one
                              policy launch over 40 N boards, both on the device

An afterstate's piece window is good for the current and the next piece only (on the move at which the environment refills
its window the entries behind them differ from the step's): search deeper than one ply from environment states.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _learn_lib
from ._learn_lib import NUM_ACTIONS, check

_MAX_BOARDS = ((1 << 31) - 1) // NUM_ACTIONS


def _boards(env, who: str) -> int:
    n = int(env.num_envs)
    if not 1 <= n <= _MAX_BOARDS:
        raise ValueError(f"{who} takes an environment of 1 .. {_MAX_BOARDS} boards (40 N must stay below 2^31)")
    return n


def _state_ptrs(env):
    from ._lib import check as env_check
    pa, pb = C.c_void_p(), C.c_void_p()
    env_check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
    return pa.value, pb.value


def _ptr(t):
    """The device address of a tensor; an address or None as it is."""
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _source_planes(env, states_a, states_b, who: str, into=None):
    """(K, plane_a, plane_b) of the states that `who` reads: int32 [K, 4] plane pairs as env.expand_states takes them, moved to
    env.device, or env's resident boards (both None: K = env.num_envs, read in place).  A plane is a tensor where it was given
    -- the caller holds it until its launch is enqueued -- and a device address where it is resident: _ptr takes either.
    `into` (afterstates' destination environment) must hold 40 K boards: a condition on K, refused before the device is asked
    for anything."""
    if (states_a is None) != (states_b is None):
        raise ValueError("states_a and states_b go together")
    if states_a is not None:
        for t in (states_a, states_b):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 2 or t.shape[1] != 4:
                raise ValueError("states_a / states_b must be int32 [K, 4] tensors")
        if states_a.shape != states_b.shape:
            raise ValueError("states_a / states_b must be int32 [K, 4] tensors of equal shape")
    k = int(env.num_envs if states_a is None else states_a.shape[0])
    if not 1 <= k <= _MAX_BOARDS:
        raise ValueError(f"{who} takes 1 .. {_MAX_BOARDS} states (40 K must stay below 2^31)")
    if into is not None and (into is env or into.num_envs != NUM_ACTIONS * k or into.device != env.device):
        raise ValueError(f"into must be another environment of exactly {NUM_ACTIONS * k} boards on {env.device}")
    if states_a is None:
        return (k, *_state_ptrs(env))
    return k, states_a.to(env.device).contiguous(), states_b.to(env.device).contiguous()


def _enumerate(env, src_a, src_b, k: int, out_a, out_b, reward, done, cleared, canonical) -> None:
    """tpl_afterstates of k states at (src_a, src_b) under env's L, M and reward parameters; tensors or device addresses."""
    stream = torch._C._cuda_getCurrentRawStream(env.device.index)
    check(_learn_lib.lib().tpl_afterstates(_ptr(src_a), _ptr(src_b), k, env.L, env.M, *env.reward_params, _ptr(out_a), _ptr(out_b),
                                           _ptr(reward), _ptr(done), _ptr(cleared), _ptr(canonical), stream))


def afterstates(env, states_a: Optional[torch.Tensor] = None, states_b: Optional[torch.Tensor] = None, with_states: bool = True,
                into=None) -> dict:
    """The 40 afterstates of K states: the resident boards of `env` (K = env.num_envs, read in place), or int32 [K, 4] plane
    pairs as env.expand_states takes them.  Uses env.L, env.M and env.reward_params; `env` itself is not changed.

    Returns states_a, states_b int32 [K, 40, 4] (unless with_states=False), reward f32 [K, 40], done, cleared, canonical u8
    [K, 40]; entry [i, a] belongs to action a = 10 r + l played from state i, and a == canonical[i, a] marks the distinct
    placements.  `into`: a BatchedTetris of exactly 40 K boards whose resident planes receive the afterstates (board 40 i + a;
    zero copy, its counters and step clock are not touched); the dict then holds no state tensors."""
    k, src_a, src_b = _source_planes(env, states_a, states_b, "afterstates", into)
    d = env.device
    out = dict(reward=torch.empty((k, NUM_ACTIONS), dtype=torch.float32, device=d))
    for name in ("done", "cleared", "canonical"):
        out[name] = torch.empty((k, NUM_ACTIONS), dtype=torch.uint8, device=d)
    planes = (None, None)
    if into is not None:
        planes = _state_ptrs(into)
    elif with_states:
        out["states_a"] = torch.empty((k, NUM_ACTIONS, 4), dtype=torch.int32, device=d)
        out["states_b"] = torch.empty((k, NUM_ACTIONS, 4), dtype=torch.int32, device=d)
        planes = (out["states_a"], out["states_b"])
    _enumerate(env, src_a, src_b, k, planes[0], planes[1], out["reward"], out["done"], out["cleared"], out["canonical"])
    return out


class LookaheadPolicy:
    """One-ply lookahead on the resident boards of `env`: act() scores action a as reward + gamma * (1 - done) * V(afterstate),
    V = max(logits[0:4]) + max(logits[4:14]) of `image` (any image env.policy_act takes; None: V = 0), and returns the arg-max
    over the distinct placements (a == canonical[a]), the lowest index on ties; a finished board gets action 0.

    Boards go `chunk` at a time: the kernel writes a chunk's afterstates straight into the resident planes of a scratch
    environment of 40 * chunk boards, on which policy_act evaluates the image (rows past a partial last chunk are ignored)."""

    def __init__(self, env, image: Optional[torch.Tensor] = None, gamma: float = 1.0, chunk: int = 16384):
        from .env import BatchedTetris
        if isinstance(chunk, bool) or int(chunk) != chunk or int(chunk) < 1:
            raise ValueError("chunk must be a positive integer")
        self.env, self.image, self.gamma = env, image, float(gamma)
        self.chunk = min(int(chunk), env.num_envs, _MAX_BOARDS)
        d, rows = env.device, NUM_ACTIONS * self.chunk
        self._reward = torch.empty((self.chunk, NUM_ACTIONS), dtype=torch.float32, device=d)
        self._done = torch.empty((self.chunk, NUM_ACTIONS), dtype=torch.uint8, device=d)
        self._canonical = torch.empty((self.chunk, NUM_ACTIONS), dtype=torch.uint8, device=d)
        self._ids = torch.arange(NUM_ACTIONS, dtype=torch.int64, device=d)
        self.scratch = None
        if image is not None:
            self.scratch = BatchedTetris(env.L, env.M, rows, device=d, seed=env.seed)
            self._scratch_action = torch.empty(rows, dtype=torch.uint8, device=d)
            self._logits = torch.empty((rows, 14), dtype=torch.float32, device=d)

    @torch.no_grad()
    def scores(self, first: int, count: int) -> torch.Tensor:
        """float32 [count, 40]: the score of every action of boards [first, first + count) (count <= chunk), -inf where the
        action is an alias of a lower one."""
        if not (0 <= first and 1 <= count <= self.chunk and first + count <= self.env.num_envs):
            raise ValueError("scores() takes a range of at most `chunk` boards of the environment")
        src_a, src_b = _state_ptrs(self.env)
        planes = (None, None) if self.scratch is None else _state_ptrs(self.scratch)
        _enumerate(self.env, src_a + 16 * first, src_b + 16 * first, count, planes[0], planes[1], self._reward, self._done, None,
                   self._canonical)
        score = self._reward[:count]
        if self.scratch is not None:
            self.scratch.policy_act(self.image, out=self._scratch_action, logits=self._logits)
            lg = self._logits[:NUM_ACTIONS * count]
            v = (lg[:, :4].max(dim=1).values + lg[:, 4:14].max(dim=1).values).view(count, NUM_ACTIONS)
            score = torch.where(self._done[:count] != 0, score, score + self.gamma * v)
        return torch.where(self._canonical[:count] == self._ids, score, torch.full_like(score, float("-inf")))

    @torch.no_grad()
    def act(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [N]: the lookahead action of every resident board of the environment (which is left as it is)."""
        n = self.env.num_envs
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=self.env.device)
        self.env._own(out, torch.uint8, "out")
        for first in range(0, n, self.chunk):
            count = min(self.chunk, n - first)
            score = self.scores(first, count)
            best = score.max(dim=1, keepdim=True).values
            pick = torch.where(score == best, self._ids, NUM_ACTIONS).min(dim=1).values     # the lowest index at the maximum
            out[first:first + count] = torch.where(pick < NUM_ACTIONS, pick, 0).to(torch.uint8)   # (no maximum: a NaN score)
        return out
