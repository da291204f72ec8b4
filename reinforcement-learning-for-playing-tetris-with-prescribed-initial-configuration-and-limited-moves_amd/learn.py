"""DQN on the batched environment: the algorithm of the upstream model/train.py (the PyTorch DQN tutorial's
`optimize_model`, with its constants as defaults), over a packed replay ring that lives on the device.

Data path of one round (collect + update):

    actor_rollout(split image of the online net, epsilon)      one launch, T steps x N boards, records the 32-B states
    tpl_replay_push                                             the chunk -> 80-B records (s, a, r, done, s') in the ring
    tpl_replay_sample                                           B draws -> obs(s) [B, 217], s' as planes of a B-board env, a, r, done
    tpl_policy_act_split(scratch env, target image)             Q'(s') [B, 14] at float32 accuracy on the bf16 matrix pipe
    torch autograd                                              Q(s) of the online net, Huber loss, AdamW(amsgrad) step
    soft update + tpl_learn_pack (split)                        the target image repacked on the device, no host copy

Factored Q over the 40 actions.  Model(217, 14) has 14 outputs for 40 actions (rotation r in 0..3, location l in 0..9,
action = 10 r + l); the environment's decode (tpl_decode_actions, and pick_action inside the policy kernels) takes
argmax(out[0:4]) as the rotation and argmax(out[4:14]) as the location.  The learner scores an action as the sum of its two
heads,

    Q(s, a) = out[a // 10] + out[4 + a % 10],      so      max_a Q(s, a) = max(out[0:4]) + max(out[4:14]),

whose arg-max is exactly the decoded action: the actor's greedy choice is the learner's greedy choice.  The 14 outputs cannot
score 40 actions any other way that agrees with that decode (a score that is not monotone in both heads separately would
have an arg-max the decode does not return).

TD target  y = r + gamma * (1 - done) * (max Q'_rot(s') + max Q'_loc(s')), in float32; loss SmoothL1 (Huber, delta 1)
between Q(s, a) and y; gradients clipped to +-100 by value; AdamW(lr, amsgrad=True); after every update the soft update
theta' <- tau * theta + (1 - tau) * theta' and a repack of the target image.  With n_step > 1 the sampler returns the n-step
return R and discount gamma^K (0 after a done) instead, and y = R + discount * (max Q'_rot(s') + max Q'_loc(s')).

Epsilon schedule  eps_end + (eps_start - eps_end) * exp(-steps_done / eps_decay), where steps_done counts LOCKSTEP
ITERATIONS of the batch: the batched reading of the reference's per-action counter (each iteration is one action on every
board).  Epsilon is held constant within one collect() -- one actor_rollout launch.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import weakref
from typing import Optional

import torch
from torch import nn

from . import _learn_lib
from ._learn_lib import check, pack_policy_device
from .actor import PolicyMLP
from .env import OBS_DIM, BatchedTetris, _OBS_CODES

RECORD_BYTES = _learn_lib.RECORD_BYTES


class ReplayRing:
    """`capacity` transitions of 80 bytes on the device (include/tpl_learn.h).  A push of a [T, N] chunk at head h writes
    transition (t, board i) to slot (h + t * N + i) mod capacity; the oldest transitions are overwritten.  Draws are uniform
    with replacement over the filled slots [0, size).

    n-step returns (sample(..., n_step > 1)) follow a board from slot to slot `stride` = N apart, so they need every push
    since construction to have come from one environment object with one N; a push that breaks this is still taken, but
    n-step sampling raises ValueError afterwards."""

    def __init__(self, capacity: int, device):
        capacity = int(capacity)
        if not 1 <= capacity < (1 << 32):
            raise ValueError("capacity must be in [1, 2^32)")
        self.capacity, self.device = capacity, torch.device(device)
        self.data = torch.zeros(capacity * RECORD_BYTES, dtype=torch.uint8, device=self.device)
        self.head = 0
        self.size = 0
        self.stride = None                                       # N of the first push
        self._source = None                                      # weak reference to the environment of the first push
        self._one_source = True                                  # every push since: that environment, that N

    def _stream(self):
        return torch._C._cuda_getCurrentRawStream(self.device.index)

    def _track_push(self, env, n: int) -> None:
        """Bookkeeping of the n-step rule: the first push fixes the environment and the stride, any other breaks it."""
        if self.stride is None:
            self.stride, self._source = int(n), weakref.ref(env)
        elif int(n) != self.stride or self._source() is not env:
            self._one_source = False

    def _nstep_args(self, n_step, gamma):
        """Validated (n_step, gamma) of a sample() call; gamma is None at n_step = 1."""
        if isinstance(n_step, bool) or int(n_step) != n_step or not 1 <= int(n_step) <= _learn_lib.NSTEP_MAX:
            raise ValueError(f"n_step must be an integer in [1, {_learn_lib.NSTEP_MAX}]")
        n_step = int(n_step)
        if n_step == 1:
            return 1, None
        if gamma is None:
            raise ValueError("n_step > 1 needs gamma")
        gamma = float(gamma)
        if not 0.0 <= gamma <= 1.0:
            raise ValueError("gamma must be in [0, 1]")
        if not self._one_source:
            raise ValueError("n-step sampling needs every push from one environment with one N: this ring was pushed from "
                             "more than one environment or with more than one N")
        return n_step, gamma

    def _sample_nstep(self, tree, batch, seed, update, next_env, obs_dtype, with_index, n_step, gamma, mirror=0) -> dict:
        """The n-step draw (mirror = 0: tpl_replay_sample_nstep) or, with a mirror mode, any draw form through
        tpl_replay_sample_mirror (n_step = 1 is then the 1-step form: no discount, no steps)."""
        d = self.device
        out = dict(obs=torch.empty((batch, OBS_DIM), dtype=obs_dtype, device=d),
                   action=torch.empty(batch, dtype=torch.uint8, device=d),
                   reward=torch.empty(batch, dtype=torch.float32, device=d),
                   done=torch.empty(batch, dtype=torch.uint8, device=d))
        if n_step > 1 or not mirror:
            out.update(discount=torch.empty(batch, dtype=torch.float32, device=d),
                       steps=torch.empty(batch, dtype=torch.uint8, device=d))
        if mirror:
            out["mirrored"] = torch.empty(batch, dtype=torch.uint8, device=d)
        if with_index or tree is not None:
            out["index"] = torch.empty(batch, dtype=torch.int64, device=d)
        if tree is not None:
            out["prob"] = torch.empty(batch, dtype=torch.float32, device=d)
        pa, pb = C.c_void_p(), C.c_void_p()
        from ._lib import check as env_check
        env_check(next_env._lib.tpl_state_ptrs(next_env._h, C.byref(pa), C.byref(pb)))
        ptr = lambda k: out[k].data_ptr() if k in out else None
        args = [self.data.data_ptr(), None if tree is None else tree.data_ptr(), self.capacity, self.size, self.head,
                self.stride or 1, n_step if "steps" in out else 0, gamma or 0.0, batch, int(seed) % (1 << 64),
                int(update) % (1 << 64), next_env.L, next_env.M, out["obs"].data_ptr(), _OBS_CODES[obs_dtype], pa.value, pb.value,
                ptr("action"), ptr("reward"), ptr("discount"), ptr("done"), ptr("steps"), ptr("index"), ptr("prob")]
        if mirror:
            check(_learn_lib.lib().tpl_replay_sample_mirror(*args, mirror, ptr("mirrored"), self._stream()))
        else:
            check(_learn_lib.lib().tpl_replay_sample_nstep(*args, self._stream()))
        return out

    def push(self, env: BatchedTetris, traj: dict) -> None:
        """Append the trajectory of env.actor_rollout(..., record=True, record_states=True), called just before: s' of the
        last step is read from the environment's resident planes."""
        if not env.auto_reset:
            raise ValueError("the replay ring takes transitions of an auto-reset environment (the state before a step must be a "
                             "running board)")
        actions, rewards, dones = traj["actions"], traj["rewards"], traj["dones"]
        sa, sb = traj["states_a"], traj["states_b"]
        steps, n = actions.shape
        if n != env.num_envs or tuple(sa.shape) != (steps, n, 4) or tuple(sb.shape) != (steps, n, 4):
            raise ValueError("the trajectory does not belong to this environment")
        if steps * n > self.capacity:
            raise ValueError(f"a chunk of {steps} x {n} transitions does not fit a ring of {self.capacity}")
        pa, pb = C.c_void_p(), C.c_void_p()
        from ._lib import check as env_check
        env_check(env._lib.tpl_state_ptrs(env._h, C.byref(pa), C.byref(pb)))
        dev = lambda t, dt: t.device == self.device and t.is_contiguous() and t.dtype in dt
        if not (dev(actions, (torch.uint8,)) and dev(rewards, (torch.float32,)) and dev(dones, (torch.uint8, torch.bool))
                and dev(sa, (torch.int32,)) and dev(sb, (torch.int32,))):
            raise ValueError("trajectory tensors must be contiguous device tensors as actor_rollout returns them")
        check(_learn_lib.lib().tpl_replay_push(self.data.data_ptr(), self.capacity, self.head, steps, n, actions.data_ptr(),
                                               rewards.data_ptr(), dones.data_ptr(), sa.data_ptr(), sb.data_ptr(), pa.value,
                                               pb.value, self._stream()))
        self.head = (self.head + steps * n) % self.capacity
        self.size = min(self.size + steps * n, self.capacity)
        self._track_push(env, n)

    def sample(self, batch: int, seed: int, update: int, next_env: BatchedTetris, obs_dtype=torch.float32,
               with_index: bool = False, n_step: int = 1, gamma: Optional[float] = None, mirror=False) -> dict:
        """One minibatch: draw i takes slot _learn_lib.replay_indices(seed, update, batch, size)[i].  Returns obs [batch, 217]
        (the observation of s, as env.expand_states makes it), action u8, reward f32, done u8 (and index i64); the s' planes
        are written into the resident state of `next_env`, an environment of exactly `batch` boards.

        n_step > 1 (gamma required): the n-step rule of include/tpl_learn.h (_learn_lib.nstep_targets restates it).  reward
        is then the return R, done and s' are those of the last record taken, and discount f32 (gamma^K, or 0 if done) and
        steps u8 (K) are added.

        mirror=True reflects each draw left to right on its coin (_learn_lib.mirror_coins), mirror="always" every draw: obs,
        the s' planes and action are those of the reflected transition (include/tpl_learn.h; _learn_lib.mirror_states,
        mirror_actions and MIRROR_OBS_PERM restate it), everything else is the plain draw's, and mirrored u8 [batch] is added."""
        mirror = _learn_lib.mirror_mode(mirror)
        n_step, gamma = self._nstep_args(n_step, gamma)
        if self.size < 1:
            raise ValueError("the replay ring is empty")
        if next_env.num_envs != batch or next_env.device != self.device:
            raise ValueError(f"next_env must hold exactly {batch} boards on {self.device}")
        if obs_dtype not in _OBS_CODES:
            raise ValueError("obs_dtype must be torch.float32 or torch.bfloat16")
        if n_step > 1 or mirror:
            return self._sample_nstep(None, batch, seed, update, next_env, obs_dtype, with_index, n_step, gamma, mirror)
        d = self.device
        out = dict(obs=torch.empty((batch, OBS_DIM), dtype=obs_dtype, device=d),
                   action=torch.empty(batch, dtype=torch.uint8, device=d),
                   reward=torch.empty(batch, dtype=torch.float32, device=d),
                   done=torch.empty(batch, dtype=torch.uint8, device=d))
        if with_index:
            out["index"] = torch.empty(batch, dtype=torch.int64, device=d)
        pa, pb = C.c_void_p(), C.c_void_p()
        from ._lib import check as env_check
        env_check(next_env._lib.tpl_state_ptrs(next_env._h, C.byref(pa), C.byref(pb)))
        idx = out.get("index")
        check(_learn_lib.lib().tpl_replay_sample(
            self.data.data_ptr(), self.capacity, self.size, batch, int(seed) % (1 << 64), int(update) % (1 << 64),
            next_env.L, next_env.M, out["obs"].data_ptr(), _OBS_CODES[obs_dtype], pa.value, pb.value,
            out["action"].data_ptr(), out["reward"].data_ptr(), out["done"].data_ptr(),
            None if idx is None else idx.data_ptr(), self._stream()))
        return out


class PrioritizedReplayRing(ReplayRing):
    """A ReplayRing with proportional prioritized draws (Schaul et al., 2016) from a 16-ary float64 sum tree that lives on the
    device next to the ring (layout and rules: include/tpl_learn.h; numpy mirror: _learn_lib.prioritized_draws and friends).

    push()               the ring push, then every pushed slot gets the running maximum priority (same stream)
    sample()             stratified proportional draws: as ReplayRing.sample, plus index i64 and prob f32 = p_slot / total
    update_priorities()  writes back priorities already shaped as (|delta| + eps)^alpha; refused after a push since the sample
    priorities(), total(), max_priority()   device views of the leaves, the root and the running maximum (no sync)"""

    def __init__(self, capacity: int, device):
        super().__init__(capacity, device)
        L = _learn_lib.lib()
        nbytes = L.tpl_priority_tree_bytes(self.capacity)
        self.tree = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.tree.data_ptr() % 128:
            raise RuntimeError("the priority tree must be 128-byte aligned")
        offsets, _, _ = _learn_lib.priority_layout(self.capacity)
        self._root = offsets[-1]
        check(L.tpl_priority_init(self.tree.data_ptr(), self.capacity, self._stream()))
        self.pushes = 0
        self._sampled_at = None                                  # self.pushes when the last minibatch was drawn

    def push(self, env: BatchedTetris, traj: dict) -> None:
        head = self.head
        super().push(env, traj)
        count = int(traj["actions"].numel())
        check(_learn_lib.lib().tpl_priority_push(self.tree.data_ptr(), self.capacity, head, count, self._stream()))
        self.pushes += 1

    def sample(self, batch: int, seed: int, update: int, next_env: BatchedTetris, obs_dtype=torch.float32, n_step: int = 1,
               gamma: Optional[float] = None, mirror=False) -> dict:
        """One minibatch of proportional draws: draw i takes the slot _learn_lib.prioritized_draws(tree, seed, update, batch)
        names.  Returns what ReplayRing.sample returns, with index i64 [batch] and prob f32 [batch]; n_step and gamma as
        there (the return, done, s', discount and steps of the n-step rule; index and prob stay the drawn slot's), and mirror
        as there (index and prob are the slot's, mirrored or not)."""
        mirror = _learn_lib.mirror_mode(mirror)
        n_step, gamma = self._nstep_args(n_step, gamma)
        if self.size < 1:
            raise ValueError("the replay ring is empty")
        if next_env.num_envs != batch or next_env.device != self.device:
            raise ValueError(f"next_env must hold exactly {batch} boards on {self.device}")
        if obs_dtype not in _OBS_CODES:
            raise ValueError("obs_dtype must be torch.float32 or torch.bfloat16")
        if n_step > 1 or mirror:
            out = self._sample_nstep(self.tree, batch, seed, update, next_env, obs_dtype, True, n_step, gamma, mirror)
            self._sampled_at = self.pushes
            return out
        d = self.device
        out = dict(obs=torch.empty((batch, OBS_DIM), dtype=obs_dtype, device=d),
                   action=torch.empty(batch, dtype=torch.uint8, device=d),
                   reward=torch.empty(batch, dtype=torch.float32, device=d),
                   done=torch.empty(batch, dtype=torch.uint8, device=d),
                   index=torch.empty(batch, dtype=torch.int64, device=d),
                   prob=torch.empty(batch, dtype=torch.float32, device=d))
        pa, pb = C.c_void_p(), C.c_void_p()
        from ._lib import check as env_check
        env_check(next_env._lib.tpl_state_ptrs(next_env._h, C.byref(pa), C.byref(pb)))
        check(_learn_lib.lib().tpl_replay_sample_prioritized(
            self.data.data_ptr(), self.tree.data_ptr(), self.capacity, self.size, batch, int(seed) % (1 << 64),
            int(update) % (1 << 64), next_env.L, next_env.M, out["obs"].data_ptr(), _OBS_CODES[obs_dtype], pa.value, pb.value,
            out["action"].data_ptr(), out["reward"].data_ptr(), out["done"].data_ptr(), out["index"].data_ptr(),
            out["prob"].data_ptr(), self._stream()))
        self._sampled_at = self.pushes
        return out

    def update_priorities(self, index: torch.Tensor, priority: torch.Tensor) -> None:
        """Write back the priorities of the last minibatch's draws: index i64 [B] as sample() returned it, priority [B] (cast to
        float64) = (|delta| + eps)^alpha.  Each is clamped to [1e-12, 1e30] (NaN -> 1e-12); a slot drawn twice takes the
        larger; an index outside [0, capacity) is ignored.  Raises ValueError if the ring was pushed since that sample: its slots may hold other transitions now."""
        if self._sampled_at is None:
            raise ValueError("update_priorities needs a sample() first")
        if self._sampled_at != self.pushes:
            raise ValueError("the ring was pushed since the minibatch was drawn: its priorities would land on overwritten slots")
        if index.dim() != 1 or priority.shape != index.shape or index.dtype != torch.int64:
            raise ValueError("index must be int64 [B] and priority [B]")
        if index.device != self.device or priority.device != self.device:
            raise ValueError(f"index and priority must be on {self.device}")
        if index.numel() < 1:
            raise ValueError("an empty write-back")
        index = index.contiguous()
        priority = priority.to(torch.float64).contiguous()
        check(_learn_lib.lib().tpl_priority_update(self.tree.data_ptr(), self.capacity, index.numel(), index.data_ptr(),
                                                   priority.data_ptr(), self._stream()))

    def _words(self) -> torch.Tensor:
        return self.tree.view(torch.float64)

    def priorities(self) -> torch.Tensor:
        """The leaf priorities, float64 [capacity] (a view of the tree: 0 for an unfilled slot)."""
        h = _learn_lib.PRIORITY_HEADER_WORDS
        return self._words()[h:h + self.capacity]

    def total(self) -> torch.Tensor:
        """The root: the sum of every priority, float64 [1] (a view of the tree)."""
        return self._words()[self._root:self._root + 1]

    def max_priority(self) -> torch.Tensor:
        """The running maximum priority that a push gives, float64 [1] (a view of the tree)."""
        return self._words()[0:1]


def factored_q(out: torch.Tensor, action: torch.Tensor) -> torch.Tensor:
    """Q(s, a) = out[a // 10] + out[4 + a % 10] for [B, 14] outputs and [B] actions."""
    a = action.long().unsqueeze(1)
    return (out.gather(1, a // 10) + out.gather(1, 4 + a % 10)).squeeze(1)


def factored_max(out: torch.Tensor) -> torch.Tensor:
    """max over the 40 actions of the factored Q: max(out[0:4]) + max(out[4:14])."""
    return out[:, :4].max(dim=1).values + out[:, 4:14].max(dim=1).values


class _TakesNStep(type):
    """DQNLearner(..., n_step=1, mirror=False): the class call takes the keyword-only options and checks them before __init__
    runs, so that __init__'s parameter list (its positional order, the prioritized options last) stays as it is."""

    def __call__(cls, *args, n_step: int = 1, mirror: bool = False, **kwargs):
        if isinstance(n_step, bool) or int(n_step) != n_step or not 1 <= int(n_step) <= _learn_lib.NSTEP_MAX:
            raise ValueError(f"n_step must be an integer in [1, {_learn_lib.NSTEP_MAX}]")
        if not isinstance(mirror, bool):
            raise ValueError("mirror must be False or True")
        self = cls.__new__(cls)
        self.n_step = int(n_step)
        self.mirror = mirror
        self.__init__(*args, **kwargs)
        return self


class DQNLearner(metaclass=_TakesNStep):
    """DQN for Model(217, 14) on a BatchedTetris (defaults: the constants of the upstream model/train.py).

    prioritized=True draws minibatches from a PrioritizedReplayRing (proportional, exponent alpha), weights the Huber loss
    per sample by importance-sampling weights (exponent beta, annealed to beta_final over beta_updates updates) and writes
    back (|q - y| + priority_eps)^alpha after each optimizer step.

    n_step=n in [1, 16] bootstraps from n-step returns drawn on the device (include/tpl_learn.h):
    y = R + discount * max Q'(s'), where R sums up to n rewards of one board discounted by gamma, the sum stops after a done,
    discount is gamma^K (0 after a done) and s' is the state K moves on.  As in Rainbow (Hessel et al., 2018) the return of
    epsilon-greedy data is not corrected for being off-policy.  n_step=1 is the 1-step target above, computed as before.

    mirror=True draws every minibatch with the mirror coin: about half of its transitions come reflected left to right (s, a
    and s'; the game is symmetric under it), so y and Q(s, a) are those of the reflected transition, and the minibatch gains
    `mirrored`.  Priorities are written back to the slot whichever way it was drawn.  mirror=False is every path as before.

    collect(steps)   one actor_rollout of the online net's split image at the scheduled epsilon, pushed into the ring
    update(n=1)      n minibatch updates (sample -> Q(s) in torch, Q'(s') on the split kernel -> Huber -> AdamW -> soft update)
    evaluate(steps)  the greedy policy (epsilon 0) on a separate environment over the same pool: episodes, wins, win rate;
                     lookahead=True plays the one-ply lookahead on the online net instead
    """

    def __init__(self, env: BatchedTetris, model: Optional[nn.Module] = None, capacity: int = 1 << 20, batch_size: int = 128,
                 gamma: float = 0.99, eps_start: float = 0.9, eps_end: float = 0.05, eps_decay: float = 1000,
                 tau: float = 0.005, lr: float = 1e-4, seed: int = 0, prioritized: bool = False, alpha: float = 0.6,
                 beta: float = 0.4, beta_final: float = 1.0, beta_updates: int = 100_000, priority_eps: float = 1e-6):
        # self.n_step, self.mirror: set and checked by the class call (_TakesNStep)
        if self.n_step > 1 and not 0.0 <= gamma <= 1.0:
            raise ValueError("n-step returns need gamma in [0, 1]")
        if not env.auto_reset:
            raise ValueError("DQNLearner needs an environment with auto_reset=True (the replay ring's s' of a finished "
                             "episode is the freshly reset board, masked by done)")
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        if prioritized and (alpha < 0 or beta_updates < 1 or priority_eps < 0):
            raise ValueError("prioritized replay needs alpha >= 0, beta_updates >= 1 and priority_eps >= 0")
        self.env, self.device = env, env.device
        self.batch_size, self.gamma, self.tau, self.lr = int(batch_size), float(gamma), float(tau), float(lr)
        self.eps_start, self.eps_end, self.eps_decay = float(eps_start), float(eps_end), float(eps_decay)
        self.seed = int(seed)
        self.model = (model if model is not None else PolicyMLP()).to(device=self.device, dtype=torch.float32)
        self.target = copy.deepcopy(self.model)                   # target_net.load_state_dict(policy_net.state_dict())
        for p in self.target.parameters():
            p.requires_grad_(False)
        self.optimizer = torch.optim.AdamW(self.model.parameters(), lr=self.lr, amsgrad=True)
        self.loss_fn = nn.SmoothL1Loss()
        self.prioritized = bool(prioritized)
        self.alpha, self.beta0, self.beta_final = float(alpha), float(beta), float(beta_final)
        self.beta_updates, self.priority_eps = int(beta_updates), float(priority_eps)
        self.ring = (PrioritizedReplayRing if self.prioritized else ReplayRing)(capacity, self.device)
        # the target network's boards: s' of each draw is written into this environment's resident planes
        self.next_env = BatchedTetris(env.L, env.M, self.batch_size, device=self.device, seed=self.seed)
        self.actor_image = pack_policy_device(_learn_lib.policy_tensors(self.model), "split")
        self.target_image = pack_policy_device(_learn_lib.policy_tensors(self.target), "split")
        self._next_action = torch.empty(self.batch_size, dtype=torch.uint8, device=self.device)
        self._next_q = torch.empty((self.batch_size, 14), dtype=torch.float32, device=self.device)
        self.steps_done = 0
        self.updates = 0
        self.last = None                                         # the last update's minibatch, Q'(s'), y and Q(s, a)
        self.eval_env = None

    # ------------------------------------------------------------------------------------------ acting
    def epsilon(self) -> float:
        return self.eps_end + (self.eps_start - self.eps_end) * math.exp(-self.steps_done / self.eps_decay)

    def collect(self, steps: int) -> dict:
        """`steps` lockstep iterations of the whole batch under the online net at the scheduled epsilon, appended to the
        ring (steps * N transitions).  Returns the recorded trajectory (device tensors) and the epsilon used."""
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be positive")
        if steps * self.env.num_envs > self.ring.capacity:
            raise ValueError(f"collect({steps}) adds {steps * self.env.num_envs} transitions, more than the ring's capacity "
                             f"{self.ring.capacity}")
        eps = self.epsilon()
        pack_policy_device(_learn_lib.policy_tensors(self.model), "split", out=self.actor_image)
        traj = self.env.actor_rollout(self.actor_image, steps, epsilon=eps, seed=self.seed, step0=self.steps_done,
                                      record=True, record_states=True)
        self.ring.push(self.env, traj)
        self.steps_done += steps
        traj["epsilon"] = eps
        return traj

    # ------------------------------------------------------------------------------------------ learning
    def update(self, n: int = 1) -> float:
        """n optimisation steps of the tutorial's optimize_model; returns the last loss."""
        if self.ring.size < self.batch_size:
            raise ValueError(f"the ring holds {self.ring.size} transitions, fewer than batch_size={self.batch_size}: collect first")
        loss = None
        for _ in range(int(n)):
            loss = self._update_once()
        return float(loss)

    def beta(self) -> float:
        """The importance-sampling exponent of the next update: beta annealed linearly to beta_final over beta_updates."""
        return self.beta0 + (self.beta_final - self.beta0) * min(1.0, self.updates / self.beta_updates)

    @torch.no_grad()
    def minibatch(self) -> dict:
        """The next update's minibatch (draws keyed by (seed, updates)) with Q'(s') of the target image and the TD target y;
        s' stays in next_env's resident planes.

        Prioritized: also prob (of each draw) and weight, the importance-sampling weight (size * prob)^-beta divided by the
        largest weight IN THE MINIBATCH (Dopamine's convention, chosen over Schaul et al.'s division by the weight of the
        globally smallest priority so that no min-tree is needed), float32."""
        nstep = dict(n_step=self.n_step, gamma=self.gamma) if self.n_step > 1 else {}
        if self.mirror:
            nstep["mirror"] = True
        if self.prioritized:
            batch = self.ring.sample(self.batch_size, self.seed, self.updates, self.next_env, **nstep)
            w = (self.ring.size * batch["prob"].double()).pow(-self.beta())
            batch["weight"] = (w / w.max()).float()
        else:
            batch = self.ring.sample(self.batch_size, self.seed, self.updates, self.next_env, with_index=True, **nstep)
        self.next_env.policy_act(self.target_image, out=self._next_action, logits=self._next_q)
        next_q = self._next_q.clone()
        if self.n_step > 1:                                      # reward: the n-step return; discount: gamma^K, 0 after a done
            y = batch["reward"] + batch["discount"] * factored_max(next_q)
        else:
            y = batch["reward"] + self.gamma * (1.0 - batch["done"].float()) * factored_max(next_q)
        return dict(batch, next_q=next_q, y=y)

    def _update_once(self) -> torch.Tensor:
        batch = self.minibatch()
        y = batch["y"]
        q = factored_q(self.model(batch["obs"]), batch["action"])
        if self.prioritized:
            loss = (batch["weight"] * nn.functional.smooth_l1_loss(q, y, reduction="none")).mean()
        else:
            loss = self.loss_fn(q, y)
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(self.model.parameters(), 100)
        self.optimizer.step()
        if self.prioritized:                                    # (|delta| + eps)^alpha of this update's forward pass
            self.ring.update_priorities(batch["index"], ((q - y).detach().double().abs() + self.priority_eps).pow(self.alpha))
        self.soft_update()
        self.updates += 1
        self.last = dict(batch, q=q.detach())
        return loss.detach()

    @torch.no_grad()
    def soft_update(self) -> None:
        """theta' <- tau * theta + (1 - tau) * theta', then the target image repacked on the device."""
        for pt, p in zip(self.target.parameters(), self.model.parameters()):
            pt.copy_(p * self.tau + pt * (1 - self.tau))
        pack_policy_device(_learn_lib.policy_tensors(self.target), "split", out=self.target_image)

    # ------------------------------------------------------------------------------------------ evaluation
    def evaluate(self, steps: int, epsilon: float = 0.0, lookahead: bool = False) -> dict:
        """`steps` iterations of the online net's policy (greedy by default) on a separate auto-reset environment with the
        learner env's size, L, M and configuration pool, from a full reset.  Returns episodes finished, wins, win rate.

        lookahead=True plays the one-ply lookahead on the online net instead of its factored arg-max (lookahead.LookaheadPolicy
        at the learner's gamma: every distinct placement scored as reward + gamma * (1 - done) * max Q(afterstate)), one step
        per iteration; it is deterministic, so it takes no epsilon."""
        if lookahead and epsilon != 0:
            raise ValueError("evaluate(lookahead=True) is greedy: epsilon must be 0")
        env = self.env
        if env._pool is None:
            raise ValueError("the learner's environment has no configuration pool to evaluate on")
        if self.eval_env is None:
            self.eval_env = BatchedTetris(env.L, env.M, env.num_envs, device=self.device, seed=env.seed + 1, auto_reset=True,
                                          assign=env.assign, reward=env.reward_params)
        ev = self.eval_env
        if getattr(self, "_eval_pool", None) is not env._pool:
            ev.load_configs(*env._pool, validate=False)
            self._eval_pool = env._pool
        ev.reset()
        image = pack_policy_device(_learn_lib.policy_tensors(self.model), "split")
        if lookahead:
            from .lookahead import LookaheadPolicy
            policy = getattr(self, "_lookahead", None)
            if policy is None:
                policy = self._lookahead = LookaheadPolicy(ev, image, gamma=self.gamma)
            policy.image = image
            action = torch.empty(ev.num_envs, dtype=torch.uint8, device=self.device)
            reward = torch.empty(ev.num_envs, dtype=torch.float32, device=self.device)
            done = torch.empty(ev.num_envs, dtype=torch.uint8, device=self.device)
            for _ in range(int(steps)):
                ev.step_into(policy.act(out=action), reward, done)
        else:
            ev.actor_rollout(image, int(steps), epsilon=float(epsilon), seed=self.seed + 1, record=False)
        st = ev.stats()
        return dict(episodes=st["episodes"], wins=st["wins"], win_rate=st["wins"] / max(st["episodes"], 1))
